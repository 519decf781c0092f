"""GPU: the split-bf16 MFMA kernels one product at a time (tests/split_probe.py).  Inputs for which every output is a SINGLE product
hi_w * hi_x + hi_w * lo_x + lo_w * hi_x, so the expected value is exact by construction and the check is per output, on every output,
to 2 * 2^-23 * (|hh| + |hl| + |lh|); an output whose expected value is exactly zero must be 0.0.  A dropped lo * hi term, a weight row
of the neighbouring tap or a lo plane paired with the wrong hi is outside that at 99.99 % of the outputs it touches
(tests/test_split_probe_cpu.py), where the max-norm tests on dense data cannot see it.  Second check, on dense data: scaling input
channel c by 2^e(c) and its weights by 2^-e(c) leaves every product and every partial sum unchanged, so the output must be
bit-identical.  Every test prints the largest error-to-tolerance ratio it saw."""
import numpy as np
import pytest
import torch

import packed_layout as P
import split_probe as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from geometric_aware_dense_matching_amd import ops as o
    return o


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _report(name, ratio):
    print("split probe %s: largest error / tolerance %.3f" % (name, ratio))


@pytest.mark.parametrize("B,Cin,Cout,H,W,stride", S.CONV3X3_SHAPES)
def test_conv3x3_one_product_per_output(ops, B, Cin, Cout, H, W, stride):
    """conv3x3_bf16x3 on the lattice rounds: Cin = 64 (the half-filled chunk), Cout = 200 (masked output rows), Cin = 256 (two chunks per
    tap: the panel switch), stride 2; image corners and edges and the first and last pixel of every wave's and workgroup's tile are
    among the outputs.  The first round also goes in as a PackedAct packed in numpy (same bits out), and comes out packed where the
    kernel takes that (decoded: hi + lo of every output == the split of the fp32 output)."""
    p = S.LatticeConv(B, Cin, Cout, H, W, stride=stride, seed=Cin + Cout)
    wpk = ops.conv3x3_pack_weight(_cuda(p.w))
    worst = 0.0
    for r in range(len(p.rounds)):
        x = p.x(r)
        got = ops.conv3x3_bf16x3(_cuda(x), wpk, Cout, stride=stride)
        exp, tol = p.expected(r)
        worst = max(worst, S.check(got.cpu().numpy(), exp, tol, "conv3x3 %s round %d" % ((B, Cin, Cout, H, W, stride), r)))
        if r == 0:
            xp = ops.PackedAct(_cuda(P.pack(x)), x.shape)
            assert torch.equal(ops.conv3x3_bf16x3(xp, wpk, Cout, stride=stride), got)
            if Cout % 128 == 0:
                f32, opk = ops.conv3x3_bf16x3(_cuda(x), wpk, Cout, stride=stride, out_packed=True)
                assert torch.equal(f32, got) and opk.shape == tuple(got.shape)
                OH, OW = got.shape[2:]
                off = P.granule_offsets(B, Cout, OH, OW) // 2                   # [B, Cout / 8, OH, OW, 2] in bf16 elements
                buf = opk.buf.cpu().numpy().view(np.uint16)
                dec = [S.bf16_to_f64(buf[off[..., k, None] + np.arange(8)]).transpose(0, 1, 4, 2, 3).reshape(B, Cout, OH, OW) for k in range(2)]
                hi, lo = S.parts(got.cpu().numpy())
                assert np.array_equal(dec[0] + dec[1], hi + lo) and np.array_equal(dec[0], hi)
    _report("conv3x3_bf16x3 %s" % ((B, Cin, Cout, H, W, stride),), worst)


def test_conv3x3_train_input_gradient_one_product_per_output(ops):
    """The backward of conv3x3_train: the input gradient is the convolution of grad_out with the flipped, transposed filter, whose rows
    conv_pack_weight_dgrad writes straight from the forward weight; grad_out on the lattice."""
    B, Cin, Cout, H, W = S.DGRAD_SHAPE
    p = S.LatticeConv(B, Cout, Cin, H, W, seed=7)                                  # p.w is the dgrad filter [Cin, Cout, 3, 3]
    w = _cuda(S.dgrad_filter(p.w))                                                # the forward weight [Cout, Cin, 3, 3] it belongs to
    assert np.array_equal(S.dgrad_filter(w.cpu().numpy()), p.w)
    worst = 0.0
    for r in range(len(p.rounds)):
        x = torch.zeros(B, Cin, H, W, device="cuda", requires_grad=True)
        assert ops.conv3x3_train_supported(x, w)
        ops.conv3x3_train(x, w).backward(_cuda(p.x(r)))
        exp, tol = p.expected(r)
        worst = max(worst, S.check(x.grad.cpu().numpy(), exp, tol, "conv3x3_train dgrad round %d" % r))
    _report("conv3x3_train input gradient %s" % (S.DGRAD_SHAPE,), worst)


@pytest.mark.parametrize("B,Cin,Cout,n", S.GEMM_SHAPES)
def test_gemm_one_product_per_output(ops, B, Cin, Cout, n):
    p = S.OneHotGemm(B, Cin, Cout, n, seed=n)
    wpk = ops.gemm_pack_weight(_cuda(p.w))
    exp, tol = p.expected()
    x = _cuda(p.x())
    worst = S.check(ops.gemm_bf16x3(x, wpk, Cout).cpu().numpy(), exp, tol, "gemm_bf16x3 %s" % ((B, Cin, Cout, n),))
    if Cin != 64:        # the 64-channel (half-chunk) form is built for NCHW output only
        got_pm = ops.gemm_bf16x3(x, wpk, Cout, pixel_major=True).cpu().view(B, n, Cout).transpose(1, 2).numpy()
        worst = max(worst, S.check(got_pm, exp, tol, "gemm_bf16x3 pixel-major %s" % ((B, Cin, Cout, n),)))
    _report("gemm_bf16x3 %s" % ((B, Cin, Cout, n),), worst)


@pytest.mark.parametrize("stride", [1, 2])
def test_conv1x1_packed2d_one_product_per_output(ops, stride):
    """The 1x1 convolution on a packed map, stride 1 and 2: the pixels it must not read at stride 2 are dense in every channel."""
    B, Cin, Cout, H, W = S.CONV1X1_2D_SHAPE
    OH, OW = H // stride, W // stride
    p = S.OneHotGemm(B, Cin, Cout, OH * OW, seed=stride)
    xp = ops.conv3x3_pack_act(_cuda(p.x_map(H, W, stride)))
    got = ops.conv1x1_packed2d(xp, ops.gemm_pack_weight(_cuda(p.w)), Cout, stride=stride)
    exp, tol = p.expected()
    _report("conv1x1_packed2d stride %d" % stride, S.check(got.cpu().numpy().reshape(B, Cout, OH * OW), exp, tol, "conv1x1_packed2d stride %d" % stride))


def test_conv64_fusion_tail_one_product_per_output(ops):
    """conv64_gather_add_act_mfma with a zero point term, scale 1, shift 0, no activation: ragged m, both layouts."""
    B, m = S.CONV64_SHAPE
    n = 37
    p = S.OneHotGemm(B, 64, 64, m, seed=m)
    wpk = ops.pack_rows64(_cuda(p.w))
    t = torch.zeros(B, 64, n, device="cuda")
    idx = torch.from_numpy(np.random.RandomState(0).randint(0, n, (B, m)).astype(np.int32)).cuda()
    one, zero = torch.ones(64, device="cuda"), torch.zeros(64, device="cuda")
    exp, tol = p.expected()
    x = _cuda(p.x())
    got = ops.conv64_gather_add_act_mfma(x, wpk, t, idx, one, zero, ops.ACT_NONE, 0.0).cpu().numpy()
    got_pm = ops.conv64_gather_add_act_mfma(x, wpk, t, idx, one, zero, ops.ACT_NONE, 0.0, pixel_major=True).cpu().numpy()
    assert got_pm.shape == (B, m, 64)
    worst = max(S.check(got, exp, tol, "conv64_gather_add_act_mfma"), S.check(got_pm.transpose(0, 2, 1), exp, tol, "conv64_gather_add_act_mfma pixel-major"))
    _report("conv64_gather_add_act_mfma", worst)


@pytest.mark.parametrize("B,Cin,Cout,H,W,parts", S.WGRAD3X3_SHAPES)
def test_conv3x3_wgrad_one_product_per_output(ops, B, Cin, Cout, H, W, parts):
    p = S.OneHotWgrad(B, Cin, Cout, H, W, taps=9, seed=Cin + B)
    x, go = _cuda(p.x()), _cuda(p.go)
    assert ops.conv3x3_wgrad_supported(x, go)
    exp, tol = p.expected()
    assert p.nzero > 0
    got = ops.conv3x3_wgrad(x, go, parts=parts)
    _report("conv3x3_wgrad %s" % ((B, Cin, Cout, H, W, parts),), S.check(got.cpu().numpy(), exp, tol, "conv3x3_wgrad parts %r" % (parts,)))


def test_conv3x3_wgrad_refuses_two_parts_of_one_chunk(ops):
    """A [1, ., 4, 32] map is one 128-pixel chunk of the contraction: no K split in two exists for it."""
    B, Cin, Cout, H, W, _ = S.WGRAD3X3_SHAPES[0]
    with pytest.raises(ValueError, match="parts do not divide"):
        ops.conv3x3_wgrad(torch.zeros(B, Cin, H, W, device="cuda"), torch.zeros(B, Cout, H, W, device="cuda"), parts=2)


def test_gemm_wgrad_one_product_per_output(ops):
    B, Cin, Cout, npix = S.WGRAD1X1_SHAPE
    p = S.OneHotWgrad(B, Cin, Cout, npix // 32, 32, taps=1, seed=3)
    got = ops.gemm_wgrad(_cuda(p.x().reshape(B, Cin, npix)), _cuda(p.go.reshape(B, Cout, npix)))
    exp, tol = p.expected()
    _report("gemm_wgrad %s" % (S.WGRAD1X1_SHAPE,), S.check(got.cpu().numpy(), exp[:, :, 0, 0], tol[:, :, 0, 0], "gemm_wgrad"))


def test_stem_one_product_per_output(ops):
    """The stem on a lattice of pitch 7 with scale 1 and shift 0; the expected value goes through its ReLU and max-pool in numpy."""
    B, C, H, W = S.STEM_SHAPE
    p = S.LatticeStem(B, H, W, seed=5)
    wpk = ops.stem_pack_weight(_cuda(p.w))
    one, zero = torch.ones(64, device="cuda"), torch.zeros(64, device="cuda")
    worst = 0.0
    for r in range(len(p.rounds)):
        got = ops.stem(_cuda(p.x(r)), wpk, one, zero)
        exp, tol = p.expected(r)
        worst = max(worst, S.check(got.cpu().numpy(), exp, tol, "stem round %d" % r))
    _report("stem", worst)


@pytest.mark.parametrize("prec", [S.MATCH_BF16X3, S.MATCH_F32])
def test_match_packed_sim_one_product_per_output(ops, prec):
    """match_packed(return_sim=True): the scene descriptor of point n is one-hot in channel n mod 128, the model is dense; the operands
    are decoded from the rows match_pack wrote, so its normalisation is part of the input.  Normalised one-hot rows are +-1 (their lo
    part is zero): a second run takes scene rows written in numpy without normalisation, whose hi and lo are both live."""
    B, N, M = S.MATCH_SHAPE
    assert (ops.MATCH_BF16X3, ops.MATCH_F32) == (S.MATCH_BF16X3, S.MATCH_F32)
    scene, model = S.match_inputs(B, N, M, seed=M)
    mrows = ops.match_pack(_cuda(model), prec)
    worst = []
    for srows in (ops.match_pack(_cuda(scene), prec), _cuda(S.encode_match_rows(scene[0].T, prec))):
        sim = ops.match_packed(srows, mrows, B, N, M, prec, return_sim=True)[2]
        exp, tol = S.match_expected(srows.cpu().numpy(), mrows.cpu().numpy(), N, prec)
        worst.append(S.check(sim[0].cpu().numpy(), exp, tol, "match_packed precision %d" % prec))
    _report("match_packed precision %d (rows of match_pack, rows written in numpy)" % prec, max(worst))


def _pow2(e):
    return torch.from_numpy(2.0 ** np.asarray(e, np.float64)).float().cuda()


def test_conv3x3_is_invariant_under_power_of_two_channel_scales(ops):
    """Dense data at mixed magnitudes: x[:, c] * 2^e(c) with w[:, c] * 2^-e(c) is the same convolution bit for bit -- powers of two commute
    with the split, with the exact bf16 products and with every fp32 addition.  Anything magnitude-dependent in the packing or the K loop
    breaks it."""
    B, Cin, Cout, H, W = 2, 256, 200, 8, 32
    g = torch.Generator(device="cpu").manual_seed(1)
    x, w = torch.randn(B, Cin, H, W, generator=g).cuda(), (torch.randn(Cout, Cin, 3, 3, generator=g) / 48).cuda()
    s = _pow2(S.rescale_exponents(Cin, 1))
    want = ops.conv3x3_bf16x3(x, ops.conv3x3_pack_weight(w), Cout)
    got = ops.conv3x3_bf16x3(x * s.view(1, -1, 1, 1), ops.conv3x3_pack_weight(w / s.view(1, -1, 1, 1)), Cout)
    assert want.abs().max().item() > 0 and torch.equal(got, want)


def test_gemm_is_invariant_under_power_of_two_channel_scales(ops):
    B, Cin, Cout, n = 2, 128, 200, 256
    g = torch.Generator(device="cpu").manual_seed(2)
    x, w = torch.randn(B, Cin, n, generator=g).cuda(), (torch.randn(Cout, Cin, generator=g) / 11).cuda()
    s = _pow2(S.rescale_exponents(Cin, 2))
    for pm in (False, True):
        want = ops.gemm_bf16x3(x, ops.gemm_pack_weight(w), Cout, pixel_major=pm)
        got = ops.gemm_bf16x3(x * s.view(1, -1, 1), ops.gemm_pack_weight(w / s.view(1, -1)), Cout, pixel_major=pm)
        assert want.abs().max().item() > 0 and torch.equal(got, want)


def test_conv64_fusion_tail_is_invariant_under_power_of_two_channel_scales(ops):
    """With its point term, folded BatchNorm and activation live: they see the same accumulator."""
    B, m, n = 2, 1000, 37
    g = torch.Generator(device="cpu").manual_seed(3)
    x, w = torch.randn(B, 64, m, generator=g).cuda(), (torch.randn(64, 64, generator=g) / 8).cuda()
    t = torch.randn(B, 64, n, generator=g).cuda()
    idx = torch.randint(0, n, (B, m), generator=g, dtype=torch.int32).cuda()
    scale, shift = (torch.rand(64, generator=g) + 0.5).cuda(), torch.randn(64, generator=g).cuda()
    s = _pow2(S.rescale_exponents(64, 3))
    want = ops.conv64_gather_add_act_mfma(x, ops.pack_rows64(w), t, idx, scale, shift, ops.ACT_RELU, 0.0)
    got = ops.conv64_gather_add_act_mfma(x * s.view(1, -1, 1), ops.pack_rows64(w / s.view(1, -1)), t, idx, scale, shift, ops.ACT_RELU, 0.0)
    assert want.abs().max().item() > 0 and torch.equal(got, want)


def test_weight_gradients_are_invariant_under_power_of_two_channel_scales(ops):
    """conv3x3_wgrad (K split in two) and gemm_wgrad: x[:, c] * 2^e(c) scales column c of the gradient by 2^e(c), exactly."""
    g = torch.Generator(device="cpu").manual_seed(4)
    B, Cin, Cout, H, W = 2, 256, 8, 4, 32
    x, go = torch.randn(B, Cin, H, W, generator=g).cuda(), torch.randn(B, Cout, H, W, generator=g).cuda()
    s = _pow2(S.rescale_exponents(Cin, 4))
    want = ops.conv3x3_wgrad(x, go, parts=2)
    got = ops.conv3x3_wgrad(x * s.view(1, -1, 1, 1), go, parts=2) / s.view(1, -1, 1, 1)
    assert want.abs().max().item() > 0 and torch.equal(got, want)
    x3, go3 = x.view(B, Cin, H * W), go.view(B, Cout, H * W)
    want = ops.gemm_wgrad(x3, go3)
    got = ops.gemm_wgrad(x3 * s.view(1, -1, 1), go3) / s.view(1, -1)
    assert want.abs().max().item() > 0 and torch.equal(got, want)
