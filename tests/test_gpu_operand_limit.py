"""GPU: the highest operand offsets the 2 GiB guard admits are computed correctly.  Every site of the convolution / GEMM kernel
(csrc/gdm_conv.hip conv_mfma16_kernel, 32-bit byte offsets into both packed operands) runs ONE shape just under the limit and is compared
with an fp64 restatement on the images (rows, columns) that lie nearest the end of the packed buffer, at the sibling tests' tolerances:
outputs 2e-5 * max(1, max|ref|) (test_gemm_bf16x3, test_conv3x3_bf16x3_vs_fp32_conv), weight gradients relative L2 3e-5 and max 1e-4 of
the gradient's scale (test_conv3x3_weight_gradient_on_the_mfma_gemm_equals_autograd).

Each comparison is also made against a reference whose highest image (highest 1 % of vertices) was zeroed -- what offsets that wrapped
would read -- and must FAIL there: the test would notice the failure it exists for.  No shape at or past the limit is launched; that side
is the refusals of tests/test_operand_limit_cpu.py and of the last test here."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LIMIT = 2 ** 31


@pytest.fixture(scope="module")
def ops():
    from geometric_aware_dense_matching_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _peak_memory_of_the_module():
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    print("\noperand-limit tests: peak GPU memory %.2f GiB" % (torch.cuda.max_memory_allocated() / 2 ** 30))
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _own_pool(ops):
    """The 2 GiB operand buffers live in a pool of the test's own and leave with it."""
    with ops.buffer_pool(ops.BufferPool()):
        yield
    torch.cuda.empty_cache()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device="cuda")


def _close(got, ref):
    """The output tests' comparison: max |got - ref| < 2e-5 * max(1, max |ref|)."""
    err = (got.double() - ref).abs().max().item()
    tol = 2e-5 * max(1.0, ref.abs().max().item())
    print("max err %.3e, bound %.3e" % (err, tol))
    return err < tol


def _grad_close(got, ref):
    """The weight-gradient tests' comparison: relative L2 3e-5 and max 1e-4 of the gradient's scale."""
    d = got.double() - ref
    l2, mx = d.norm().item() / ref.norm().item(), d.abs().max().item() / ref.abs().max().item()
    print("relative L2 %.3e (bound 3e-5), max %.3e of the scale (bound 1e-4)" % (l2, mx))
    return l2 < 3e-5 and mx < 1e-4


def test_gemm_of_many_images(ops):
    B, Cin, n, Cout = 32, 64, 43680, 128
    assert B * 3 * (n + 2) * 512 == 2147057664 < LIMIT
    g = _gen(1)
    x = _randn(g, B, Cin, n)
    w = _randn(g, Cout, Cin) / Cin ** 0.5
    got = ops.gemm_bf16x3(x, ops.gemm_pack_weight(w), Cout)
    assert got.shape == (B, Cout, n)
    imgs = [0, 15, 30, 31]
    ref = torch.matmul(w.double(), x[imgs].double())
    assert _close(got[imgs], ref)
    ref[-1] = 0                                                     # image 31 read as zeros
    assert not _close(got[imgs], ref)


@pytest.mark.parametrize("pixel_major", [False, True])
def test_gemm_of_two_long_images(ops, pixel_major):
    B, Cin, n, Cout = 2, 128, 699040, 128
    assert B * 3 * (n + 2) * 512 == 2147457024 < LIMIT
    g = _gen(2)
    x = _randn(g, B, Cin, n)
    w = _randn(g, Cout, Cin) / Cin ** 0.5
    got = ops.gemm_bf16x3(x, ops.gemm_pack_weight(w), Cout, pixel_major=pixel_major)
    if pixel_major:
        assert got.shape == (B * n, Cout)
        got = got.view(B, n, Cout).transpose(1, 2)
    cols = torch.cat([torch.arange(4096, device="cuda"), torch.arange(n - 4096, n, device="cuda"),
                      torch.randint(0, n, (4096,), generator=g, device="cuda")])
    xs = x[:, :, cols].double()
    ref = torch.matmul(w.double(), xs)
    assert _close(got[:, :, cols], ref)
    xs[1] = 0                                                       # the second image read as zeros
    assert not _close(got[:, :, cols], torch.matmul(w.double(), xs))


@pytest.fixture(scope="module")
def conv_case(ops):
    """x [962, 64, 64, 64] -> 64 channels with scale, shift, ReLU and residual; the fp64 reference of images 0, 480, 960, 961 (on the CPU,
    as test_conv3x3_bf16x3_vs_fp32_conv computes it), computed once."""
    B, C, H, W = 962, 64, 64, 64
    assert B * (H + 2) * (W + 2) * 512 == 2145521664 < LIMIT
    g = _gen(3)
    w = _randn(g, C, C, 3, 3) / (9 * C) ** 0.5
    sc, sh = torch.rand(C, generator=g, device="cuda") + 0.5, 0.1 * _randn(g, C)
    imgs = [0, 480, 960, 961]

    def make():                                                     # (the big tensors are made per test and leave with it)
        gg = _gen(4)
        return _randn(gg, B, C, H, W), _randn(gg, B, C, H, W)

    x, res = make()

    def reference(xi):
        y = torch.nn.functional.conv2d(xi.double().cpu(), w.double().cpu(), padding=1)
        y = y * sc.double().cpu().view(1, -1, 1, 1) + sh.double().cpu().view(1, -1, 1, 1) + res[imgs].double().cpu()
        return torch.relu(y).cuda()

    xi = x[imgs].clone()
    ref = reference(xi)
    xi[-1] = 0                                                      # image 961 read as zeros
    ref_zeroed = reference(xi)
    del x, res
    return dict(make=make, w=w, sc=sc, sh=sh, imgs=imgs, ref=ref, ref_zeroed=ref_zeroed, C=C)


def test_conv3x3_with_scale_shift_relu_and_residual(ops, conv_case):
    c = conv_case
    x, res = c["make"]()
    got = ops.conv3x3_bf16x3(x, ops.conv3x3_pack_weight(c["w"]), c["C"], c["sc"], c["sh"], ops.ACT_RELU, res)
    assert got.shape == x.shape
    assert _close(got[c["imgs"]], c["ref"])
    assert not _close(got[c["imgs"]], c["ref_zeroed"])


def test_conv3x3_packed_output_is_the_pack_of_its_fp32_output(ops, conv_case):
    c = conv_case
    x, res = c["make"]()
    got, opk = ops.conv3x3_bf16x3(x, ops.conv3x3_pack_weight(c["w"]), c["C"], c["sc"], c["sh"], ops.ACT_RELU, res, out_packed=True)
    assert _close(got[c["imgs"]], c["ref"])
    del x, res
    written = opk.buf.clone()                                        # (the pack below may reuse the pooled buffer)
    assert torch.equal(written, ops.conv3x3_pack_act(got).buf)


def test_stride_2_convolution_and_downsample_on_one_packed_map(ops):
    B, C, H, W = 248, 64, 128, 128
    assert B * (H + 2) * (W + 2) * 512 == 2145894400 < LIMIT
    g = _gen(5)
    x = _randn(g, B, C, H, W)
    w3 = _randn(g, C, C, 3, 3) / (9 * C) ** 0.5
    w1 = _randn(g, C, C) / C ** 0.5
    xp = ops.conv3x3_pack_act(x)
    got3 = ops.conv3x3_bf16x3(xp, ops.conv3x3_pack_weight(w3), C, stride=2)
    got1 = ops.conv1x1_packed2d(xp, ops.gemm_pack_weight(w1), C, stride=2)
    assert got3.shape == got1.shape == (B, C, H // 2, W // 2)
    imgs = [0, 124, 247]
    xi = x[imgs].double().cpu()
    for zero_last in (False, True):
        if zero_last:
            xi[-1] = 0                                              # image 247 read as zeros
        ref3 = torch.nn.functional.conv2d(xi, w3.double().cpu(), stride=2, padding=1).cuda()
        ref1 = torch.nn.functional.conv2d(xi, w1.double().cpu().view(C, C, 1, 1), stride=2).cuda()
        assert _close(got3[imgs], ref3) != zero_last
        assert _close(got1[imgs], ref1) != zero_last


def test_grouped_gemm_gathers_the_highest_vertices(ops):
    Cin, M, R = 128, 1398080, 256
    assert 3 * (M + 2) * 512 == 2147453952 < LIMIT
    g = _gen(6)
    x = _randn(g, 1, Cin, M)
    w = _randn(g, 128, Cin) / Cin ** 0.5
    top = M - M // 100                                               # the last 1 % of the vertices
    rowidx = torch.cat([torch.tensor([0, M - 1], device="cuda"),
                        torch.randint(top, M, (127,), generator=g, device="cuda"),
                        torch.randint(0, M, (127,), generator=g, device="cuda")]).to(torch.int32)
    assert rowidx.shape[0] == R and 0 <= int(rowidx.min()) and int(rowidx.max()) == M - 1
    tile_co0 = torch.zeros(R // 256, dtype=torch.int32, device="cuda")
    got = ops.gemm_grouped(x, ops.gemm_pack_weight(w), rowidx, tile_co0, 128)
    assert got.shape == (R, 128)
    xs = x[0][:, rowidx.long()].double()                             # [Cin, R]
    ref = torch.matmul(w.double(), xs).t()
    assert _close(got, ref)
    xs[:, rowidx.long() >= top] = 0                                  # the last 1 % read as zeros
    assert not _close(got, torch.matmul(w.double(), xs).t())


def _conv3x3_wgrad_fp64(x, go):
    """dW[co,ci,ky,kx] = sum_{b,y,x} go[b,co,y,x] * x[b,ci,y+ky-1,x+kx-1] in fp64, a few images at a time."""
    B, Cin, H, W = x.shape
    dw = torch.zeros(go.shape[1], Cin, 3, 3, dtype=torch.float64, device=x.device)
    for b0 in range(0, B, 8):
        xp = torch.nn.functional.pad(x[b0:b0 + 8].double(), (1, 1, 1, 1))
        gd = go[b0:b0 + 8].double()
        for ky in range(3):
            for kx in range(3):
                dw[:, :, ky, kx] += torch.einsum("bohw,bihw->oi", gd, xp[:, :, ky:ky + H, kx:kx + W])
    return dw


@pytest.fixture(scope="module")
def wgrad_case():
    B, Cin, H, W, Cout = 46, 256, 64, 64, 8
    assert B * H * W * (Cin + 2) * 44 == 2138898432 < LIMIT
    g = _gen(7)
    go = _randn(g, B, Cout, H, W)

    def make():
        return _randn(_gen(8), B, Cin, H, W)

    x = make()
    ref = _conv3x3_wgrad_fp64(x, go)
    ref_zeroed = ref - _conv3x3_wgrad_fp64(x[-1:], go[-1:])           # image 45 read as zeros
    del x
    return dict(make=make, go=go, ref=ref, ref_zeroed=ref_zeroed)


@pytest.mark.parametrize("parts", [None, 1])
def test_conv3x3_weight_gradient(ops, wgrad_case, parts):
    c = wgrad_case
    x = c["make"]()
    assert ops.conv3x3_wgrad_supported(x, c["go"])
    got = ops.conv3x3_wgrad(x, c["go"], parts=parts)
    assert got.shape == c["ref"].shape
    assert _grad_close(got, c["ref"])
    assert not _grad_close(got, c["ref_zeroed"])


def test_weight_gradient_of_a_1x1_product(ops):
    B, Cin, P, Cout = 42, 256, 16384, 64
    assert B * P * (Cin + 2) * 12 == 2130444288 < LIMIT
    g = _gen(9)
    x = _randn(g, B, Cin, P)
    go = _randn(g, B, Cout, P)
    got = ops.gemm_wgrad(x, go)
    per_image = torch.bmm(go.double(), x.double().transpose(1, 2))
    ref = per_image.sum(0)
    assert got.shape == ref.shape
    assert _grad_close(got, ref)
    assert not _grad_close(got, ref - per_image[-1])                 # image 41 read as zeros


def test_the_wrappers_refuse_past_the_limit_without_allocating(ops):
    g = _gen(10)
    wpk = ops.gemm_pack_weight(_randn(g, 128, 64))
    x1 = _randn(g, 1, 64, 43680)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="2 GiB"):
        ops.gemm_bf16x3(x1.expand(33, -1, -1), wpk, 128)
    assert torch.cuda.memory_allocated() == before
    xm = _randn(g, 1, 64, 64, 64)
    w = _randn(g, 64, 64, 3, 3)
    assert ops.conv3x3_supported(xm.expand(962, -1, -1, -1), w)
    assert not ops.conv3x3_supported(xm.expand(963, -1, -1, -1), w)
