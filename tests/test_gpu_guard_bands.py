"""Does every kernel stay inside the tensors it is given, and does the other branch of every address test compute the same thing?

tests/guard_bands.py places each tensor argument of a library call between two 1 MiB bands of 0xFF and looks at the bands, and at
the interior of every `const` argument, after the call (the module's docstring says what that proves and what it cannot).

Depth (sections 1 to 6): new cases at ragged shapes -- the smallest with a partial tile in every tiled dimension, the tail in the
last rows of the last batch item -- for the families where tiles, masks and vector tails live.  `_three_ways` runs a body
  (a) plain, recording the bytes of every output of every library call,
  (b) under guards at the same alignment: every output must be bit-identical to (a), outside the entries of ATOMIC,
  (c) the body itself compares with its fp64 restatement, at the tolerance the op's existing test states (named beside each body;
      bodies imported from another test module carry theirs with them) -- in all of (a), (b) and the skewed run,
and, where the body reaches an entry of guard_bands.SKEW_BRANCH, once more with the listed arguments 4 bytes off a 16-byte boundary:
(c) again, and bit-identical to (a) for the entries of SAME_BITS_UNDER_SKEW.
Breadth (section 8): the suite's own test bodies, at their smallest parametrisation, under guards; the last test counts which
`*_hip` entries of include/gdm.h ran under guards in this file.

Tensors whose addresses travel inside job structures are guarded by hand (`_HandGuarded`, the job tests of section 2).
"""
import numpy as np
import pytest
import torch

import guard_bands as gb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from geometric_aware_dense_matching_amd import ops as o
    return o


# entries that add floats with atomics: two runs may differ in the last bits, so (b) compares them through (c) only
ATOMIC = {
    "gdm_group_gather_bwd2_hip": "atomicAdd scatter into grad_feat (LDS-privatised partial sums flushed with atomics)",
    "gdm_gather_max_bwd_hip": "atomicAdd scatter into grad_feat",
    "gdm_prelu1_bwd_hip": "one atomicAdd per workgroup into grad_slope",
    "gdm_edge_feature_bwd_hip": "atomicAdd of the neighbour and centre terms into grad_x",
    "gdm_edge_bwd_scatter_hip": "atomicAdd of the neighbours' rows into grad_pq",
}

# pure selections and per-element expressions: the 16-byte and the dword path must give the same bits.  Not listed, because the two
# paths sum in another order or are held to the fp64 bound only: gdm_att_pool_hip / gdm_att_pool_bwd_hip at K = 16 (the quad form
# adds four partial sums per row, the scalar form one running sum), gdm_pointwise2_hip (the 16-byte FMA form gives a thread four
# consecutive points instead of one), gdm_feature_knn_hip (the selected indices and values are compared with the restatement),
# gdm_group_gather_bwd2_hip (atomics).
SAME_BITS_UNDER_SKEW = ("gdm_gather_max_hip", "gdm_upsample_bilinear_hip", "gdm_upconv3x3_gather_hip")


def _three_ways(monkeypatch, body, *args, skew_same=SAME_BITS_UNDER_SKEW, **kw):
    with gb.filled_empties():
        with gb.guarded_calls(monkeypatch, guard=False, record=True) as plain:
            body(*args, **kw)
        with gb.guarded_calls(monkeypatch, record=True) as guarded:
            body(*args, **kw)
        assert sum(guarded.counts.values()) == len(plain.record) > 0
        gb.assert_same_record(plain, guarded, skip=ATOMIC)
        branch = sorted({n for n, _ in plain.record} & set(gb.SKEW_BRANCH))
        if branch:
            with gb.guarded_calls(monkeypatch, skew=4, only=branch, record=True) as skewed:
                body(*args, **kw)
            assert sum(skewed.counts.values()) > 0
            gb.assert_same_record(plain, skewed, skip=set(n for n, _ in plain.record) - set(skew_same), what="skewed")
    return plain


def _close(got, want, rel, what=""):
    """|got - want| < rel * max(1, max |want|), `want` in fp64: the form most of the suite's operator tests use."""
    err = (got.double().cpu() - want.cpu()).abs().max().item()
    tol = rel * max(1.0, want.abs().max().item())
    assert err < tol, "%s: max |err| %.3e, tolerance %.3e" % (what, err, tol)


# --------------------------------------------------------------------------------------
# 1. gather family (gdm_gather.hip: GB = 256 threads, CCHUNK = 8 channels, LCH = 4)
# --------------------------------------------------------------------------------------
GATHER_SHAPES = [(2, 9, 36, 37, 16),       # one channel over a chunk, 16-byte rows (n % 4 == 0), odd m, the K = 16 int4 index path
                 (1, 3, 33, 7, 5),         # scalar throughout
                 (2, 8, 260, 257, 16),     # n and m just over a block
                 (1, 5, 40, 40, 20)]       # the K > 16 kernels


def _gather_case(B, C, n, m, K, seed):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(B, C, n, generator=g)
    idx = torch.randint(0, n, (B, m, K), generator=g, dtype=torch.int32)
    idx[-1, -1, :] = n - 1                         # the last rows of the last item read the last source column ...
    idx[-1, -2, -1] = n - 1
    idx[-1, 0, 0] = 0                              # ... and the first
    return feat, idx


def _scatter64(go, idx, n):
    B, C = go.shape[:2]
    want = torch.zeros(B, C, n, dtype=torch.float64)
    return want.scatter_add_(2, idx.long().view(B, 1, -1).expand(B, C, -1), go.reshape(B, C, -1).double())


def body_group_gather(ops, B, C, n, m, K):
    """test_group_gather: bit-exact; backward: test_gather_backward_reads_a_channel_slice_in_place, 1e-5 * max(1, max |want|),
    from a dense gradient and from a channel slice of a wider one (ops._GroupGather.backward reads it where it lies)."""
    feat, idx = _gather_case(B, C, n, m, K, 3)
    f = feat.cuda().requires_grad_(True)
    out = ops.group_gather(f, idx.cuda())
    want = torch.gather(feat.double(), 2, idx.long().view(B, 1, m * K).expand(B, C, m * K)).view(B, C, m, K)
    assert torch.equal(out.detach().cpu().double(), want)
    g = torch.Generator().manual_seed(4)
    wide = torch.randn(B, C + 3, m, K, generator=g).cuda()
    for go in (wide[:, 3:].contiguous(), wide[:, 3:]):
        (ga,) = torch.autograd.grad(ops.group_gather(f, idx.cuda()), f, go)
        _close(ga, _scatter64(go.cpu(), idx, n), 1e-5, "group_gather backward")


def body_gather_nn(ops, B, C, n, m, K):
    """test_gather_nn: bit-exact; backward as group_gather."""
    feat, idx = _gather_case(B, C, n, m, 1, 5)
    f = feat.cuda().requires_grad_(True)
    out = ops.gather_nn(f, idx.cuda())
    assert torch.equal(out.detach().cpu(), torch.gather(feat, 2, idx.long().view(B, 1, m).expand(B, C, m)))
    go = torch.randn(B, C, m, generator=torch.Generator().manual_seed(6))
    (ga,) = torch.autograd.grad(out, f, go.cuda())
    _close(ga, _scatter64(go, idx, n), 1e-5, "gather_nn backward")


def body_gather_max(ops, B, C, n, m, K):
    """test_gather_max: bit-exact (first maximum); backward: test_gather_backward_matches_autograd, allclose(rtol 1e-5, atol 1e-5)."""
    feat, idx = _gather_case(B, C, n, m, K, 7)
    f = feat.cuda().requires_grad_(True)
    out = ops.gather_max(f, idx.cuda())
    gathered = torch.gather(feat.double(), 2, idx.long().view(B, 1, m * K).expand(B, C, m * K)).view(B, C, m, K)
    want, at = gathered.max(dim=3)
    assert torch.equal(out.detach().cpu().double(), want)
    go = torch.randn(B, C, m, generator=torch.Generator().manual_seed(8))
    (ga,) = torch.autograd.grad(out, f, go.cuda())
    f64 = feat.double().requires_grad_(True)
    g64 = torch.gather(f64, 2, idx.long().view(B, 1, m * K).expand(B, C, m * K)).view(B, C, m, K).max(dim=3)[0]
    (wa,) = torch.autograd.grad(g64, f64, go.double())
    # ties: autograd's max and the kernel may credit another of several equal neighbours (repeated indices: the same source either way)
    assert torch.allclose(ga.cpu().double(), wa, rtol=1e-5, atol=1e-5)


def body_att_pool(ops, B, C, n, m, K):
    """test_att_pool: allclose(rtol 1e-5, atol 1e-6); backward: test_att_pool_backward_any_k, 1e-5 * max(1, max |grad|)."""
    g = torch.Generator().manual_seed(9)
    att = (torch.randn(B, C, n, K, generator=g) * 3)
    feat = torch.randn(B, C, n, K, generator=g)
    w = torch.randn(B, C, n, generator=g)
    a, f = att.cuda().requires_grad_(True), feat.cuda().requires_grad_(True)
    out = ops.att_pool(a, f)
    a64, f64 = att.double().requires_grad_(True), feat.double().requires_grad_(True)
    want = (torch.softmax(a64, dim=3) * f64).sum(3)
    assert torch.allclose(out.detach().cpu().double(), want.detach(), rtol=1e-5, atol=1e-6)
    (out * w.cuda()).sum().backward()
    (want * w.double()).sum().backward()
    _close(a.grad, a64.grad, 1e-5, "att_pool grad_att")
    _close(f.grad, f64.grad, 1e-5, "att_pool grad_feat")


def body_rel_pos_enc(ops, B, C, n, m, K):
    """test_rel_pos_enc: channels 1..9 bit-exact, the norm allclose(rtol 3e-7, atol 1e-12)."""
    g = torch.Generator().manual_seed(10)
    xyz = torch.rand(B, n, 3, generator=g)
    idx = torch.randint(0, n, (B, n, K), generator=g, dtype=torch.int32)
    idx[-1, -1, :] = n - 1
    got = ops.rel_pos_enc(xyz.cuda(), idx.cuda()).cpu()
    nb = torch.gather(xyz.unsqueeze(1).expand(B, n, n, 3), 2, idx.long().unsqueeze(3).expand(B, n, K, 3))        # [B,n,K,3]
    ctr = xyz.unsqueeze(2).expand(B, n, K, 3)
    rel = ctr - nb
    want = torch.cat([rel, ctr, nb], dim=3).permute(0, 3, 1, 2)
    assert torch.equal(got[:, 1:], want)
    dist = rel.double().pow(2).sum(3).sqrt()
    assert torch.allclose(got[:, 0].double(), dist, rtol=3e-7, atol=1e-12)


@pytest.mark.parametrize("B,C,n,m,K", GATHER_SHAPES)
@pytest.mark.parametrize("body", [body_group_gather, body_gather_nn, body_gather_max, body_att_pool, body_rel_pos_enc],
                         ids=lambda f: f.__name__[5:])
def test_gather_family(ops, monkeypatch, body, B, C, n, m, K):
    plain = _three_ways(monkeypatch, body, ops, B, C, n, m, K)
    names = {n_ for n_, _ in plain.record}
    assert names & {"gdm_group_gather_hip", "gdm_gather_max_hip", "gdm_att_pool_hip", "gdm_rel_pos_enc_hip"}


def test_gather_max_row_in_lds_form_on_both_sides_of_its_address_tests(ops, monkeypatch):
    """gather_max_rowlds_kernel (n >= 1024, m K >= 2048, not the flat form) stages a source row with float4 loads and reads K = 16
    index rows as int4 only where the addresses allow: the smallest shape that reaches it, with n % 4 == 0 so that the address decides."""
    _three_ways(monkeypatch, body_gather_max, ops, 2, 3, 1028, 257, 16)


# --------------------------------------------------------------------------------------
# 2. pointwise (gdm_pointwise.hip: PT = 64 points per tile): segment and job tensors guarded by hand
# --------------------------------------------------------------------------------------
class _HandGuarded:
    """The package's `ops` with `pointwise` placing every segment tensor and the output between guard bands: their addresses travel
    in gdm_pw_seg structures, which guarded_calls cannot see.  skew moves the segments' x (gdm_pointwise2_hip branches on them)."""

    def __init__(self, ops, skew=0):
        self._ops, self._skew, self.checked = ops, skew, 0

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def pointwise(self, segs, wt, scale=None, shift=None, act=0, slope=0.0, point_major=False, out=None, out_c0=0, w_rowmajor=False):
        if not isinstance(segs, list):
            segs = [segs]
        held, gsegs = [], []
        for i, sp in enumerate(segs):
            x, idx = (sp, None) if torch.is_tensor(sp) else sp
            gx = gb.guard(x.contiguous(), self._skew)
            held.append((gx, "segs[%d].x" % i))
            if idx is None:
                gsegs.append(gx.t)
            else:
                gi = gb.guard(idx.to(torch.int32).contiguous())
                held.append((gi, "segs[%d].idx" % i))
                gsegs.append((gx.t, gi.t))
        if out is None:
            B = held[0][0].t.shape[0]
            last = gsegs[-1]
            n = last.reshape(B, last.shape[1], -1).shape[2] if torch.is_tensor(last) else last[1].reshape(B, -1).shape[1]
            cout = wt.shape[0] if w_rowmajor else wt.shape[1]
            go = gb.guard_like((B, n, cout) if point_major else (B, cout, n), torch.float32)
        else:
            go = gb.guard(out)
        held.append((go, "out"))
        ret = self._ops.pointwise(gsegs, wt, scale, shift, act, slope, point_major, go.t, out_c0, w_rowmajor)
        torch.cuda.synchronize()
        assert ret.data_ptr() == go.t.data_ptr()
        for g, name in held:
            g.check("gdm_pointwise2_hip", name)
        flat = [t for sp in segs for t in ((sp,) if torch.is_tensor(sp) else sp)]
        for (g, name), src in zip(held, flat):
            assert gb.same_bits(g.t, src.to(torch.int32).contiguous() if src.dtype == torch.int64 else src.contiguous()), name + " was written"
        self.checked += 1
        if out is not None:
            out.copy_(go.t)
            return out
        return go.t


    def point_heads(self, a, b, layers, last, feat_layer, res_layer, residual=None):
        """The layer arrays of gdm_point_heads2_hip (packed weights, scales, shifts: host arrays of device addresses)."""
        held, glayers = [], []
        for i, (wpk, sc, sh, act) in enumerate(layers):
            gs = [None if t is None else gb.guard(t) for t in (wpk, sc, sh)]
            held += [(g, t, "%s[%d]" % (nm, i)) for g, t, nm in zip(gs, (wpk, sc, sh), ("w", "scale", "shift")) if g is not None]
            glayers.append(tuple(None if g is None else g.t for g in gs) + (act,))
        ret = self._ops.point_heads(a, b, glayers, last, feat_layer, res_layer, residual)
        torch.cuda.synchronize()
        for g, t, name in held:
            g.check("gdm_point_heads2_hip", name)
            assert gb.same_bits(g.t, t), name + " was written"
        self.checked += 1
        return ret


POINTWISE = [  # (B, n, segment channels, Cout, n_src of the indexed middle segment, point_major) for test_pointwise_layer_vs_torch
    (2, 65, (3, 29, 35), 17, 10, False),          # MFMA form, K = 67 in four parts of 20 rows: the waves straddle the segment
    (2, 68, (3, 29, 35), 17, 10, False),          #   boundaries 3 | 32 | 67 and the last wave has 7 rows; n % 4 == 0 beside it
    (2, 65, (3, 29, 35), 17, 10, True),
    (2, 68, (3, 29, 35), 17, None, True),
    (2, 68, (3, 61, 67), 17, None, False),        # K = 131 in eight parts of 20 rows: the last wave has none, the one before 11
    (2, 65, (5, 9, 11, 8), 33, None, False),      # four segments, Cout >= 32
    (2, 68, (8, 12, 4, 16), 40, 12, False),
    (2, 65, (3, 8), 5, None, False),              # FMA form, K = 11
    (2, 68, (3, 8), 5, None, False),
    (2, 68, (4, 8), 8, None, False),              # ... its 16-byte form (n % 4 == 0, Cout % 4 == 0)
    (2, 68, (3, 8), 5, None, True),
]


@pytest.mark.parametrize("skew", [0, 4])
@pytest.mark.parametrize("B,n,cs,cout,n_src,pm", POINTWISE)
def test_pointwise_segments_and_output_between_guards(ops, monkeypatch, B, n, cs, cout, n_src, pm, skew):
    """tests/test_gpu_ops.py::test_pointwise_layer_vs_torch (fp64, 1e-5 relative to the output scale; the out_c0 = 5 slice of an
    output nine channels wider, whose other channels must stay untouched) at ragged shapes, every segment and the output guarded by
    hand, the other arguments by the wrapper; skew 4: the segments and the weight 4 bytes off, the dword paths must agree with fp64."""
    import test_gpu_ops as t
    hand = _HandGuarded(ops, skew)
    with gb.guarded_calls(monkeypatch, skew=skew, only=("gdm_pointwise2_hip",)) as calls:
        t.test_pointwise_layer_vs_torch(hand, B, n, cs, cout, n_src, pm)
    assert hand.checked == calls.counts["gdm_pointwise2_hip"] == (2 if pm else 3)


@pytest.mark.parametrize("skew", [0, 4])
@pytest.mark.parametrize("B,n,K,cout", [(2, 65, 67, 17), (2, 68, 11, 5), (2, 68, 12, 8)])
def test_pointwise_rowmajor_weight_between_guards(ops, monkeypatch, B, n, K, cout, skew):
    import test_gpu_ops as t
    hand = _HandGuarded(ops, skew)
    with gb.guarded_calls(monkeypatch, skew=skew, only=("gdm_pointwise2_hip",)):
        t.test_pointwise_rowmajor_weight_equals_transposed_copy(hand, B, n, K, cout)
    assert hand.checked == 2


@pytest.mark.parametrize("B,n,C0,C1,C2,acts", [(1, 257, 1, 3, 2, (0, 2)), (1, 257, 16, 16, 32, (1, 0))])
def test_pointwise_chain2(ops, monkeypatch, B, n, C0, C1, C2, acts):
    import test_gpu_ops as t
    _three_ways(monkeypatch, t.test_pointwise_chain2_equals_two_launches_bit_for_bit, ops, B, n, C0, C1, C2, acts)


@pytest.mark.parametrize("skew", [0, 4])
def test_pointwise_jobs_between_guards(ops, monkeypatch, skew):
    """gdm_pointwise_jobs_hip on a job table built here, every x, weight and output between guard bands: ns = (1, 4, 9, 36), K = 64,
    Cout = 40 (three 16-channel blocks, the last half empty).  test_pointwise_jobs_equal_separate_launches_bit_for_bit: 2e-6 relative
    to the output scale against the fp64 product, and bit-identical to one gdm_pointwise2_hip launch per job.  skew 4 moves x (the
    launcher branches on it per job); `out` must stay aligned (it is refused otherwise) and the weight is read by dwords."""
    from geometric_aware_dense_matching_amd import _lib
    B, K, Cout, ns = 2, 64, 40, (1, 4, 9, 36)
    g = torch.Generator().manual_seed(K + Cout)
    xs = [torch.randn(B, K, n, generator=g).cuda() for n in ns]
    wts = [(torch.randn(K, Cout, generator=g) / K ** 0.5).cuda() for _ in ns]
    gx = [gb.guard(x, skew) for x in xs]
    gw = [gb.guard(w) for w in wts]
    go = [gb.guard_like((B, Cout, n), torch.float32) for n in ns]
    arr = (_lib.PwJob * len(ns))()
    for j, n in enumerate(ns):
        arr[j] = _lib.PwJob(gx[j].t.data_ptr(), gw[j].t.data_ptr(), go[j].t.data_ptr(), n)
    with gb.guarded_calls(monkeypatch) as calls:
        ops.call("gdm_pointwise_jobs_hip", arr, len(ns), B, K, Cout)
    torch.cuda.synchronize()
    assert calls.counts["gdm_pointwise_jobs_hip"] == 1
    for j, n in enumerate(ns):
        for grd, name, src in ((gx[j], "jobs[%d].x" % j, xs[j]), (gw[j], "jobs[%d].wt" % j, wts[j]), (go[j], "jobs[%d].out" % j, None)):
            grd.check("gdm_pointwise_jobs_hip", name)
            assert src is None or gb.same_bits(grd.t, src), name + " was written"
        want = torch.einsum("kc,bkn->bcn", wts[j].double(), xs[j].double())
        _close(go[j].t, want, 2e-6, "job %d" % j)
        assert torch.equal(go[j].t, ops.pointwise([xs[j]], wts[j]))


# --------------------------------------------------------------------------------------
# 3. convolution / GEMM (gdm_conv.hip: workgroups of 256 pixels x 128 output channels, Cout padded to 128), gdm_wgrad.hip
# --------------------------------------------------------------------------------------
def body_p2r_epilogue(ops, misaligned_idx):
    """conv1x1_packed_gather_add_act at (B, Cin, cout, H, W, n) = (1, 128, 200, 8, 32, 5): one workgroup, 200 = 128 + 72 channels,
    against fp64 at test_fused_epilogue_against_fp64's bound, 2e-5 * max(1, max |reference|).  misaligned_idx: the index is a view
    4 bytes into its allocation -- ops.conv1x1_packed_gather_add_act clones it (the epilogue loads four indices at once)."""
    import test_gpu_p2r_epilogue as t
    Cin, Cout, B, H, W, gn = 128, 200, 1, 8, 32, 5
    x, w, tt, idx, sc, sh = t._case(Cin, Cout, B, H, W, gn, seed=9)
    if misaligned_idx:
        base = torch.empty(idx.numel() + 1, dtype=torch.int32, device="cuda")
        base[1:] = idx.view(-1)
        idx = base[1:].view(B, H * W)
        assert idx.data_ptr() % 16 == 4 and idx.is_contiguous()
    wpk = ops.gemm_pack_weight(w)
    got = t._fused(ops, x, wpk, Cout, tt, idx, sc, sh, 1, True)[0]
    mm = torch.matmul(w.cpu().double(), x.cpu().double().view(B, Cin, H * W))
    src = idx.cpu().long().clamp(0, gn - 1).unsqueeze(1).expand(B, Cout, H * W)
    ref = (sc.cpu().double()[None, :, None] * (mm + torch.gather(tt.cpu().double(), 2, src)) + sh.cpu().double()[None, :, None]).clamp(min=0)
    _close(got, ref, 2e-5, "fused epilogue")


def _conv_cases():
    import test_gpu_ops as t
    import test_gpu_train as tt
    return {
        "conv3x3-1x128x72x5x32": (t.test_conv3x3_bf16x3_vs_fp32_conv, (1, 128, 72, 5, 32)),           # scale, shift, residual, ReLU inside
        "conv3x3-3x64x200x3x32": (t.test_conv3x3_bf16x3_vs_fp32_conv, (3, 64, 200, 3, 32)),
        "conv3x3-small-3x64x200x3x32": (t.test_conv3x3_bf16x3_small_channel_counts, (3, 64, 200, 3, 32)),
        "conv3x3-stride2-1x128x136x4x64": (t.test_strided_conv3x3_and_conv1x1_downsample_vs_fp64, (1, 128, 136, 4, 64)),   # + conv1x1_packed2d, stride 2
        "conv3x3-packed-out-2x128x64x72x4x32": (t.test_conv3x3_packed_output_feeds_the_next_convolution, (2, 128, 64, 72, 4, 32)),
        "gemm-1x64x128x32": (t.test_gemm_bf16x3, (1, 64, 128, 32)),
        "gemm-2x128x200x96": (t.test_gemm_bf16x3, (2, 128, 200, 96)),                                  # both output layouts
        # (Cout, Cin, taps): the packed layer has Cin output and Cout input channels, and its input channels must be 64 or a multiple
        # of 128 (cin_ok of csrc/gdm_conv.hip), so the ragged count goes in the Cin slot; (72, 200, 1) and (136, 128, 9) are refused
        # (test_dgrad_weight_pack_refuses_a_ragged_channel_count_on_its_input_side)
        "pack-weight-dgrad-64x200x1": (t.test_dgrad_weight_pack_equals_pack_of_flipped_transposed_filter, (64, 200, 1)),
        "pack-weight-dgrad-128x72x1": (t.test_dgrad_weight_pack_equals_pack_of_flipped_transposed_filter, (128, 72, 1)),
        "pack-weight-dgrad-128x136x9": (t.test_dgrad_weight_pack_equals_pack_of_flipped_transposed_filter, (128, 136, 9)),
        "p2r-epilogue-1x128x200x8x32x5": (body_p2r_epilogue, (False,)),
        "p2r-epilogue-misaligned-index": (body_p2r_epilogue, (True,)),
    }, {
        "wgrad-1x256x72x4x32-parts1": (tt.test_conv3x3_weight_gradient_on_the_mfma_gemm_equals_autograd, (1, 256, 72, 4, 32, 1)),
        "wgrad-1x256x72x4x32": (tt.test_conv3x3_weight_gradient_on_the_mfma_gemm_equals_autograd, (1, 256, 72, 4, 32, None)),
    }


@pytest.mark.parametrize("case", ["conv3x3-1x128x72x5x32", "conv3x3-3x64x200x3x32", "conv3x3-small-3x64x200x3x32", "conv3x3-stride2-1x128x136x4x64",
                                  "conv3x3-packed-out-2x128x64x72x4x32", "gemm-1x64x128x32", "gemm-2x128x200x96", "pack-weight-dgrad-64x200x1",
                                  "pack-weight-dgrad-128x72x1", "pack-weight-dgrad-128x136x9", "p2r-epilogue-1x128x200x8x32x5", "p2r-epilogue-misaligned-index",
                                  "wgrad-1x256x72x4x32-parts1", "wgrad-1x256x72x4x32"])
def test_conv_and_gemm(ops, monkeypatch, case):
    with_ops, without = _conv_cases()
    if case in with_ops:
        body, args = with_ops[case]
        _three_ways(monkeypatch, body, ops, *args)
    else:
        body, args = without[case]
        _three_ways(monkeypatch, body, *args)


@pytest.mark.parametrize("Cout,Cin,taps", [(72, 200, 1), (136, 128, 9)])
def test_dgrad_weight_pack_refuses_a_ragged_channel_count_on_its_input_side(ops, monkeypatch, Cout, Cin, taps):
    """conv_pack_weight_dgrad packs the weight of the layer that maps Cout channels back to Cin: 72 or 136 INPUT channels are no
    shape of the convolution kernel (64, or a multiple of 128).  The call is refused before any launch, nothing is written."""
    from geometric_aware_dense_matching_amd import _lib
    w = torch.randn((Cout, Cin, 3, 3) if taps == 9 else (Cout, Cin), generator=torch.Generator().manual_seed(Cout)).cuda()
    with gb.guarded_calls(monkeypatch) as calls:
        with pytest.raises(_lib.GdmError):
            ops.conv_pack_weight_dgrad(w)
    assert not calls.counts


def body_gemm_grouped(ops, R):
    """gemm_grouped (the SplineConv training path's row-gathering GEMM): R gathered rows in 256-row tiles, the last tile holding
    three real rows and 253 repeats of vertex 0's, each tile against its own 128 output columns.  test_gemm_bf16x3's bound."""
    g = torch.Generator().manual_seed(R)
    Cin, nt, M = 128, R // 256, 300
    x = torch.randn(1, Cin, M, generator=g).cuda()
    w = (torch.randn(128 * nt, Cin, generator=g) / Cin ** 0.5).cuda()
    rowidx = torch.randint(0, M, (R,), generator=g, dtype=torch.int32)
    rowidx[R - 253:] = 0
    rowidx[R - 256:R - 253] = M - 1                     # the real rows of the last tile gather the last vertex
    tile_co0 = (torch.arange(nt, dtype=torch.int32) * 128).cuda()
    got = ops.gemm_grouped(x, ops.gemm_pack_weight(w), rowidx.cuda(), tile_co0, 128 * nt)
    xs = x[0].double()[:, rowidx.long().cuda()]                                       # [Cin, R]
    want = torch.stack([w.double()[128 * (r // 256):128 * (r // 256) + 128] @ xs[:, r] for r in range(R)], 0)           # [R, 128]
    assert got.shape == (R, 128)
    _close(got, want, 2e-5, "gemm_grouped")


@pytest.mark.parametrize("R", [256, 512])
def test_gemm_grouped_with_a_last_group_that_is_mostly_padding(ops, monkeypatch, R):
    _three_ways(monkeypatch, body_gemm_grouped, ops, R)


# --------------------------------------------------------------------------------------
# 4. image branch and elementwise kernels (gdm_image.hip, gdm_bn.hip, gdm_stem.hip, gdm_upconv.hip)
# --------------------------------------------------------------------------------------
def body_affine_act(ops, inner, res, inplace):
    """tests/test_gpu_instances.py::test_affine_act_every_residual_form: 1e-6 * max(1, max |want|)."""
    g = torch.Generator().manual_seed(inner + 2 * res + inplace)
    shape = (2, 5, inner)
    x, r = torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
    sc, sh, rs, rb = (torch.randn(5, generator=g).cuda() for _ in range(4))
    v = lambda t: t.double().view(1, 5, 1)
    want = x.double() * v(sc) + v(sh)
    if res:
        want = want + r.double() * v(rs) + v(rb)
    want = torch.where(want > 0, want, want * 0.2)
    xin = x.clone()
    got = ops.affine_act(xin, sc, sh, ops.ACT_LEAKY, 0.2, res=r if res else None, res_scale=rs if res else None,
                         res_shift=rb if res else None, inplace=inplace)
    assert (got.data_ptr() == xin.data_ptr()) == inplace and (inplace or torch.equal(xin, x))
    _close(got, want, 1e-6, "affine_act")


def body_affine_act_maxk(ops):
    """tests/test_gpu_instances.py::test_affine_act_maxk_every_activation: 1e-6 * max(1, max |want|); n = 257 points: two blocks."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 257, 20, generator=g).cuda()
    sc, sh = torch.randn(3, generator=g).cuda(), torch.randn(3, generator=g).cuda()
    y = x.double() * sc.double().view(1, 3, 1, 1) + sh.double().view(1, 3, 1, 1)
    _close(ops.affine_act_maxk(x, sc, sh, 2, 0.2), torch.where(y > 0, y, y * 0.2).max(dim=3)[0], 1e-6, "affine_act_maxk")


def _image_cases():
    import test_gpu_instances as ti
    import test_gpu_ops as t
    import test_gpu_train as tt
    with_ops = {
        "upsample-1x1-to-5x31": (t.test_upsample_bilinear_align_corners, (1, 3, 1, 1, 5, 31)),        # the ox0 + 3 < OW tail, forward and backward
        "upsample-1x1-to-5x33": (t.test_upsample_bilinear_align_corners, (1, 3, 1, 1, 5, 33)),
        "upsample-3x3-to-5x33": (t.test_upsample_bilinear_align_corners, (2, 3, 3, 3, 5, 33)),
        "upsample-3x3-to-5x31": (t.test_upsample_bilinear_align_corners, (2, 3, 3, 3, 5, 31)),
        "affine-relu-maxpool-1x3x7x9": (t.test_affine_relu_maxpool_equals_modules, (1, 3, 7, 9)),
        "psp-pools-and-final": (t.test_final_stage_and_psp_pools, ()),                                 # psp_pools forward at (1, 3, 13, 9)
        "psp-combine-3x24x10x12": (t.test_psp_combine_with_packed_output, (3, 24, 10, 12)),
        "psp-combine-packed-1x64x8x32": (t.test_psp_combine_with_packed_output, (1, 64, 8, 32)),
        "upconv-gather-1x5x3x7x9": (t.test_upconv3x3_gather_equals_conv_after_upsample, (1, 5, 3, 7, 9)),
        "upconv-gather-one-channel": (t.test_upconv3x3_gather_equals_conv_after_upsample, (1, 5, 1, 7, 9)),
        "upconv-gather-packed-1x64x8x32": (t.test_upconv_gather_eight_channel_form_with_packed_output, (1, 64, 8, 32, 1)),
        "upconv-gather-12x31": (t.test_upconv3x3_gather_other_scale_factors, (1, 6, 5, 9, 12, 12, 31)),
        "upconv-gather-train-12x31": (t.test_upconv3x3_gather_train_forward_backward_any_scale, (1, 5, 9, 12, 12, 31)),
        "upconv-final-points-N33": (t.test_upconv_final_points_equals_dense_stage_at_the_chosen_pixels, (1, 5, 7, 33)),
        "conv64-fusion-m256-n5": (t.test_conv64_fusion_kernel_packed_output, (1, 8, 32, 5, 1)),
        "conv1x1-logsoftmax-hw63": (ti.test_final_stage_at_several_sizes, (1, 7, 9, True)),
        "stem-1x7x9": (t.test_stem_kernel_vs_torch_fp64, (1, 7, 9)),
        "stem-1x100x70": (t.test_stem_kernel_vs_torch_fp64, (1, 100, 70)),
        "affine-act-inner4": (body_affine_act, (4, False, True)),
        "affine-act-inner4-res": (body_affine_act, (4, True, False)),
        "affine-act-inner100": (body_affine_act, (100, False, False)),
        "affine-act-inner100-res-inplace": (body_affine_act, (100, True, True)),
        "affine-act-maxk": (body_affine_act_maxk, ()),
    }
    without = {
        "prelu1": (tt.test_prelu1_forward_backward_equals_torch, ()),
        "psp-pools-backward-1x3x13x9": (tt.test_psp_pools_backward_matches_adaptive_avg_pool, (1, 3, 13, 9)),
        "batchnorm-1x7x8": (tt.test_fused_batchnorm_act_training_matches_modules, ((1, 7, 8), 2)),
        "batchnorm-3x8x100": (tt.test_fused_batchnorm_act_training_matches_modules, ((3, 8, 100), 2)),
    }
    return with_ops, without


IMAGE_CASES = ["upsample-1x1-to-5x31", "upsample-1x1-to-5x33", "upsample-3x3-to-5x33", "upsample-3x3-to-5x31", "affine-relu-maxpool-1x3x7x9", "psp-pools-and-final",
               "psp-combine-3x24x10x12", "psp-combine-packed-1x64x8x32", "upconv-gather-1x5x3x7x9", "upconv-gather-one-channel",
               "upconv-gather-packed-1x64x8x32", "upconv-gather-12x31", "upconv-gather-train-12x31", "upconv-final-points-N33",
               "conv64-fusion-m256-n5", "conv1x1-logsoftmax-hw63", "stem-1x7x9", "stem-1x100x70", "affine-act-inner4", "affine-act-inner4-res",
               "affine-act-inner100", "affine-act-inner100-res-inplace", "affine-act-maxk", "prelu1", "psp-pools-backward-1x3x13x9",
               "batchnorm-1x7x8", "batchnorm-3x8x100"]


@pytest.mark.parametrize("case", IMAGE_CASES)
def test_image_and_elementwise(ops, monkeypatch, case):
    with_ops, without = _image_cases()
    assert set(IMAGE_CASES) == set(with_ops) | set(without)
    if case in with_ops:
        body, args = with_ops[case]
        _three_ways(monkeypatch, body, ops, *args)
    else:
        body, args = without[case]
        _three_ways(monkeypatch, body, *args)


@pytest.mark.parametrize("pm,tpm", [(False, False), (True, True)])
def test_conv64_gather_add_act_mfma_both_point_term_layouts(ops, monkeypatch, pm, tpm):
    import test_gpu_instances as ti
    _three_ways(monkeypatch, ti.test_conv64_gather_add_act_mfma_every_layout_and_activation, ops, 1, pm, tpm)


@pytest.mark.parametrize("tpm", [False, True])
def test_conv64_gather_add_act_mfma_at_m256_n5(ops, monkeypatch, tpm):
    """conv64_gather_add_act_mfma at m = 8 x 32 pixels, n = 5 points, the point term channel-major and point-major, with the packed
    operand beside the map; the last pixels gather the last point.  fp64 at the bound of
    tests/test_gpu_instances.py::test_conv64_gather_add_act_mfma_every_layout_and_activation, 3e-5 * max(1, max |want|)."""
    def body():
        g = torch.Generator().manual_seed(19 + tpm)
        B, n, m = 1, 5, 256
        x = torch.randn(B, 64, m, generator=g).cuda()
        w = (torch.randn(64, 64, generator=g) / 8).cuda()
        t = torch.randn(B, 64, n, generator=g).cuda()
        idx = torch.randint(0, n, (B, m), generator=g).int().cuda()
        idx[:, -4:] = n - 1
        sc, sh = (torch.rand(64, generator=g) + 0.5).cuda(), torch.randn(64, generator=g).cuda()
        got = ops.conv64_gather_add_act_mfma(x, ops.pack_rows64(w), t.transpose(1, 2).contiguous() if tpm else t, idx, sc, sh, 2, 0.2,
                                             t_point_major=tpm, hw=(8, 32))
        want = torch.einsum("oc,bcm->bom", w.double(), x.double()) + torch.gather(t.double(), 2, idx.long().view(B, 1, m).expand(B, 64, m))
        want = want * sc.double().view(1, 64, 1) + sh.double().view(1, 64, 1)
        _close(got, torch.where(want > 0, want, want * 0.2), 3e-5, "conv64_gather_add_act_mfma")
        assert getattr(got, "_gdm_packed", None) is not None
    _three_ways(monkeypatch, body)


def test_upconv_fused64_from_5x7(ops, monkeypatch):
    """upconv_fused64 at (1, 64, 5, 7) -> (10, 14): a partial tile in both directions, against upsample -> conv3x3 -> affine -> PReLU
    in fp64 at tests/test_gpu_instances.py::test_upconv_kernels_every_activation's bound, 3e-5 * max(1, max |want|)."""
    def body():
        g = torch.Generator().manual_seed(12)
        x = torch.randn(1, 64, 5, 7, generator=g).cuda()
        w3 = (torch.randn(64, 64, 3, 3, generator=g) * 0.05).cuda()
        sc, sh = (torch.rand(64, generator=g) + 0.5).cuda(), torch.randn(64, generator=g).cuda()
        up = torch.nn.functional.interpolate(x.double(), size=(10, 14), mode="bilinear", align_corners=True)
        h = torch.nn.functional.conv2d(up, w3.double(), padding=1) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
        h = torch.where(h > 0, h, h * 0.25)
        got = ops.upconv_fused64(x, ops.upconv_fused64_pack_weight(w3), sc, sh, (10, 14), 2, 0.25)
        _close(got, h, 3e-5, "upconv_fused64")
    _three_ways(monkeypatch, body)


# --------------------------------------------------------------------------------------
# 5. point branch
# --------------------------------------------------------------------------------------
def _point_cases():
    import test_gpu_dgcnn_fused as td
    import test_gpu_ops as t
    with_ops = {
        "lfa-stage-32x65": (t.test_fused_lfa_stage_equals_unfused_block, (32, 65)),
        "point-heads-N65": (t.test_point_heads_chain_equals_the_layers_in_fp64, (1, 65, 128)),        # HD_P = 64 points per block
        "point-heads-N100": (t.test_point_heads_chain_equals_the_layers_in_fp64, (2, 100, 72)),
        "point-heads-two-launches": (t.test_point_heads_in_two_launches_equals_one, ()),
        "edge-feature": (t.test_edge_feature_and_backward, ()),
        "topk-rows-3x33x32": (t.test_topk_rows, (3, 33, 32)),
    }
    without = {
        "feature-knn-n33-k5": (td.test_feature_knn_vs_oracle, (2, 9, 33, 5, "randn", 131)),
        "feature-knn-n100-k20": (td.test_feature_knn_vs_oracle, (1, 64, 100, 20, "randn", 132)),
        "feature-knn-channel-slice": (td.test_feature_knn_reads_a_channel_slice_in_place, ()),
        "edge-block-two-layers-c0": (td.test_edge_block_vs_fp64_restatement, (2, 9, 33, 5, True, 64, 133)),
        "edge-block-one-layer": (td.test_edge_block_vs_fp64_restatement, (1, 64, 65, 20, False, 0, 134)),
    }
    return with_ops, without


POINT_CASES = ["lfa-stage-32x65", "point-heads-N65", "point-heads-N100", "point-heads-two-launches", "edge-feature", "topk-rows-3x33x32",
               "feature-knn-n33-k5", "feature-knn-n100-k20", "feature-knn-channel-slice", "edge-block-two-layers-c0", "edge-block-one-layer"]


@pytest.mark.parametrize("case", POINT_CASES)
def test_point_branch(ops, monkeypatch, case):
    with_ops, without = _point_cases()
    assert set(POINT_CASES) == set(with_ops) | set(without)
    if case in with_ops:
        body, args = with_ops[case]
        _three_ways(monkeypatch, body, ops, *args)
    else:
        body, args = without[case]
        _three_ways(monkeypatch, body, *args)


@pytest.mark.parametrize("B,N,Ca", [(1, 65, 128), (2, 100, 72)])
def test_point_heads_layer_arrays_between_guards(ops, monkeypatch, B, N, Ca):
    """tests/test_gpu_ops.py::test_point_heads_chain_equals_the_layers_in_fp64 (3e-5 / 5e-5 relative) with every layer's packed weight,
    scale and shift placed between guard bands by hand (HD_P = 64 points per block: N = 65 and 100 leave a partial block)."""
    import test_gpu_ops as t
    hand = _HandGuarded(ops)
    with gb.guarded_calls(monkeypatch, only=("gdm_point_heads2_hip",)) as calls:
        t.test_point_heads_chain_equals_the_layers_in_fp64(hand, B, N, Ca)
    assert hand.checked == calls.counts["gdm_point_heads2_hip"] >= 1


def body_spline_16_channels(ops):
    """The two SplineConv entries that pick a 16-byte or a one-channel-per-thread kernel by the address (gdm_spline_direct3_hip,
    gdm_spline_pairs_aggregate3_hip), at C = 16 (C % 4 == 0, 512 % C == 0) with the row-major output alone, M = 133 vertices (eight
    per block: a partial last block).  tests/test_gpu_ops.py::test_spline_scalar_kernels_for_odd_channel_counts: the direct layer
    against the dense form and the pair aggregation against its fp64 definition, both 1e-5 * max(1, max |want|)."""
    from geometric_aware_dense_matching_amd import splinecnn
    torch.manual_seed(20)
    M, C = 133, 16
    ei, ea = splinecnn.build_mesh_graph(torch.rand(M, 3, device="cuda"), k=4)
    order = torch.argsort(ei[1], stable=True)
    rowptr = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
    rowptr[1:] = torch.cumsum(torch.bincount(ei[1][order], minlength=M), 0).to(torch.int32)
    src, attr = ei[0][order].to(torch.int32).contiguous(), ea[order].contiguous()
    conv = splinecnn.SplineConv(9, C).cuda()
    conv.bias.data.normal_(0, 0.1)
    x = torch.randn(M, 9, device="cuda")
    with torch.enable_grad():
        dense = conv(x, rowptr, src, attr, relu=True).detach()
    with torch.no_grad():
        direct = conv(x, rowptr, src, attr, relu=True)
    _close(direct, dense.double(), 1e-5, "spline direct layer")
    E, R = int(rowptr[-1]), 500
    g = torch.Generator().manual_seed(21)
    Y = torch.randn(R, C, generator=g).cuda()
    pos = torch.randint(0, R, (E, 8), generator=g).int().cuda()
    pos[-1] = R - 1
    basis = torch.rand(E, 8, generator=g).cuda()
    root = torch.randn(M, C, generator=g).cuda()
    out = torch.empty(M, C, device="cuda")
    splinecnn.call("gdm_spline_pairs_aggregate3_hip", Y, rowptr, pos, basis, root, conv.bias.detach(), M, C, 1, out, None, None)
    msg = (basis.double().unsqueeze(2) * Y.double()[pos.long()]).sum(1)
    tgt = torch.repeat_interleave(torch.arange(M, device="cuda"), (rowptr[1:] - rowptr[:-1]).long())
    acc = torch.zeros(M, C, dtype=torch.float64, device="cuda").index_add_(0, tgt, msg)
    deg = (rowptr[1:] - rowptr[:-1]).double().clamp(min=1).unsqueeze(1)
    _close(out, torch.relu(acc / deg + root.double() + conv.bias.detach().double()), 1e-5, "spline pair aggregation")


def test_spline_address_branches_on_both_sides(ops, monkeypatch):
    plain = _three_ways(monkeypatch, body_spline_16_channels, ops)
    assert {"gdm_spline_direct3_hip", "gdm_spline_pairs_aggregate3_hip"} <= {n for n, _ in plain.record}


def body_edge_feature_n33(ops):
    """edge_feature at n = 33, K = 5: tests/test_gpu_ops.py::test_edge_feature_and_backward -- forward bit-exact, backward
    allclose(rtol 1e-4, atol 1e-4)."""
    g = torch.Generator().manual_seed(13)
    B, C, n, K = 2, 5, 33, 5
    x = torch.randn(B, C, n, generator=g)
    idx = torch.randint(0, n, (B, n, K), generator=g, dtype=torch.int32)
    idx[-1, -1, :] = n - 1
    a = x.double().requires_grad_(True)
    nb = torch.gather(a.unsqueeze(2).expand(B, C, n, n), 3, idx.long().unsqueeze(1).expand(B, C, n, K))
    ctr = a.unsqueeze(3).expand(B, C, n, K)
    want = torch.cat([nb - ctr, ctr], dim=1)
    b = x.cuda().requires_grad_(True)
    got = ops.edge_feature(b, idx.cuda())
    assert torch.equal(got.detach().cpu(), want.detach().float())
    w = torch.randn(want.shape, generator=g)
    (want * w.double()).sum().backward()
    (got * w.cuda()).sum().backward()
    assert torch.allclose(b.grad.cpu().double(), a.grad, rtol=1e-4, atol=1e-4)


def test_edge_feature_at_n33(ops, monkeypatch):
    _three_ways(monkeypatch, body_edge_feature_n33, ops)


def test_knn_jobs_and_copy_views_with_their_inputs_between_guards(ops, monkeypatch):
    """gdm_knn_job and gdm_copy_job carry addresses: the supports, queries and source views are placed between guard bands here, the
    workspace by the wrapper.  Results against ops.knn_batch (itself held to the oracle bit for bit) and against .contiguous()."""
    g = torch.Generator().manual_seed(14)
    B = 2
    cloud = torch.rand(B, 133, 3, generator=g).cuda()
    gc = gb.guard(cloud)
    sup, qry = gc.t[:, :77], gc.t[:, :33]                              # prefix views: the batch stride stays 133 * 3
    with gb.guarded_calls(monkeypatch) as calls:
        got16, got1 = ops.knn_jobs([(sup, qry, 16), (gc.t, sup, 1)], B)
        want16 = ops.knn_batch(cloud[:, :77].contiguous(), cloud[:, :33].contiguous(), 16)
        want1 = ops.knn_batch(cloud, cloud[:, :77].contiguous(), 1)
        wide = gb.guard(torch.randn(3, 7, 5, 6, generator=g).cuda())
        views = [wide.t[:, 2:5], wide.t[:, :, 1:4], wide.t[1:, 6:, 4:]]
        dense = ops.copy_views(views)
    torch.cuda.synchronize()
    gc.check("gdm_knn_jobs_ws_hip", "jobs[].support / query")
    wide.check("gdm_copy_jobs_hip", "jobs[].src")
    assert gb.same_bits(gc.t, cloud)
    assert torch.equal(got16, want16) and torch.equal(got1, want1)
    for v, d in zip(views, dense):
        assert d.is_contiguous() and torch.equal(d, v)
    assert calls.counts["gdm_knn_jobs_ws_hip"] >= 1 and calls.counts["gdm_copy_jobs_hip"] == 1 and calls.counts["gdm_knn_batch_hip"] == 2


# --------------------------------------------------------------------------------------
# 6. matching and the matching losses
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1])
def test_match_1x200x333(ops, monkeypatch, prec):
    import test_gpu_ops as t
    _three_ways(monkeypatch, t.test_match_vs_oracle, ops, prec, 1, 200, 333)


@pytest.mark.parametrize("prec", [0, 1])
def test_match_soft_1x200x333(monkeypatch, prec):
    import test_gpu_match_soft as t

    def body():
        t._soft.cache_clear()                               # the module keeps its launches' results: launch again in every run
        t.test_soft_outputs_vs_fp64_restatement(1, 200, 333, prec, t.GAMMAS[0])
    try:
        plain = _three_ways(monkeypatch, body)
    finally:
        t._soft.cache_clear()
    assert {"gdm_match_pack2_hip", "gdm_match_soft_packed_hip", "gdm_match_packed_hip"} <= {n for n, _ in plain.record}


def test_soft_coord_match_smallest_case(monkeypatch):
    import test_gpu_soft_coord as t
    for R, M in sorted(t.SHAPES, key=lambda s: s[0] * s[1])[:2]:          # the two smallest cases of tests/soft_coord_cases.py: (1, 1), (5, 31)
        _three_ways(monkeypatch, t.test_forward_within_the_bounds_of_6k, R, M, t.GAMMAS[1])
        _three_ways(monkeypatch, t.test_backward_within_the_derived_bounds, R, M, t.GAMMAS[1])


def body_circle(ops):
    """circle_match forward and backward at R = 130 rows against M = 129 vertices (one row and one column over a 128 tile), against
    the fp64 restatement of tests/train_replay.py (r_circle_match) at the tolerances its table holds the Function to (1e-4, from
    tests/test_gpu_model.py::test_fused_matching_loss_training_shape_and_empty_positive_sets), gradients in both of its measures."""
    import train_replay as tr
    g = torch.Generator().manual_seed(15)
    R, M, B = 130, 129, 2
    xyz = ((torch.rand(M, 3, generator=g) - 0.5) * 0.1).cuda()
    vis = (torch.rand(B, M, generator=g) < 0.6).to(torch.uint8).cuda()
    gt = torch.randint(0, M + 1, (R,), generator=g, dtype=torch.int32)
    gt[-1], gt[-2] = M - 1, M                            # the last rows: the last vertex, and "no vertex" (the padding column)
    item = torch.sort(torch.randint(0, B, (R,), generator=g, dtype=torch.int32))[0].cuda()
    gt = gt.cuda()
    x0 = torch.nn.functional.normalize(torch.randn(R, 128, generator=g), dim=1).cuda()
    y0 = torch.nn.functional.normalize(torch.randn(M, 128, generator=g), dim=1).cuda()
    w = torch.rand(R, generator=g).cuda()
    nbr, visb = ops.circle_nbr_table(xyz, 0.02), ops.circle_visbits(vis)
    x, y = x0.clone().requires_grad_(True), y0.clone().requires_grad_(True)
    loss = ops.circle_match(x, y, gt, item, nbr=nbr, visb=visb)
    (loss * w).sum().backward()
    x64, y64 = x0.double().requires_grad_(True), y0.double().requires_grad_(True)
    want = tr.r_circle_match(None, torch.float64, x64, y64, gt, None, item, nbr, visb, 16.0, 0.2)
    (want * w.double()).sum().backward()
    entry = tr.TABLE["_CircleMatch"]
    assert tr.rel_err(loss.detach(), want.detach()) < entry.fwd
    for got_g, want_g in ((x.grad, x64.grad), (y.grad, y64.grad)):
        assert tr.rel_err(got_g, want_g) < entry.bwd and tr.scale_free_err(got_g, want_g) < entry.bwd
    # the materialised form on the same rows (gdm_circle_rows_*_hip over the [R, M + 1] similarity), against its own restatement
    xb, yb = x0.clone().requires_grad_(True), y0.clone().requires_grad_(True)
    pad = torch.full((1, 128), -1.0 / 128 ** 0.5, device="cuda")
    rows = ops.circle_rows(xb @ torch.cat([yb, pad], dim=0).t(), gt, item, xyz, vis, 0.02)
    (rows * w).sum().backward()
    rentry = tr.TABLE["_CircleRows"]
    assert tr.rel_err(rows.detach(), want.detach()) < rentry.fwd
    assert tr.rel_err(xb.grad, x64.grad) < rentry.bwd and tr.rel_err(yb.grad, y64.grad) < rentry.bwd
    # one positive table per item (gdm_circle_match_nbr_items_hip) with every radius equal: the tables of the shared form
    items = ops.circle_nbr_items(xyz, torch.full((B, M), 0.02, device="cuda"))
    d = (xyz.double()[:, None] - xyz.double()[None]).pow(2).sum(2).add(1e-7).sqrt()
    sure = (d - 0.02).abs() > 1e-6                     # away from the threshold the fp32 comparison is the fp64 one
    for b in range(B):
        assert torch.equal(tr._bits(items[b], M)[sure], (d < 0.02)[sure])
    x2, y2 = x0.clone().requires_grad_(True), y0.clone().requires_grad_(True)
    assert tr.rel_err(ops.circle_match(x2, y2, gt, item, nbr=items, visb=visb), want.detach()) < entry.fwd


def test_circle_match_R130_M129(ops, monkeypatch):
    _three_ways(monkeypatch, body_circle, ops)


# --------------------------------------------------------------------------------------
# 7. misaligned addresses: refusals, and the contract at the level of `ops`
# --------------------------------------------------------------------------------------
def _offset_view(t):
    """A contiguous view of the same values 4 bytes into its own allocation: what ops._dev lets through as it is."""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    base[1:] = t.reshape(-1)
    v = base[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _refusal_bodies(ops):
    """entry of SKEW_REFUSE -> a body that reaches it with every listed parameter present, or {parameter: body} where no one call
    carries them all.  Bodies from other test modules bring their own assertions; here only the refusal matters."""
    import test_gpu_dgcnn_fused as td
    import test_gpu_dgcnn_train as tdt
    import test_gpu_instances as ti
    import test_gpu_match_soft as ms
    import test_gpu_ops as t
    import test_gpu_p2r_epilogue as tp
    import test_gpu_pose_robust as tpr
    import test_gpu_soft_coord as tsc
    import test_gpu_spline_train as tst
    import test_gpu_targets as tg
    import test_gpu_train as tt
    g = torch.Generator().manual_seed(16)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    idx40 = torch.randint(0, 5, (1, 40), generator=g).int().cuda()

    def soft():
        ms._soft.cache_clear()
        try:
            ms.test_soft_outputs_vs_fp64_restatement(1, 200, 333, 1, ms.GAMMAS[0])
        finally:
            ms._soft.cache_clear()

    conv = lambda: t.test_conv3x3_bf16x3_vs_fp32_conv(ops, 1, 128, 72, 5, 32)
    strided = lambda: t.test_strided_conv3x3_and_conv1x1_downsample_vs_fp64(ops, 1, 128, 136, 4, 64)
    wgrad = lambda: tt.test_conv3x3_weight_gradient_on_the_mfma_gemm_equals_autograd(1, 256, 72, 4, 32, 1)
    wgrad1 = lambda: tt.test_pixel_contraction_weight_gradient_of_a_1x1_product_equals_fp64(3, 1024, 2304, 256)
    bn = lambda: tt.test_fused_batchnorm_act_training_matches_modules((3, 8, 100), 2)
    edge_train = lambda: tdt.test_edge_block_train_vs_fp64_autograd(*tdt.STAGE_CASES[0])
    spline = lambda: tst.test_kernels_against_fp64("m12", 128, True)
    targets = lambda: tg.test_visibility_equals_reference(_golden("pose_targets"), tg.CASES[0], "default")
    mfma64 = lambda pm, tpm: ops.conv64_gather_add_act_mfma(r(1, 64, 40), ops.pack_rows64(r(64, 64)), r(1, 5, 64) if tpm else r(1, 64, 5), idx40,
                                                            r(64), r(64), 1, 0.0, pixel_major=pm, t_point_major=tpm)
    return {
        "gdm_affine_act_hip": lambda: ops.affine_act(r(2, 5, 8), r(5), r(5), 1, 0.0, res=r(2, 5, 8), inplace=False),
        "gdm_affine_act_maxk_hip": lambda: ops.affine_act_maxk(r(1, 3, 9, 4), r(3), r(3), 1, 0.0),
        "gdm_prelu1_hip": tt.test_prelu1_forward_backward_equals_torch,
        "gdm_prelu1_bwd_hip": tt.test_prelu1_forward_backward_equals_torch,
        "gdm_psp_combine2_hip": lambda: t.test_psp_combine_with_packed_output(ops, 1, 64, 8, 32),
        "gdm_bn_stats_hip": bn, "gdm_bn_fwd_apply_hip": bn, "gdm_bn_bwd_reduce_hip": bn, "gdm_bn_bwd_apply_hip": bn,
        "gdm_edge_block_hip": lambda: td.test_edge_block_vs_fp64_restatement(2, 9, 33, 5, True, 64, 133),
        "gdm_edge_stats_hip": edge_train, "gdm_edge_bwd_reduce_hip": edge_train, "gdm_edge_bwd_mid_hip": edge_train,
        "gdm_edge_bwd_scatter_hip": edge_train,
        "gdm_conv3x3_strided_hip": conv,
        "gdm_conv1x1_strided_hip": strided,
        "gdm_conv1x1_packed_hip": lambda: t.test_gemm_bf16x3(ops, 1, 64, 128, 32),
        "gdm_conv1x1_packed_wb_hip": wgrad,
        "gdm_conv1x1_gather_add_hip": lambda: body_p2r_epilogue(ops, False),
        "gdm_gemm_grouped_hip": lambda: body_gemm_grouped(ops, 256),
        "gdm_pointwise2_hip": lambda: ops.pointwise([r(2, 8, 68)], r(8, 8)),
        "gdm_wgrad_direct_hip": lambda: ti.test_wgrad_direct_every_block_shape(ops, 8, 8),
        "gdm_knn_jobs_ws_hip": lambda: ops.knn_jobs([(torch.rand(2, 77, 3, device="cuda"), torch.rand(2, 33, 3, device="cuda"), 16)], 2),
        "gdm_gather_add_affine_act2_hip": lambda: tp.test_fused_epilogue_equals_the_two_launches(ops, "A", 0),
        "gdm_conv1x1_gather_add_act2_hip": lambda: ops.conv1x1_gather_add_act(r(1, 64, 40), r(64, 64), r(1, 64, 5), idx40, r(64), r(64), 1, 0.0,
                                                                              pixel_major=True),
        "gdm_conv64_gather_add_act_mfma2_hip": {"t": lambda: mfma64(False, True), "y": lambda: mfma64(True, False),
                                                "ypk": lambda: t.test_conv64_fusion_kernel_packed_output(ops, 1, 8, 32, 5, 1)},
        "gdm_conv64_gather_add_final_hip": lambda: ops.conv64_gather_add_final(r(1, 64, 40), ops.pack_rows64(r(64, 64)), r(1, 5, 64), idx40, r(64), r(64),
                                                                               1, 0.0, r(64, 64), None),
        "gdm_soft_coord_fwd_hip": lambda: tsc.test_backward_within_the_derived_bounds(5, 31, tsc.GAMMAS[1]),
        "gdm_soft_coord_bwd_hip": lambda: tsc.test_backward_within_the_derived_bounds(5, 31, tsc.GAMMAS[1]),
        "gdm_upconv3x3_gather2_hip": lambda: t.test_upconv_gather_eight_channel_form_with_packed_output(ops, 1, 64, 8, 32, 1),
        "gdm_stem_hip": lambda: t.test_stem_kernel_vs_torch_fp64(ops, 1, 128, 128),
        "gdm_stem_pack_weight_hip": lambda: t.test_stem_kernel_vs_torch_fp64(ops, 1, 7, 9),
        "gdm_match_pack_hip": lambda: ops.match_pack(r(1, 128, 37), ops.MATCH_F32),
        "gdm_match_pack2_hip": lambda: t.test_match_pack2_equals_two_pack_launches(ops, "MATCH_F32", 3, 100, 37),
        "gdm_match_hip": lambda: t.test_match_vs_oracle(ops, 1, 1, 200, 333),
        "gdm_match_packed_hip": soft,
        "gdm_match_soft_packed_hip": soft,
        "gdm_circle_match_pack_hip": lambda: body_circle(ops), "gdm_circle_match_fwd2_hip": lambda: body_circle(ops),
        "gdm_circle_match_bwd2_hip": lambda: body_circle(ops),
        "gdm_wgrad_pack_x_hip": wgrad, "gdm_wgrad_pack_go_hip": wgrad, "gdm_wgrad_pack_x1_hip": wgrad1,
        "gdm_spline_segment_sum_hip": spline, "gdm_spline_wgrad_hip": spline, "gdm_spline_pairs_grad_hip": spline,
        "gdm_hpr_visible_hip": targets,
        "gdm_pose_targets_hip": lambda: tg.test_pose_gt_info_equals_reference(_golden("pose_targets"), tg.CASES[0]),
        "gdm_ransac_pose_hip": lambda: tpr.test_ransac_matches_reference_golden(_golden("pose_robust")),
    }


REFUSALS = [(e, p) for e in sorted(gb.SKEW_REFUSE) for p in gb.SKEW_REFUSE[e]]


@pytest.mark.parametrize("entry,param", REFUSALS, ids=["%s-%s" % (e[4:-4], p) for e, p in REFUSALS])
def test_unaligned_addresses_are_refused_before_any_launch(ops, monkeypatch, entry, param):
    """Every row of SKEW_REFUSE, one parameter at a time: with that argument 4 bytes off a 16-byte boundary the entry raises a
    GdmError that speaks of the alignment, before any launch -- guarded_calls has verified that every band AND every interior of that
    call is untouched -- and the entry never ran.  (The error is read from the wrapper's record: a body may wrap what it catches.)"""
    bodies = _refusal_bodies(ops)
    assert set(bodies) == set(gb.SKEW_REFUSE)
    body = bodies[entry][param] if isinstance(bodies[entry], dict) else bodies[entry]
    with gb.guarded_calls(monkeypatch, skew=4, only=(entry,), skew_params=(param,)) as calls:
        with pytest.raises(Exception):
            body()
    assert entry in calls.refused, "%s was not refused with `%s` off alignment" % (entry, param)
    assert calls.refused[entry].startswith("GdmError") and "align" in calls.refused[entry], calls.refused[entry]


def test_a_contiguous_view_at_a_4_byte_offset_gives_the_right_answer_or_is_refused(ops):
    """The contract at the level of `ops`: ops._dev passes any contiguous view through, so a view 4 bytes into its allocation reaches
    the library.  It gives the answer the aligned tensor gives (bit for bit where the op selects, at the op's bound otherwise) or a
    GdmError raised before any launch -- never another result."""
    from geometric_aware_dense_matching_amd import _lib
    g = torch.Generator().manual_seed(17)
    feat = torch.randn(2, 3, 1028, generator=g).cuda()
    idx = torch.randint(0, 1028, (2, 257, 16), generator=g).int().cuda()
    want = ops.gather_max(feat, idx)
    assert torch.equal(ops.gather_max(_offset_view(feat), idx), want) and torch.equal(ops.gather_max(feat, _offset_view(idx)), want)
    small, sidx = torch.randn(2, 9, 36, generator=g).cuda().requires_grad_(True), torch.randint(0, 36, (2, 37, 16), generator=g).int().cuda()
    go = torch.randn(2, 9, 37, 16, generator=g).cuda()
    (ga,) = torch.autograd.grad(ops.group_gather(small, sidx), small, go)
    (gv,) = torch.autograd.grad(ops.group_gather(small, _offset_view(sidx)), small, _offset_view(go))
    _close(gv, _scatter64(go.cpu(), sidx.cpu(), 36), 1e-5, "group_gather backward from offset views")
    _close(ga, _scatter64(go.cpu(), sidx.cpu(), 36), 1e-5, "group_gather backward")
    att, f = torch.randn(2, 5, 33, 16, generator=g).cuda(), torch.randn(2, 5, 33, 16, generator=g).cuda()
    w64 = (torch.softmax(att.double(), 3) * f.double()).sum(3)
    for a, b in ((att, f), (_offset_view(att), f), (att, _offset_view(f))):
        assert torch.allclose(ops.att_pool(a, b).double(), w64, rtol=1e-5, atol=1e-6)
    x = torch.randn(2, 3, 3, 3, generator=g).cuda()
    assert torch.equal(ops.upsample_bilinear(_offset_view(x), (5, 33)), ops.upsample_bilinear(x, (5, 33)))
    xk = torch.randn(1, 8, 100, generator=g).cuda()
    (ik, vk), (io, vo) = ops.feature_knn(xk, 5, return_values=True), ops.feature_knn(_offset_view(xk), 5, return_values=True)
    sq = (xk[0] ** 2).sum(0).double()
    score = 2 * (xk[0].double().t() @ xk[0].double()) - sq[:, None] - sq[None, :]             # dgcnn.py:22-25 in fp64
    for i_, v_ in ((ik, vk), (io, vo)):
        # every selected column's score is the value reported, and no unselected column beats the k-th by more than rounding
        assert (torch.gather(score, 1, i_[0].long()) - v_[0].double()).abs().max().item() < 1e-4 * max(1.0, score.abs().max().item())
        assert (score.topk(5, dim=1)[0] - v_[0].double()).abs().max().item() < 1e-4 * max(1.0, score.abs().max().item())
    seg, wt = torch.randn(2, 8, 68, generator=g).cuda(), (torch.randn(8, 8, generator=g) / 3).cuda()
    want = torch.einsum("kc,bkn->bcn", wt.double(), seg.double())
    for s, w in ((seg, wt), (_offset_view(seg), wt), (seg, _offset_view(wt))):
        _close(ops.pointwise([s], w), want, 1e-5, "pointwise from an offset view")
    sc, sh = torch.randn(64, generator=g).cuda(), torch.randn(64, generator=g).cuda()
    # a point-major point term 4 bytes off: ops.conv64_gather_add_act_mfma / conv64_gather_add_final clone it (16-byte row loads)
    x64, t64 = torch.randn(1, 64, 40, generator=g).cuda(), torch.randn(1, 5, 64, generator=g).cuda()
    i64 = torch.randint(0, 5, (1, 40), generator=g).int().cuda()
    wpk, wf = ops.pack_rows64((torch.randn(64, 64, generator=g) / 8).cuda()), (torch.randn(64, 64, generator=g) / 8).cuda()
    assert torch.equal(ops.conv64_gather_add_act_mfma(x64, wpk, _offset_view(t64), i64, sc, sh, 1, 0.0, t_point_major=True),
                       ops.conv64_gather_add_act_mfma(x64, wpk, t64, i64, sc, sh, 1, 0.0, t_point_major=True))
    assert torch.equal(ops.conv64_gather_add_final(x64, wpk, _offset_view(t64), i64, sc, sh, 1, 0.0, wf, None),
                       ops.conv64_gather_add_final(x64, wpk, t64, i64, sc, sh, 1, 0.0, wf, None))
    # refused: the library checks the address before it launches
    pq, eidx = torch.randn(1, 33, 128, generator=g).cuda(), torch.randint(0, 33, (1, 33, 5), generator=g).int().cuda()
    with pytest.raises(_lib.GdmError, match="align"):
        ops.edge_block(_offset_view(pq), eidx, sc, sh)
    with pytest.raises(_lib.GdmError, match="align"):
        ops.affine_act_maxk(_offset_view(torch.randn(1, 3, 9, 4, generator=g).cuda()), sc[:3].contiguous(), sh[:3].contiguous(), 1, 0.0)
    # a residual 4 bytes off: ops.affine_act and ops.conv3x3_bf16x3 clone it (both kernels read it 16 bytes at a time)
    res, xa = torch.randn(2, 5, 8, generator=g).cuda(), torch.randn(2, 5, 8, generator=g).cuda()
    s5, b5 = sc[:5].contiguous(), sh[:5].contiguous()
    assert torch.equal(ops.affine_act(xa, s5, b5, res=_offset_view(res), inplace=False), ops.affine_act(xa, s5, b5, res=res, inplace=False))
    xc, rc = torch.randn(1, 128, 4, 32, generator=g).cuda(), torch.randn(1, 72, 4, 32, generator=g).cuda()
    wc = ops.conv3x3_pack_weight((torch.randn(72, 128, 3, 3, generator=g) / 34).cuda())
    assert torch.equal(ops.conv3x3_bf16x3(xc, wc, 72, None, None, ops.ACT_RELU, _offset_view(rc)),
                       ops.conv3x3_bf16x3(xc, wc, 72, None, None, ops.ACT_RELU, rc))
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------
# 8. breadth: the suite's own bodies under guards, and which entries ran
# --------------------------------------------------------------------------------------
def _golden(name):
    """A recorded fixture of tests/golden, as the module-scoped `gold` fixtures of the other test modules load it."""
    import os
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")))


def _bop_scene():
    """The `scene` of tests/test_gpu_bop_errors.py: the mesh, the poses and the restatement's images."""
    import test_gpu_bop_errors as tb
    gold = _golden("bop_errors")
    verts, faces = tb.bi.mesh()
    est, gt = tb.bi.poses()
    return dict(verts=verts, faces=faces, est=est, gt=gt, d_est=gold["vsd_depth_est"], d_gt=gold["vsd_depth_gt"],
                d_test=gold["vsd_depth_test"], diameter=float(gold["vsd_diameter"]), errors=gold["vsd_errors"])


def _breadth():
    import test_gpu_bop_errors as tb
    import test_gpu_frontend_augment as tfa
    import test_gpu_frontend_boxes as tfb
    import test_gpu_frontend_fill as tff
    import test_gpu_frontend_sample as tfs
    import test_gpu_icp_plane as tip
    import test_gpu_instances as ti
    import test_gpu_ops as t
    import test_gpu_pointops as tp
    import test_gpu_pose_robust as tpr
    import test_gpu_pose_shapes as tps
    import test_gpu_spline_train as tst
    import test_gpu_targets as tg
    import test_gpu_train as tt
    from geometric_aware_dense_matching_amd import ops as o
    from geometric_aware_dense_matching_amd import pointops as po
    tgold = lambda: _golden("pose_targets")
    scene = _bop_scene
    return {
        "pointops-three-nn-interpolation": lambda: tp.test_three_nn_and_interpolation_forward_backward(po),
        "pointops-grouping-gathering": lambda: tp.test_grouping_gathering_and_int_payload(po),
        "pointops-ballquery-labelstats": lambda: tp.test_ballquery_labelstats_and_featuredistribute(po),
        "pointops-knn-queries": lambda: tp.test_knn_queries_and_group_modules(po),
        "ops-ballquery-fps": lambda: t.test_pointops_ballquery_fps(o),
        "targets-flipped-points": lambda: tg.test_flipped_points_equal_documented_formula(tgold(), tg.CASES[0]),
        "targets-visibility": lambda: tg.test_visibility_equals_reference(tgold(), tg.CASES[0], "default"),
        "targets-pose-gt-info": lambda: tg.test_pose_gt_info_equals_reference(tgold(), tg.CASES[0]),
        "frontend-depth-normals": lambda: tfb.test_depth_normals_equal_the_restatement(),
        "frontend-crop-from-boxes": lambda: tfb.test_crop_from_boxes_equals_the_restatement(),
        "frontend-identity-boxes": lambda: tfb.test_identity_boxes_equal_make_inputs(),
        "frontend-fill-fast": lambda: tff.test_stages_equal_the_restatement(sorted(tff.BATCHES)[0], "fast"),
        "frontend-fill-multiscale": lambda: tff.test_stages_equal_the_restatement(sorted(tff.BATCHES)[0], "multiscale"),
        "frontend-sample": lambda: tfs.test_kernel_equals_the_restatement(True),
        "frontend-augment": lambda: tfa.test_kernel_equals_the_restatement(32, tfa.SEEDS),
        "frontend-dzi-boxes": lambda: tfa.test_dzi_boxes_hash_equals_the_restatement(),
        "bop-render-depth": lambda: tb.test_render_depth_follows_the_pixel_rule(scene(), torch.float32),
        "bop-vsd-counts": lambda: tb.test_vsd_counts_equal_the_restatement_and_the_reference(scene(), False),
        "bop-mssd-mspd": lambda: tb.test_mssd_mspd_many_points_and_ties(),          # (the parametrised body measures allocations)
        "pose-ransac-golden": lambda: tpr.test_ransac_matches_reference_golden(_golden("pose_robust")),
        "pose-icp-golden": lambda: tpr.test_icp_matches_reference_golden(_golden("pose_robust")),
        "pose-kabsch-stats": lambda: tps.test_kabsch_stats_vs_fp64_sum(65, 1),
        "pose-kabsch-solve": lambda: tps.test_kabsch_solve_vs_svd(1, 5),
        "icp-plane-starved-crops": lambda: tip.test_starved_crops_stop_unchanged(),     # (the one-iteration bodies call the C ABI directly)
        "icp-plane-degenerate-models": lambda: tip.test_degenerate_models_are_frozen_and_flagged("plane"),
        "match-score": _match_score,
        "conv64-gather-add-final": lambda: __import__("test_gpu_fused_passes").test_fused_fusion_final_without_bias_and_with_int64_index(o),
        "training-step-dense-mesh-branch": lambda: _training_step(False),
        "spline-train-m12": lambda: tst.test_kernels_against_fp64("m12", 9, True),
        "spline-train-m12-128": lambda: tst.test_kernels_against_fp64("m12", 128, False),
        "spline-scalar-kernels": lambda: t.test_spline_scalar_kernels_for_odd_channel_counts(o),
        "spline-layers-without-relu": lambda: ti.test_spline_layers_without_relu(o),
        "knn-oracle-smallest": lambda: t.test_knn_matches_oracle_bit_exact(o, 512, 2048, 1),
        "knn-cell-list-few": lambda: t.test_knn_cell_list_search_equals_oracle(o, "few"),
        "knn1-job-table-s64": lambda: t.test_knn1_through_job_table_equals_oracle(o, "s64"),
        "knn-organised-24x40": lambda: t.test_knn_organised_support_window_search_equals_brute_force(o, 24, 40, 5, 77, 1.0),
        "seg-mask": lambda: t.test_seg_mask(o),
        "match-pack2": lambda: t.test_match_pack2_equals_two_pack_launches(o, "MATCH_F32", 3, 100, 37),
        "topk-negdist": lambda: ti.test_topk_negdist_with_few_neighbours(o, 4),
        "gather-add-affine-act": lambda: ti.test_gather_add_affine_act_every_activation(o, 2),
        "conv1x1-gather-add-act": lambda: t.test_conv1x1_gather_add_act(o, 1),
        "upconv-kernels": lambda: ti.test_upconv_kernels_every_activation(o, 2),
        "wgrad-direct": lambda: ti.test_wgrad_direct_every_block_shape(o, 8, 8),
        "wgrad-pixel-contraction": lambda: tt.test_pixel_contraction_weight_gradient_of_a_1x1_product_equals_fp64(3, 1024, 2304, 256),
        "conv1x1-train": lambda: tt.test_conv1x1_train_as_batched_gemms_equals_torch_convolution((3, 16, 50), 24, True),
        "wx-training-products": lambda: tt.test_wx_training_products_on_the_mfma_gemm_equal_fp64_autograd(2, 64, 32, 1000, False),
        "edge-block-train": lambda: __import__("test_gpu_dgcnn_train").test_edge_block_train_vs_fp64_autograd(
            *__import__("test_gpu_dgcnn_train").STAGE_CASES[0]),
        "edge-block-train-one-layer": lambda: __import__("test_gpu_dgcnn_train").test_edge_block_train_batch_statistics_and_forward_kernel(),
        "match-soft-score-and-fit": lambda: __import__("test_gpu_match_soft").test_weighted_statistics_and_fit("soft"),
        "circle-rows-and-match-in-a-training-step": _training_step,
    }


def _match_score():
    """ops.match_score at (B, N) = (3, 257), one crop with an empty mask, through tests/test_gpu_match_soft.py::_check_score
    (2^-24: one rounding of an fp64 mean in [0, 1]).  (The suite's own caller of it captures a graph, which guarded_calls refuses.)"""
    import test_gpu_match_soft as ms
    from geometric_aware_dense_matching_amd import ops as o
    g = torch.Generator().manual_seed(18)
    conf = torch.rand(3, 257, generator=g).cuda()
    mask = (torch.rand(3, 257, generator=g) < 0.6).to(torch.uint8)
    mask[1] = 0
    mask[2, -1] = 1
    ms._check_score(dict(conf=conf, mask=mask.cuda(), score=o.match_score(conf, mask.cuda())))


def _training_step(grouped=True):
    """One forward + backward of the FFB6D variant in train mode (B = 2, N = 1024, M = 512, the step of tests/test_gpu_train_replay.py),
    every library call under guards: the circle losses, the batch-norm kernels, the weight gradients and the mesh branch at the
    shapes the network itself gives them.  The loss must be finite; what each call computes is held to fp64 by that module."""
    import test_gpu_train_replay as r
    model = r._ffb6d(grouped=grouped)
    r._step(model, [], "guarded")


BREADTH = ["pointops-three-nn-interpolation", "pointops-grouping-gathering", "pointops-ballquery-labelstats", "pointops-knn-queries",
           "ops-ballquery-fps", "targets-flipped-points", "targets-visibility", "targets-pose-gt-info", "frontend-depth-normals",
           "frontend-crop-from-boxes", "frontend-identity-boxes", "frontend-fill-fast", "frontend-fill-multiscale", "frontend-sample",
           "frontend-augment", "frontend-dzi-boxes", "bop-render-depth", "bop-vsd-counts", "bop-mssd-mspd", "pose-ransac-golden",
           "pose-icp-golden", "pose-kabsch-stats", "pose-kabsch-solve", "icp-plane-starved-crops", "icp-plane-degenerate-models",
           "match-score", "conv64-gather-add-final", "training-step-dense-mesh-branch", "spline-train-m12", "spline-train-m12-128",
           "spline-scalar-kernels", "spline-layers-without-relu", "knn-oracle-smallest", "knn-cell-list-few", "knn1-job-table-s64",
           "knn-organised-24x40", "seg-mask", "match-pack2", "topk-negdist", "gather-add-affine-act", "conv1x1-gather-add-act",
           "upconv-kernels", "wgrad-direct", "wgrad-pixel-contraction", "conv1x1-train", "wx-training-products", "edge-block-train",
           "edge-block-train-one-layer", "match-soft-score-and-fit", "circle-rows-and-match-in-a-training-step"]


@pytest.mark.parametrize("case", BREADTH)
def test_the_suites_own_bodies_under_guards(monkeypatch, case):
    """Each body keeps its own fp64 (or bit-exact) assertions; the wrapper adds the memory check to every library call it makes."""
    table = _breadth()
    assert set(BREADTH) == set(table)
    with gb.guarded_calls(monkeypatch) as calls:
        table[case]()
    assert sum(calls.counts.values()) > 0, "the body made no library call"


# entries that never run under guards here, one reason each; at most 10 % of the `*_hip` entries of include/gdm.h
NOT_GUARDED = {
    "gdm_mfma_probe_hip": "a probe of the MFMA lane layout, no part of the product path (tests/test_gpu_ops.py::test_mfma_probes_run)",
    "gdm_mfma_probe_lds_hip": "the same probe through LDS",
    "gdm_conv3x3_packed_hip": "no caller in the package since the stride argument: ops reaches the kernel through gdm_conv3x3_strided_hip",
}


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_guarded_calls_refuse_inside_graph_capture(ops, monkeypatch):
    """The wrapper allocates and synchronises: while the current stream captures it raises instead of doing either."""
    conf, mask = torch.rand(2, 70, device="cuda"), torch.ones(2, 70, dtype=torch.uint8, device="cuda")
    ops.match_score(conf, mask)                          # (warm: nothing is allocated lazily inside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with gb.guarded_calls(monkeypatch):
        with pytest.raises(RuntimeError, match="capture"):
            with torch.cuda.graph(graph):
                ops.match_score(conf, mask)


def test_every_hip_entry_ran_under_guards(request):
    """From the wrapper's per-entry counts over this file: every `*_hip` entry of include/gdm.h ran under guard bands at least once,
    but for NOT_GUARDED.  (It needs the whole file: with only a part of its tests selected it fails and says so.)"""
    selected = sum(1 for i in request.session.items if i.parent is request.node.parent)
    whole = len(request.node.parent.collect())
    if selected != whole:
        pytest.fail("only %d of the %d tests of this file were selected: the count of guarded entries needs them all" % (selected, whole))
    assert set(NOT_GUARDED) <= set(gb.HIP_ENTRIES) and len(NOT_GUARDED) <= len(gb.HIP_ENTRIES) // 10
    missing = sorted(n for n in gb.HIP_ENTRIES if gb.COUNTS[n] == 0 and n not in NOT_GUARDED)
    ran = sum(1 for n in gb.HIP_ENTRIES if gb.COUNTS[n] > 0)
    print("%d of %d *_hip entries ran under guards; never: %s" % (ran, len(gb.HIP_ENTRIES), missing))
    assert not missing, missing
    assert ran >= 0.9 * len(gb.HIP_ENTRIES)
    assert not [n for n in NOT_GUARDED if gb.COUNTS[n]], "an entry listed as never guarded did run: take it off the list"

