"""Guard bands (tests/guard_bands.py) round the two launches that start matching sooner: the first mesh layer with its weight slice
in LDS (gdm_spline_direct3_hip, weights_in_lds = 1) and the heads kernel that writes the scene's matching rows
(gdm_point_heads3_hip).  Every tensor argument sits between two 1 MiB bands of 0xFF, the bands and the interior of every const
argument are looked at after the call, and every output must hold the bytes of the plain run.

(The file's name sorts in front of tests/test_gpu_guard_bands.py, whose last test counts the `*_hip` entries that ran under guards in
the process so far: the new entry gdm_point_heads3_hip is counted here, as tests/test_gpu_consensus.py does for its own.)"""
import numpy as np
import pytest
import torch

import guard_bands as gb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from geometric_aware_dense_matching_amd import ops as o
    return o


def _plain_and_guarded(monkeypatch, body, only):
    with gb.filled_empties():
        with gb.guarded_calls(monkeypatch, guard=False, record=True) as plain:
            body()
        with gb.guarded_calls(monkeypatch, only=only, record=True) as guarded:
            body()
    assert all(guarded.counts[n] >= 1 for n in only), guarded.counts
    gb.assert_same_record(plain, guarded)
    return plain


@pytest.mark.parametrize("M,Cin", [(1, 9), (200, 9), (333, 16)])
def test_lds_mesh_layer_out_out_t_and_packed_between_guards(monkeypatch, M, Cin):
    """M = 200 and 333 end inside a vertex run of 128 and inside a pass of 64 vertices: the last workgroups' tails are the stores
    nearest the end of `out`, the last columns of every row of `out_t`, and the last pixels of the packed planes."""
    import test_gpu_spline_lds as t
    from geometric_aware_dense_matching_amd import splinecnn
    c = t._case(M, Cin, 128, np.arange(M) % 7, 40 + M)

    def body():
        from geometric_aware_dense_matching_amd import _lib
        out = torch.empty(M, 128, device="cuda")
        out_t = torch.empty(128, M, device="cuda")
        pk = torch.zeros(_lib.lib().gdm_conv3x3_act_bytes(1, 128, 1, M), dtype=torch.uint8, device="cuda")
        splinecnn.call("gdm_spline_direct3_hip", c["x"], c["weight"], c["rowptr"], c["src"], c["attr"], c["root_t"], c["bias"], M, Cin, 128,
                       5, 1, out, out_t, pk, 1)
        old = [torch.empty_like(out), torch.empty_like(out_t), torch.zeros_like(pk)]
        splinecnn.call("gdm_spline_direct3_hip", c["x"], c["weight"], c["rowptr"], c["src"], c["attr"], c["root_t"], c["bias"], M, Cin, 128,
                       5, 1, old[0], old[1], old[2], 0)
        assert torch.equal(out, old[0]) and torch.equal(out_t, old[1]) and torch.equal(pk, old[2])

    _plain_and_guarded(monkeypatch, body, ("gdm_spline_direct3_hip",))


def test_lds_mesh_layer_takes_the_scalar_kernel_at_a_4_byte_offset(monkeypatch):
    """guard_bands.SKEW_BRANCH names weight / out / root_t / bias of gdm_spline_direct3_hip: 4 bytes off a 16-byte boundary neither the
    LDS kernel nor the 16-byte kernel applies, and the one-channel-per-thread kernel must give the row-major output alone
    (1e-5 * max |want| against the aligned run: another order of the four channels' loads, the same sums)."""
    import test_gpu_spline_lds as t
    from geometric_aware_dense_matching_amd import splinecnn
    M = 133
    c = t._case(M, 9, 128, np.full(M, 4), 9)
    got = {}

    def body(key):
        out = torch.empty(M, 128, device="cuda")
        splinecnn.call("gdm_spline_direct3_hip", c["x"], c["weight"], c["rowptr"], c["src"], c["attr"], c["root_t"], c["bias"], M, 9, 128, 5,
                       1, out, None, None, 1)
        got[key] = out

    with gb.guarded_calls(monkeypatch, only=("gdm_spline_direct3_hip",)):
        body("aligned")
    with gb.guarded_calls(monkeypatch, skew=4, only=("gdm_spline_direct3_hip",)) as skewed:
        body("skewed")
    assert skewed.counts["gdm_spline_direct3_hip"] == 1
    want = got["aligned"].double()
    assert (got["skewed"].double() - want).abs().max().item() < 1e-5 * max(1.0, want.abs().max().item())


class _HandGuardedHeads:
    """ops.point_heads with every layer's packed weight, scale and shift between guard bands placed by hand (their addresses travel in
    host arrays, which the generic wrapper cannot see); the tensor arguments -- a, b, out_feat, out_last, out_rows -- are the wrapper's."""

    def __init__(self, ops):
        self._ops, self.checked = ops, 0

    def point_heads(self, a, b, layers, last, feat_layer, res_layer, rows=False):
        guards, glayers = [], []
        for k, (w, sc, sh, act) in enumerate(layers):
            gs = [gb.guard(t) if t is not None else None for t in (w, sc, sh)]
            guards += [(g, "%s[%d]" % (n, k)) for g, n in zip(gs, ("w", "scale", "shift")) if g is not None]
            glayers.append(tuple(g.t if g is not None else None for g in gs) + (act,))
        ret = self._ops.point_heads(a, b, glayers, last, feat_layer, res_layer, rows=rows)
        torch.cuda.synchronize()
        for g, name in guards:
            g.check("gdm_point_heads3_hip", name)
        self.checked += 1
        return ret


@pytest.mark.parametrize("B,N,Ca", [(1, 65, 128), (2, 100, 64)])
def test_heads_rows_between_guards(ops, monkeypatch, B, N, Ca):
    """N = 65 and 100 leave a partial tile of 64 points: the last rows of the row buffer are the last workgroup's, and the rows past
    N -- which the kernel computes from zeros -- must not be written.  The bytes are those of ops.match_pack, guarded too."""
    import test_gpu_heads_rows as t
    layers, last = t._chain(ops, N)
    x0 = torch.from_numpy(np.random.RandomState(N).randn(B, 128, N).astype(np.float32)).cuda()
    hand = _HandGuardedHeads(ops)

    def body():
        a = x0[:, :Ca].contiguous()
        b = x0[:, Ca:].contiguous() if Ca < 128 else None
        feat, seg, rows = hand.point_heads(a, b, layers, last, 3, 4, rows=True)
        assert torch.equal(rows, ops.match_pack(feat, ops.MATCH_BF16X3))

    only = ("gdm_point_heads3_hip", "gdm_match_pack_hip")
    plain = _plain_and_guarded(monkeypatch, body, only)
    assert hand.checked == 2 and {n for n, _ in plain.record} == set(only)
