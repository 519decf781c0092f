"""Guard bands (tests/guard_bands.py) round the two launches of two-way matching: gdm_match_twoway_packed_hip and
gdm_match_cycle_hip.  Every tensor argument sits between two 1 MiB bands of 0xFF, the bands and the interior of every const argument
are looked at after the call, and every output must hold the bytes of the plain run -- also with the outputs 4 bytes off a 16-byte
boundary, which the rule allows (they are written one element at a time); the packed rows and the workspace off that boundary are
refused before any launch.

(The file's name sorts in front of tests/test_gpu_guard_bands.py, whose last test counts the `*_hip` entries that ran under guards in
the process so far: the two new entries are counted here, as tests/test_gpu_guard_band_match_sooner.py does for its own.)"""
import pytest
import torch

import guard_bands as gb
import match_twoway_cases as mc
from geometric_aware_dense_matching_amd import _lib

pytestmark = pytest.mark.gpu

ENTRIES = ("gdm_match_twoway_packed_hip", "gdm_match_cycle_hip")
OUTPUTS = ("best_idx", "best_sim", "col_idx", "col_sim", "pair_mask", "pair_count", "cycle_d2")


@pytest.fixture(scope="module")
def ops():
    from geometric_aware_dense_matching_amd import ops as o
    return o


def _body(ops, B, N, M, prec, kind):
    scene, model = mc.descriptors(B, N, M)
    cld = torch.from_numpy(mc.rng("guard cloud %d %d" % (B, N)).uniform(-0.05, 0.05, (B, 9, N)).astype("float32")).cuda()
    mask = torch.from_numpy(mc.mask(B, N, kind)).cuda()
    srows, mrows = ops.match_pack2(torch.from_numpy(scene).cuda(), torch.from_numpy(model).cuda(), prec)
    got = {}

    def body():
        bi, bs, ci, cs = ops.match_twoway_packed(srows, mrows, mask, B, N, M, prec)
        got["out"] = (bi, bs, ci, cs) + tuple(ops.match_cycle(cld, bi, ci, mask, 0.02))
    return body, got, (srows, mrows)


@pytest.mark.parametrize("skew", [0, 4])
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", [(2, 70, 200), (2, 300, 513)])
def test_twoway_and_cycle_between_guards(ops, monkeypatch, B, N, M, prec, skew):
    """(2,70,200): the one row block is partial and spans both crops, the one panel is partial; (2,300,513): three row blocks, the
    crop boundary inside the second, a last panel one column wide.  The last rows and columns of the four matching outputs, the
    keys behind the row partials in the workspace, and the last points of the filter's three outputs are the stores nearest an edge."""
    body, got, _ = _body(ops, B, N, M, prec, "random")
    with gb.filled_empties():
        with gb.guarded_calls(monkeypatch, guard=False, record=True) as plain:
            body()
        want = [t.clone() for t in got["out"]]
        with gb.guarded_calls(monkeypatch, only=ENTRIES, record=True, skew=skew, skew_params=OUTPUTS if skew else None) as guarded:
            body()
    assert all(guarded.counts[n] == 1 for n in ENTRIES), guarded.counts
    gb.assert_same_record(plain, guarded, skip=("gdm_match_twoway_packed_hip",))          # its workspace keeps row partials of either run
    for a, b in zip(want, got["out"]):
        assert gb.same_bits(a, b)
    assert int(got["out"][5].sum()) > 0                                                   # the filter kept something: the case is not empty


def test_rows_and_workspace_off_a_16_byte_boundary_are_refused(ops, monkeypatch):
    body, _, _ = _body(ops, 2, 70, 200, 0, "ones")
    for param in ("scene_rows", "model_rows", "partial"):
        with gb.guarded_calls(monkeypatch, only=ENTRIES[:1], skew=4, skew_params=(param,)) as calls:
            with pytest.raises(_lib.GdmError, match="16-byte aligned"):
                body()
        assert calls.counts[ENTRIES[0]] == 0 and ENTRIES[0] in calls.refused
