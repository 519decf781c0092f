"""Guard bands (tests/guard_bands.py) round the launch sequence of dual-softmax matching: gdm_match_dual_packed_hip.  Every tensor
argument sits between two 1 MiB bands of 0xFF, the bands and the interior of every const argument are looked at after the call, and
every output must hold the bytes of the plain run -- also with the outputs 4 bytes off a 16-byte boundary, which the rule allows (they
are written one element at a time); the packed rows and the workspace off that boundary are refused before any launch.

(The file's name sorts in front of tests/test_gpu_guard_bands.py, whose last test counts the `*_hip` entries that ran under guards in
the process so far: the new entry is counted here, as tests/test_gpu_guard_band_match_twoway.py does for its own.)"""
import pytest
import torch

import guard_bands as gb
import match_dual_cases as dc
import match_twoway_cases as mc
from geometric_aware_dense_matching_amd import _lib

pytestmark = pytest.mark.gpu

ENTRY = "gdm_match_dual_packed_hip"
OUTPUTS = ("best_idx", "best_sim", "lse", "conf", "soft_xyz", "col_idx", "col_sim", "col_lse", "col_conf", "dual")


@pytest.fixture(scope="module")
def ops():
    from geometric_aware_dense_matching_amd import ops as o
    return o


def _body(ops, B, N, M, prec, kind):
    scene, model = mc.descriptors(B, N, M)
    xyz = torch.from_numpy(dc.model_xyz(M)).cuda()
    mask = torch.from_numpy(dc.mask(B, N, kind)).cuda()
    srows, mrows = ops.match_pack2(torch.from_numpy(scene).cuda(), torch.from_numpy(model).cuda(), prec)
    got = {}

    def body():
        got["out"] = ops.match_dual_packed(srows, mrows, xyz, mask, B, N, M, prec, 16.0)
    return body, got


@pytest.mark.parametrize("skew", [0, 4])
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("B,N,M", [(2, 70, 200), (2, 300, 513), (5, 20, 300)])
def test_dual_between_guards(ops, monkeypatch, B, N, M, prec, skew):
    """(2,70,200): one partial row block per crop, the one panel partial; (2,300,513): two row blocks per crop, the second 44 rows
    long, a last panel one column wide; (5,20,300): row blocks of 20 real rows.  The last rows and columns of the ten outputs, the
    rows behind a crop's end that a row block must not write, and the last column partial and the last Zc in the workspace are the
    stores nearest an edge."""
    assert tuple(ops.DUAL_KEYS) == OUTPUTS
    body, got = _body(ops, B, N, M, prec, "half")
    with gb.filled_empties():
        with gb.guarded_calls(monkeypatch, guard=False, record=True) as plain:
            body()
        want = [t.clone() for t in got["out"]]
        with gb.guarded_calls(monkeypatch, only=(ENTRY,), record=True, skew=skew, skew_params=OUTPUTS if skew else None) as guarded:
            body()
    assert guarded.counts[ENTRY] == 1, guarded.counts
    gb.assert_same_record(plain, guarded, skip=(ENTRY,))          # its workspace keeps row partials of either run
    for a, b in zip(want, got["out"]):
        assert gb.same_bits(a, b)
    assert bool((got["out"][9] > 0).any())                        # the case is not empty: some point holds a dual confidence


def test_rows_and_workspace_off_a_16_byte_boundary_are_refused(ops, monkeypatch):
    body, _ = _body(ops, 2, 70, 200, 0, "ones")
    for param in ("scene_rows", "model_rows", "partial"):
        with gb.guarded_calls(monkeypatch, only=(ENTRY,), skew=4, skew_params=(param,)) as calls:
            with pytest.raises(_lib.GdmError, match="16-byte aligned"):
                body()
        assert calls.counts[ENTRY] == 0 and ENTRY in calls.refused
