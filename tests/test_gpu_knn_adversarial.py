"""The kNN kernels on the adversarial cases of tests/knn_adversarial_cases.py, against brute force (oracle.knn.knn_batch):
indices AND squared distances bit-equal, the distances being the kernels' own (gdm_knn_job.d2, which ops.knn_jobs leaves NULL:
the launch hook below fills it in).  Every case runs in every form that can serve it:

  default  the library's ladder with the full workspace: ratio ranges + knn_grid_kernel where the organised hint is given and
           accepted, cell lists + knn_cells_kernel from 1024 points, hashed tiles + knn_wave_kernel below
  nohint   an organised support without its hint (cell lists, or tiles below 1024 points)
  tiles    a workspace with room for the hashed tiles only: knn_wave_kernel on packed tiles
  ws0      no workspace: knn_wave_kernel gathering from the [S,3] array

with K = 16 and K = 32 in one job table, and K = 1 (knn_kernel<1>) beside them in the default form.  tests/
test_knn_prune_model_cpu.py holds a float32 restatement of the two pruning rules to the same oracle on the same cases: where a
case fails here and not there, the kernel differs from its restatement."""
import numpy as np
import pytest
import torch

import knn_adversarial_cases as kc
import knn_prune_model as pm

pytestmark = pytest.mark.gpu

FORMS = ("default", "nohint", "tiles", "ws0")


@pytest.fixture(scope="module")
def ops():
    from geometric_aware_dense_matching_amd import ops as o
    return o


def _tiles_bytes(S, B):
    ntiles = (S + 1023) // 1024
    npad = 64
    while npad < (S + ntiles - 1) // ntiles:
        npad <<= 1
    return B * ntiles * npad * 16


def _cells_bytes(S, B):
    return B * S * 16 + (B * (1024 + 4 + 8) * 4 + 15) // 16 * 16


def _ranges_bytes(S, W, B):
    H = S // W
    return (B * (2 * W + 2 * H + 2 * ((H + 15) // 16)) * 4 + 15) // 16 * 16


def _full_bytes(S, W, B):
    """The workspace of ONE support searched with K > 1 (include/gdm.h): the first layout of its ladder."""
    if pm.is_grid_job(S, W, 16):
        return _ranges_bytes(S, W, B)
    return _cells_bytes(S, B) if S >= pm.KC_MIN_S else _tiles_bytes(S, B)


def run_jobs(ops, monkeypatch, jobs, B, nbytes=None, expect_full=None):
    """ops.knn_jobs with the distances switched on and a workspace of `nbytes` (None: what the library asks for).
    -> [(idx i64[B,Q,K], d2 f32[B,Q,K])] per job."""
    from geometric_aware_dense_matching_amd import _lib
    d2s = []

    def launch(arr, n, B, device):
        full = int(_lib.lib().gdm_knn_jobs_workspace_bytes(arr, n, B))
        if expect_full is not None:
            assert full == expect_full                    # the ladder gives this support the layout the test is about
        for i in range(n):
            d2 = torch.full((B, arr[i].Q, arr[i].K), float("nan"), dtype=torch.float32, device=device)
            arr[i].d2 = d2.data_ptr()
            d2s.append(d2)
        ws = torch.empty(max(full, 16), dtype=torch.uint8, device=device)
        ops.call("gdm_knn_jobs_ws_hip", arr, n, B, ws, full if nbytes is None else nbytes)
        return ws

    monkeypatch.setattr(ops, "_knn_launch", launch)
    idx = ops.knn_jobs(jobs, B)
    torch.cuda.synchronize()
    return [(i.cpu().numpy().astype(np.int64), d.cpu().numpy()) for i, d in zip(idx, d2s)]


def assert_bit_equal(got, want, what):
    (gi, gd), (wi, wd) = got, want
    bad = (gi != wi).any(axis=2) | (gd.view(np.uint32) != wd.view(np.uint32)).any(axis=2)
    assert not bad.any(), "%s: %d of %d queries differ from the oracle, first (crop, query) %s" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


# "nohint" only where there is a hint to leave out
RUNS = [(n, f) for n in kc.NAMES for f in FORMS if f != "nohint" or n in kc.ORGANISED]


@pytest.mark.parametrize("name,form", RUNS)
def test_knn_adversarial_case_equals_oracle(ops, monkeypatch, name, form):
    c = kc.make(name)
    S = c.sup.shape[1]
    sup, qry = torch.from_numpy(c.sup.copy()).cuda(), torch.from_numpy(c.qry.copy()).cuda()
    W = c.W if form == "default" else 0
    Ks = (16, 32, 1) if form == "default" else (16, 32)
    jobs = [(sup, qry, K, W) if W else (sup, qry, K) for K in Ks]
    nbytes = {"default": None, "nohint": None, "tiles": _tiles_bytes(S, kc.B), "ws0": 0}[form]
    if form == "tiles":
        assert S < pm.KC_MIN_S or nbytes < _cells_bytes(S, kc.B)         # no room for the cell list
    got = run_jobs(ops, monkeypatch, jobs, kc.B, nbytes, expect_full=_full_bytes(S, W, kc.B))
    for K, g in zip(Ks, got):
        assert_bit_equal(g, kc.want(name, K), "%s %s K=%d" % (name, form, K))


def test_knn_mixed_job_table_keeps_per_job_state_apart(ops, monkeypatch):
    """One launch with a cell-list support far from the origin, an organised wall, a K = 1 job and a small tiled support: every
    entry gets its own box, ranges and tiles, and the wall is searched a second time by the far queries."""
    a, w, e, s = (kc.make(n) for n in ("offset_cube_2p16", "flat_wall", "edge_points", "sizes_1023_dups"))
    t = lambda x: torch.from_numpy(x.copy()).cuda()
    wall, far = t(w.sup), t(a.qry)                        # one tensor each: a support is shared by its address
    jobs = [(t(a.sup), far, 16), (wall, t(w.qry), 16, w.W), (t(e.sup), t(e.qry), 1), (t(s.sup), t(s.qry), 32),
            (wall, far, 16, w.W)]
    full = (_cells_bytes(a.sup.shape[1], kc.B) + _ranges_bytes(w.sup.shape[1], w.W, kc.B) + _tiles_bytes(s.sup.shape[1], kc.B))
    got = run_jobs(ops, monkeypatch, jobs, kc.B, expect_full=full)
    from oracle import knn as oknn
    wants = [kc.want(a.name, 16), kc.want(w.name, 16), kc.want(e.name, 1), kc.want(s.name, 32),
             oknn.knn_batch(w.sup, a.qry, 16, return_d2=True)]
    for i, (g, wnt) in enumerate(zip(got, wants)):
        assert_bit_equal(g, wnt, "job %d" % i)
