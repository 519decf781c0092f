"""CPU: THE DEPTH REFINEMENT RULE of include/gdm.h as pose.refine_poses_depth_numpy restates it -- the increment
against a least-squares solve, recovery of a planted offset, occlusion, the gate's exact edges, the status paths, and the conditions
every scene of tests/test_gpu_depth_refine.py must meet for its 1e-9 bound to be derivable.  Frames of 96 x 80 (one of 160 x 144)."""
import numpy as np
import pytest

import depth_refine_cases as dc
from geometric_aware_dense_matching_amd import pose


def _sums(p, rt, depth=None, **kw):
    return pose.refine_depth_sums_numpy(p["verts"], p["faces"], rt, p["depth"] if depth is None else depth, p["K"], kw.pop("window", None),
                                        p["reject"], near=p["near"], **kw)


@pytest.mark.parametrize("huber", [None, 0.002])
def test_increment_equals_least_squares(huber):
    """One iteration's increment against np.linalg.lstsq on the stacked rows sqrt(w) J, sqrt(w) r, in the scaled unknowns (rotation
    columns divided by the root of the weighted mean |x|^2, as the solve scales them), to 1e-12."""
    p = dc.planted(2, "clean")
    s = _sums(p, p["start"], huber=huber, terms=True)
    assert s["pairs"] >= 200 and (huber is None or (s["w"] < 1).sum() > 20)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s["sums"][:21]
    A = A + np.triu(A, 1).T
    sol = pose.icp_plane_solve_numpy(A, s["sums"][21:27], s["sums"][27], s["sums"][28], p["start"][:, :3], p["start"][:, 3])
    assert not sol["degenerate"] and sol["min_pivot"] > 1e-3
    sc = 1.0 / np.sqrt(s["sums"][28] / s["sums"][27])
    D = np.array([sc, sc, sc, 1.0, 1.0, 1.0])
    rw = np.sqrt(s["w"])
    want = np.linalg.lstsq(rw[:, None] * s["J"] * D[None], -rw * s["r"], rcond=None)[0]
    got = sol["xi"] / D
    print("scaled increment %s, largest deviation from lstsq %.2e" % (got, np.abs(got - want).max()))
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("level,scene,bound", dc.PLANTED)
def test_a_planted_offset_is_recovered(level, scene, bound):
    p = dc.planted(level, scene)
    out = pose.refine_poses_depth_numpy(p["verts"], p["faces"], p["start"][None, None], p["depth"], p["K"], iters=3, reject=p["reject"],
                                        near=p["near"], trace=True)
    ratio = dc.add_error(p["verts"], out["RT"][0, 0], p["true"]) / p["add0"]
    tr = out["trace"][0][0]
    print("level %d %s: ADD %.3e -> ratio %.2e, pairs %s, smallest pivot %.1e" % (level, scene, p["add0"], ratio, [t["pairs"] for t in tr],
                                                                                 min(t["min_pivot"] for t in tr)))
    assert out["status"][0, 0] == 0 and out["iters"][0, 0] == 3
    assert 4e-3 < p["add0"] < 7e-3 and ratio <= bound


def test_occlusion_does_not_pull():
    """The sums of iteration 1 on the occluded frame equal, bit for bit, those on the same frame with the occluded pixels set to 0:
    what stands in front of the model is FRONT for verification and nothing here."""
    for level in (2, 3):
        p = dc.planted(level, "occluded")
        blanked = np.where(p["depth"] == np.float32(0.3), np.float32(0.0), p["depth"])
        assert (blanked == 0).sum() > 1000
        a, b = _sums(p, p["start"]), _sums(p, p["start"], depth=blanked)
        assert a["pairs"] == b["pairs"] >= 200 and a["sums"].tobytes() == b["sums"].tobytes()
        clean = _sums(dc.planted(level, "clean"), p["start"])
        assert clean["pairs"] > a["pairs"]                                 # the occluder did hide drawn pixels


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gate_edges(dtype):
    """A fronto-parallel triangle that renders exactly 1.0f against columns of 1, 1 + r, the next float above, 1 - r, the next below,
    0, -1 and NaN: the first, second and fourth pair, nothing else does."""
    e = dc.edge_case(dtype)
    s = _sums(e, e["RT"][0, 0], terms=True)
    z, f = pose.raster_depth_face_numpy(e["verts"], e["faces"], e["RT"][0, 0], e["K"], dc.H, dc.W, e["near"])
    assert set(np.unique(z[f >= 0]).tolist()) == {1.0}
    paired = np.zeros((dc.H, dc.W), dtype=bool)
    paired[s["uv"][:, 1], s["uv"][:, 0]] = True
    want = (f >= 0) & dc.EDGE_PAIRS[np.arange(dc.W) % 8][None, :]
    assert np.array_equal(paired, want) and s["pairs"] == want.sum() > 500
    for k in range(8):
        assert ((f >= 0)[:, k::8]).sum() > 50                             # every edge value is met by drawn pixels


def _same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_status_paths_leave_the_pose_alone():
    p = dc.planted(2, "clean")
    run = lambda RT, **kw: pose.refine_poses_depth_numpy(p["verts"], p["faces"], RT, p["depth"], p["K"], iters=3, reject=p["reject"],
                                                         near=p["near"], **kw)
    start = p["start"][None, None]
    # 2: a window of 2 x 2 pixels; a pose behind `near`; a NaN pose
    out = run(start, window=np.array([[47, 39, 48, 40]], dtype=np.int32))
    assert out["status"].tolist() == [[2]] and out["pairs"][0, 0] <= 4 and out["iters"][0, 0] == 0 and _same_bits(out["RT"], start)
    behind = start.copy()
    behind[0, 0, 2, 3] = 0.01
    nan = start.copy()
    nan[0, 0, 1, 1] = np.nan
    for RT in (behind, nan):
        out = run(RT)
        assert out["status"].tolist() == [[2]] and out["pairs"].tolist() == [[0]] and _same_bits(out["RT"], RT)
    # 4: an invalid candidate beside a valid one
    two = np.concatenate([start, start], axis=1)
    out = run(two, cand_valid=np.array([[False, True]]))
    assert out["status"].tolist() == [[4, 0]] and out["iters"].tolist() == [[0, 3]] and _same_bits(out["RT"][0, 0], start[0, 0])
    assert not _same_bits(out["RT"][0, 1], start[0, 0])
    # 3: a single fronto-parallel triangle -- the rotation about z is unobservable and the third pivot is exactly 0
    f = dc.flat_case()
    out = pose.refine_poses_depth_numpy(f["verts"], f["faces"], f["RT"], f["depth"], f["K"], iters=3, reject=f["reject"], near=f["near"],
                                        trace=True)
    assert out["status"].tolist() == [[3]] and out["iters"].tolist() == [[0]] and out["pairs"][0, 0] > 500 and _same_bits(out["RT"], f["RT"])
    assert out["trace"][0][0][0]["min_pivot"] == 0.0


def _accuracy_conditions(what, verts, faces, RT, depth, K, kw, answer):
    """The conditions under which the 1e-9 bound of the GPU comparison is derived, for one iteration from the poses RT."""
    n, C = RT.shape[:2]
    depth = np.broadcast_to(depth, (n,) + depth.shape[-2:])
    K = np.broadcast_to(K, (n, 3, 3))
    worst = dict(pivot=np.inf, huber=np.inf, cos=np.inf, stop=np.inf, pairs=10 ** 9)
    for i in range(n):
        for c in range(C):
            tr = answer["trace"][i][c]
            if not tr or tr[0]["mean"] is None:                            # invalid on entry, starved or degenerate: a status case
                assert answer["status"][i, c] in (2, 3, 4)
                continue
            win = None if kw["window"] is None else kw["window"][i]
            s = pose.refine_depth_sums_numpy(verts, faces, RT[i, c], depth[i], K[i], win, kw["reject"], kw["huber"], kw["min_cos"],
                                             kw["near"], terms=True)
            assert s["pairs"] == tr[0]["pairs"]
            worst["pairs"] = min(worst["pairs"], s["pairs"])
            worst["pivot"] = min(worst["pivot"], tr[0]["min_pivot"])
            if kw["huber"]:
                worst["huber"] = min(worst["huber"], np.abs(s["huber_margin"]).min())
            if kw["min_cos"] > 0:
                worst["cos"] = min(worst["cos"], np.abs(s["cos_margin"]).min())
            if kw["tolerance"] > 0:                                        # (with tolerance 0 the comparison |.| < 0 is false for every value)
                worst["stop"] = min(worst["stop"], tr[0]["stop_margin"])
    print("%s: %s" % (what, ", ".join("%s %.2e" % kv for kv in worst.items())))
    assert worst["pivot"] >= 1e-3 and worst["huber"] >= 1e-9 and worst["cos"] >= 1e-9 and worst["stop"] >= 1e-6 and worst["pairs"] >= 200
    return worst


@pytest.mark.parametrize("name", dc.SWEEP)
def test_conditions_of_the_one_iteration_cases(name):
    args, kw = dc.call_args(dc.sweep_case(name))
    starts, answers = dc.sweep_starts(name)
    active = 0
    for k in range(3):
        _accuracy_conditions("%s, start %d" % (name, k), args[0], args[1], starts[k], args[3], args[4], kw, answers[k])
        active += int((answers[k]["status"] == 0).sum())
    assert active >= 3                                                     # the case is not made of status paths alone


@pytest.mark.parametrize("name", dc.FREE + ("converged",))
def test_conditions_of_the_free_runs(name):
    """Every iteration of the 4-iteration free runs and of the converged case meets the same conditions."""
    case, iters = (dc.converged_case()[0], 6) if name == "converged" else (dc.free_case(name), 4)
    args, kw = dc.call_args(case)
    out = pose.refine_poses_depth_numpy(*args, iters=iters, trace=True, **kw)
    for i, row in enumerate(out["trace"]):
        for c, tr in enumerate(row):
            assert all(t["min_pivot"] >= 1e-3 and t["pairs"] >= 200 for t in tr)
            if kw["tolerance"] > 0:
                assert all(t["stop_margin"] >= 1e-6 for t in tr)
    if name == "converged":
        assert out["status"].tolist() == [[1, 1]] and out["iters"][0, 0] == dc.converged_case()[1] and out["iters"][0, 1] < 6
    else:
        assert out["status"].tolist() == [[0, 0]] and out["iters"].tolist() == [[4, 4]]


def test_perturbation_bound_of_the_free_run():
    """The free run started from the case's pose with every entry moved by up to 1e-12, 20 seeded draws: the largest movement d of a
    final pose entry.  The GPU free run is held to 10 max(d, 1e-9); d is recorded in depth_refine_cases' docstring and DESIGN.md 6r
    (measured 2.6e-12)."""
    d = 0.0
    for name in dc.FREE:
        args, kw = dc.call_args(dc.free_case(name))
        base = dc.free_run(name)["RT"]
        rs = np.random.RandomState(5)
        for _ in range(20):
            RT = args[2] + (rs.rand(*args[2].shape) * 2 - 1) * 1e-12
            out = pose.refine_poses_depth_numpy(args[0], args[1], RT, args[3], args[4], iters=4, **kw)
            d = max(d, float(np.abs(out["RT"] - base).max()))
    print("largest movement of a final pose entry under 1e-12 perturbations of the start: d = %.2e" % d)
    assert d < 1e-9                                                        # no snapped pixel flipped: the bound is the 1e-9 floor


def test_workspace_planner_and_host_side_refusals(monkeypatch):
    """One row of 32 doubles per tile a window can have; 0 for shapes the entry refuses; a limit is refused with its name before any
    HIP call (so this needs no GPU)."""
    monkeypatch.setattr(pose._lib, "_stream", lambda: None)
    plan = lambda *a: pose.call("gdm_pose_refine_depth_workspace_bytes", *a)
    assert plan(4, 8, 480, 640) == 4 * 8 * 10 * 8 * 32 * 8 and plan(1, 1, 64, 64) == 256 and plan(1, 1, 65, 64) == 512
    assert plan(0, 1, 80, 96) == 0 and plan(1, 1, 0, 96) == 0 and plan(1, 1, 16385, 16) == 0 and plan(65535, 65535, 64, 64) == 0
    import ctypes
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    ok = [p, 0, p, p, p, 0, p, 0, None, None, 1, 1, 3, 1, 64, 64, 0.05, 1, 0.01, 0.0, 0.0, 16, 0.0, 1e-6, p, 4096, p, p, p, p, p]
    for pos, bad, msg in ((17, 0, "iters"), (17, 65, "iters"), (18, 0.0, "reject"), (18, 1e39, "reject"), (19, -1.0, "huber"),
                          (20, 1.0, "min_cos"), (22, -1.0, "tolerance"), (23, 0.0, "pivot_min"), (25, 255, "workspace_bytes")):
        args = list(ok)
        args[pos] = bad
        with pytest.raises(pose._lib.GdmError, match=msg):
            pose._lib.call("gdm_pose_refine_depth_hip", *args)
