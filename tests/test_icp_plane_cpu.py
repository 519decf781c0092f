"""CPU: point-to-plane ICP -- the fp64 restatement (pose.icp_plane_step_numpy / icp_plane_numpy) against numpy's least
squares, the solve fragment (csrc/gdm_icp_plane_solve.inc) compiled for the host as a stand-alone program (plain and under
AddressSanitizer + UBSan) against the restatement, the accuracy claim against point-to-point ICP, and the conditions that the inputs
of tests/test_gpu_icp_plane.py must meet for its bounds to mean anything."""
import os
import subprocess

import numpy as np
import pytest

import icp_plane_cases as C
from geometric_aware_dense_matching_amd import pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "icp_plane_solve_host.cpp")


def _noise_free(M=512, N=300, seed=3):
    """Scene points on the model's vertex planes exactly (a vertex plus a tangential offset), so that at the planted pose r = 0."""
    rs = np.random.RandomState(seed)
    xyz, nrm = C.model_of("ellipsoid", M)
    xyz, nrm = xyz.astype(np.float64), nrm.astype(np.float64)
    j = rs.randint(0, M, N)
    tang = np.cross(nrm[j], rs.randn(N, 3))
    pts = xyz[j] + 0.0005 * C.unit(tang)                       # 0.5 mm off the vertex, in its tangent plane: still its nearest
    R, t = C.rand_rot(rs), np.array([0.02, -0.03, 0.7])
    return xyz, nrm, pts, j, R, t


def test_step_is_the_weighted_least_squares_solution():
    """The increment of the restatement equals np.linalg.lstsq on the stacked rows sqrt(w) J, -sqrt(w) r, to 1e-12 relative, with
    and without the options."""
    case = C.make_case("ellipsoid", 512, 257, [1, 2, 3])
    for b in range(3):
        sc, sn = C.scene_of(case, b)
        for opt in C.OPTIONS.values():
            s = pose.icp_plane_step_numpy(sc, sn, case["model"], case["model_nrm"], case["RT0"][b], **opt)
            assert s["status"] == 0
            ref = np.linalg.lstsq(s["rows"], -s["rhs"], rcond=None)[0]
            assert np.abs(s["xi"] - ref).max() <= 1e-12 * np.abs(ref).max()


def test_step_recovers_a_planted_offset_to_first_order():
    xyz, nrm, pts, j, R, t = _noise_free()
    scene = pts @ R.T + t
    dR = C.axis_angle([0.3, -0.5, 0.8], np.deg2rad(1.0))
    RT0 = np.concatenate([dR @ R, (t + 0.001 * C.unit(np.array([1.0, 2.0, -1.0])))[:, None]], axis=1)
    gt = np.concatenate([R, t[:, None]], axis=1)
    s = pose.icp_plane_step_numpy(scene, None, xyz, nrm, RT0, nn=j, d2=np.zeros(len(j), np.float32))
    assert s["status"] == 0
    before, after = C.add_error(RT0, gt, xyz), C.add_error(s["RT"], gt, xyz)
    # one Gauss-Newton step on a zero-residual problem is quadratically convergent: the remaining error is second order in the
    # offset (1 degree = 1.7e-2 rad: 1.7e-2 ** 2 of the 10 cm object is 3e-5 m)
    assert before > 5e-4 and after < 3e-5, (before, after)
    s2 = pose.icp_plane_step_numpy(scene, None, xyz, nrm, s["RT"], nn=j, d2=np.zeros(len(j), np.float32))
    assert C.add_error(s2["RT"], gt, xyz) < 1e-8


def test_huber_and_gate_act_on_exactly_the_planted_outliers():
    xyz, nrm, pts, j, R, t = _noise_free()
    N = len(pts)
    rs = np.random.RandomState(5)
    out_h = rs.choice(N, 20, replace=False)                     # moved 1 cm along the normal: |r| = 1 cm, ten times the Huber threshold
    pts = pts.copy()
    pts[out_h] += 0.01 * nrm[j[out_h]]
    scene, RT = pts @ R.T + t, np.concatenate([R, t[:, None]], axis=1)
    snrm = nrm[j] @ R.T
    out_g = np.setdiff1d(np.arange(N), out_h)[:15]              # normals turned away: cosine -1
    snrm[out_g] *= -1.0
    d2 = np.zeros(N, np.float32)
    s = pose.icp_plane_step_numpy(scene, snrm, xyz, nrm, RT, nn=j, d2=d2, normal_gate=0.5, huber=0.001)
    dropped = np.nonzero(~s["keep"])[0]
    assert np.array_equal(dropped, np.sort(out_g))
    kept = np.nonzero(s["keep"])[0]
    down = kept[s["w"] < 1.0]
    assert np.array_equal(down, np.sort(out_h))
    assert np.allclose(s["w"][s["w"] < 1.0], 0.1, rtol=1e-6)   # delta / |r| = 1 mm / 1 cm
    # without the options the outliers drag the pose; with them it stays at the planted pose to a tenth of what they did
    free = pose.icp_plane_step_numpy(scene, snrm, xyz, nrm, RT, nn=j, d2=d2)
    assert C.add_error(s["RT"], RT, xyz) < 0.2 * C.add_error(free["RT"], RT, xyz)


# ---- the solve fragment as a host program ----
@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("icp_plane_host")
    cxx = os.environ.get("CXX", "g++")
    plain, san = str(d / "solve_plain"), str(d / "solve_san")
    subprocess.check_call([cxx, "-O2", "-ffp-contract=off", "-o", plain, SRC, "-lm"])
    subprocess.check_call([cxx, "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", san, SRC, "-lm"])
    return d, plain, san


def _run(prog, d, recs):
    path = str(d / "in.bin")
    np.ascontiguousarray(recs, np.float64).tofile(path)
    p = subprocess.run([prog, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-2000:]
    return np.array([[float(v) for v in line.split()] for line in p.stdout.splitlines()]).reshape(len(recs), 32)


def _record(A, g, S, L2, R, t, pivot_min=1e-6):
    return np.concatenate([A[np.triu_indices(6)], g, [S, L2], np.concatenate([R, t[:, None]], axis=1).ravel(), [pivot_min]])


def _sums_of(kind, seed):
    """The sums the kernel would hand to the fragment for one crop of a degenerate model."""
    case = C.make_case(kind, 512, 257, [seed])
    sc, sn = C.scene_of(case, 0)
    s = pose.icp_plane_step_numpy(sc, sn, case["model"], case["model_nrm"], case["RT0"][0])
    RT = case["RT0"][0].astype(np.float64)
    x = ((sc - RT[:, 3]) @ RT[:, :3])[s["keep"]]
    J = s["rows"]
    return _record(J.T @ J, J.T @ s["rhs"], float(len(J)), float((x * x).sum()), RT[:, :3], RT[:, 3]), s


def test_solve_fragment_on_the_host(host_programs):
    d, plain, san = host_programs
    rs = np.random.RandomState(20400)
    recs, want = [], []
    for k in range(1200):                                        # well-conditioned systems: random pairs on a random ellipsoid
        n = 40 + rs.randint(0, 200)
        radii = 0.02 + 0.1 * rs.rand(3)
        u = C.unit(rs.randn(n, 3))
        x, nr = u * radii + 0.002 * rs.randn(n, 3) + 0.01 * rs.randn(3), C.unit(u / radii)
        w = rs.rand(n) + 0.1
        J = np.concatenate([np.cross(x, nr), nr], axis=1)
        r = 0.003 * rs.randn(n)
        A, g = (w[:, None] * J).T @ J, (w[:, None] * J).T @ r
        R, t = C.rand_rot(rs), rs.randn(3)
        S, L2 = w.sum(), (w * (x * x).sum(1)).sum()
        sol = pose.icp_plane_solve_numpy(A, g, S, L2, R, t)
        if sol["degenerate"] or sol["min_pivot"] < 1e-3:
            continue
        recs.append(_record(A, g, S, L2, R, t))
        D = np.array([1.0 / np.sqrt(L2 / S)] * 3 + [1.0] * 3)
        want.append((D * np.linalg.solve(A * D[:, None] * D[None, :] / S, -g * D / S), D, sol))
    assert len(recs) >= 1000
    got = _run(plain, d, np.array(recs))
    for o, (xi_ref, D, sol) in zip(got, want):
        assert o[0] == 0.0
        assert np.abs((o[2:8] - xi_ref) / D).max() <= 1e-12 * np.abs(xi_ref / D).max()     # in the scaled unknowns (all of one unit)
        assert np.abs(o[2:8] - sol["xi"]).max() <= 1e-12 * np.abs(sol["xi"]).max()
        Rn = o[8:17].reshape(3, 3)
        assert np.abs(Rn @ Rn.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Rn) - 1.0) <= 1e-12
        assert np.abs(Rn - sol["R"]).max() <= 1e-12 and np.abs(o[17:20] - sol["t"]).max() <= 1e-12 * max(1.0, np.abs(sol["t"]).max())
        assert abs(o[1] - sol["min_pivot"]) <= 1e-9 * sol["min_pivot"]
        assert np.array_equal(o[20:32].reshape(3, 4)[:, :3], Rn.astype(np.float32).astype(np.float64))
    # the same bits under the sanitizers
    assert np.array_equal(_run(san, d, np.array(recs)), got)


def test_solve_fragment_flags_degenerate_systems(host_programs):
    d, plain, san = host_programs
    recs = []
    for kind in ("plane", "sphere"):
        for seed in (1, 2):
            rec, s = _sums_of(kind, seed)
            assert s["status"] == 3 and s["min_pivot"] <= 1e-12      # the restatement agrees, and by a wide margin
            recs.append(rec)
    zero = recs[0].copy()
    zero[28] = 0.0                                              # l2 = 0
    neg = recs[0].copy()
    neg[28] = -1.0
    recs += [zero, neg]
    for prog in (plain, san):
        got = _run(prog, d, np.array(recs))
        assert np.array_equal(got[:, 0], np.ones(len(recs)))
        for o, rec in zip(got, recs):                            # the pose comes back as it went in
            assert np.array_equal(o[8:17], rec[29:41].reshape(3, 4)[:, :3].ravel()) and np.array_equal(o[17:20], rec[29:41].reshape(3, 4)[:, 3])


# ---- the claim ----
@pytest.mark.parametrize("M,N,seeds", [(512, 257, C.SEEDS_SMALL), (8192, 2048, C.SEEDS_LARGE)])
def test_five_plane_iterations_beat_twenty_point_iterations(M, N, seeds):
    """ADD to the planted pose after 5 point-to-plane iterations is below half of ADD after 20 point-to-point iterations
    (measured: 0.18 or less at M = 512, 0.05 or less at M = 8192)."""
    case = C.make_case("ellipsoid", M, N, list(seeds))
    for b in range(len(seeds)):
        sc, sn = C.scene_of(case, b)
        pl = pose.icp_plane_numpy(sc, sn, case["model"], case["model_nrm"], case["RT0"][b], iters=5, tolerance=0.0)
        assert pl["iters"] == 5
        a_pl = C.add_error(pl["RT"], case["RT_gt"][b], case["model"])
        a_pt = C.add_error(C.point_icp(sc, case["model"], case["RT0"][b], 20), case["RT_gt"][b], case["model"])
        print("M=%d seed %d: plane %.3e m, point %.3e m, ratio %.3f" % (M, seeds[b], a_pl, a_pt, a_pl / a_pt))
        assert a_pl < 0.5 * a_pt


# ---- the conditions on the GPU test's inputs ----
def _conditions(s):
    assert s["status"] == 0
    assert s["min_pivot"] >= 1e-3
    assert s["near_gate"] == 0


@pytest.mark.parametrize("opt", sorted(C.OPTIONS))
def test_input_conditions_single_iteration(opt):
    for B, N, M in C.ONE_ITER_SHAPES:
        case = C.one_iteration_case(B, N, M, opt)
        for b in range(B):
            sc, sn = C.scene_of(case, b)
            _conditions(pose.icp_plane_step_numpy(sc, sn, case["model"], case["model_nrm"], case["RT_start"][b], case["mask"][b],
                                                  **C.OPTIONS[opt]))


def test_input_conditions_whole_run():
    """The free-running case: additionally no near-tie query in any iteration and no stop comparison within 1e-6 of the tolerance."""
    case = C.make_case("ellipsoid", 512, 257, list(C.WHOLE_RUN_SEEDS))
    for b in range(len(C.WHOLE_RUN_SEEDS)):
        sc, sn = C.scene_of(case, b)
        run = pose.icp_plane_numpy(sc, sn, case["model"], case["model_nrm"], case["RT0"][b], iters=10, tolerance=1e-4,
                                   **C.OPTIONS["all"])
        assert run["status"] == 1 and 2 <= run["iters"] < 10
        assert min(run["min_pivot"]) >= 1e-3
        assert sum(run["near_gate"]) == 0 and sum(run["near_reject"]) == 0
        assert sum(run["ties"]) == 0
        assert min(run["stop_margin"]) >= 1e-6


def test_input_conditions_product_shape():
    case = C.make_case("ellipsoid", 8192, 2048, list(C.PRODUCT_SEEDS))
    for b in range(len(C.PRODUCT_SEEDS)):
        sc, sn = C.scene_of(case, b)
        _conditions(pose.icp_plane_step_numpy(sc, sn, case["model"], case["model_nrm"], case["RT0"][b], **C.OPTIONS["all"]))


def test_estimate_poses_refuses_plane_without_normals():
    with pytest.raises(ValueError, match="model_nrm"):
        pose.estimate_poses({}, None, None, icp_iters=2, pose_opts=dict(icp_metric="plane"))
    with pytest.raises(ValueError, match="icp_metric"):
        pose.estimate_poses({}, None, None, icp_iters=2, pose_opts=dict(icp_metric="surface"))


def test_command_line_options():
    from geometric_aware_dense_matching_amd import train_lm
    a = train_lm.build_parser().parse_args("-state=test -cls_id=1 --icp-iters 4 --icp-metric plane --icp-huber 0.002 --icp-normal-gate 0.5".split())
    assert (a.icp_metric, a.icp_huber, a.icp_normal_gate) == ("plane", 0.002, 0.5)
    d = train_lm.build_parser().parse_args("-state=test -cls_id=1".split())
    assert (d.icp_metric, d.icp_huber, d.icp_normal_gate) == ("point", None, None)
