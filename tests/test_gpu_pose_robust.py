"""GPU: the robust pose fits (csrc/gdm_pose_robust.hip) -- RANSAC and ICP against golden vectors made by the real reference
(tests/golden/make_golden_pose_robust.py), robustness to outliers, ICP on a partial view, bit-determinism eager / hipGraph, and the
pipeline / command-line entry points."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, G)

from geometric_aware_dense_matching_amd import infer, pose, synthetic  # noqa: E402
from geometric_aware_dense_matching_amd.config import make_model_cfg  # noqa: E402

SENTINEL = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -1000]], np.float32)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(G, "pose_robust.npz")))


def _res(mask, idx):
    return dict(mask=torch.from_numpy(mask).cuda(), best_idx=torch.from_numpy(idx).cuda())


def test_ransac_matches_reference_golden(gold):
    res = _res(gold["r_mask"], gold["r_idx"])
    cld = torch.from_numpy(gold["r_cld"]).cuda()
    model = torch.from_numpy(gold["r_model"]).cuda()
    RT, valid, counts, winner = pose.ransac_poses(res, cld, model, int(gold["H"]), float(gold["match_err"]), float(gold["fix_percent"]),
                                                  int(gold["seed"]))
    RT, valid, counts, winner = RT.cpu().numpy(), valid.cpu().numpy(), counts.cpu().numpy(), winner.cpu().numpy()
    assert np.array_equal(winner, gold["r_winner"])
    assert np.array_equal(valid.astype(np.uint8), gold["r_valid"])
    live = gold["r_mask"].sum(1) >= 5
    d = np.abs(counts - gold["r_counts"])[live]
    assert (d <= gold["r_near"][live]).all(), (counts, gold["r_counts"])
    for b in range(RT.shape[0]):
        if gold["r_valid"][b]:
            assert np.abs(RT[b] - gold["r_RT"][b]).max() < 1e-5, b
        else:
            assert np.array_equal(RT[b], SENTINEL), b             # incl. the zero-inlier crop (the reference's zeros)
    # the crop that exited at hypothesis 0 refit the inliers of the plain Kabsch fit; that fit itself is solve_poses' answer
    RTk, vk = pose.solve_poses(res, cld, model)
    assert np.array_equal(vk.cpu().numpy(), live)
    RT1, v1, c1, w1 = pose.ransac_poses(res, cld, model, 1, float(gold["match_err"]), 1.0)
    one = np.where((c1[:, 0] > 0).cpu().numpy() & live)[0]
    assert len(one) >= 2 and torch.equal(RT1[one], RTk[one]) and (w1[one] == 0).all()


def _outlier_case(frac, seed=5, B=4, N=1500, M=600):
    rs = np.random.RandomState(seed)
    model = ((rs.rand(M, 3) - 0.5) * 0.2).astype(np.float32)
    idx = rs.randint(0, M, size=(B, N)).astype(np.int32)
    mask = np.ones((B, N), np.uint8)
    cld = np.zeros((B, 9, N), np.float32)
    RT = np.zeros((B, 3, 4), np.float32)
    for b in range(B):
        q, _ = np.linalg.qr(rs.randn(3, 3))
        q *= np.sign(np.linalg.det(q))
        t = np.array([0.05 * b, -0.02, 0.9])
        RT[b, :, :3], RT[b, :, 3] = q, t
        pts = model[idx[b]] @ q.T + t + 0.001 * rs.randn(N, 3)
        out = rs.rand(N) < frac
        pts[out] = t + np.array([0.3, 0.3, 0.0]) + (rs.rand(int(out.sum()), 3) - 0.5) * 0.3     # a background cluster beside it
        cld[b, :3] = pts.T
    return model, idx, mask, cld, RT


@pytest.mark.parametrize("frac", [0.4, 0.5])
def test_ransac_survives_outliers_kabsch_does_not(frac):
    model, idx, mask, cld, RT = _outlier_case(frac)
    res = _res(mask, idx)
    m, c, gt = torch.from_numpy(model).cuda(), torch.from_numpy(cld).cuda(), torch.from_numpy(RT).cuda()
    diam = float(torch.cdist(m, m).max())
    RTk, vk = pose.solve_poses(res, c, m)
    RTr, vr = pose.solve_poses(res, c, m, method="ransac", ransac_iters=256, fix_percent=0.45)
    add_k, add_r = pose.add_metric(RTk, gt, m), pose.add_metric(RTr, gt, m)
    assert bool(vk.all()) and bool(vr.all())
    assert bool((add_k > 0.10 * diam).all()), add_k
    assert bool((add_r < 0.01 * diam).all()), add_r


def test_icp_matches_reference_golden(gold):
    B, _, N = gold["i_cld"].shape
    cld = torch.from_numpy(gold["i_cld"]).cuda()
    model = torch.from_numpy(gold["i_model"]).cuda()
    RT0 = torch.from_numpy(gold["i_RT0"]).cuda()
    valid = torch.ones(B, dtype=torch.bool, device="cuda")
    mask = torch.ones((B, N), dtype=torch.uint8, device="cuda")
    RT, iters, resid = pose.refine_icp(RT0, valid, cld, mask, model, int(gold["i_max_iters"]), float(gold["i_tol"]))
    assert np.array_equal(iters.cpu().numpy(), gold["i_iters"])
    assert np.abs(RT.cpu().numpy() - gold["i_RT"]).max() < 1e-5
    assert np.abs(resid.cpu().numpy() - gold["i_resid"]).max() < 1e-5
    assert torch.equal(RT0, torch.from_numpy(gold["i_RT0"]).cuda())          # the input is not modified


def _rot(axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def test_icp_partial_view_converges_and_freezes():
    rs = np.random.RandomState(11)
    M, B = 3000, 4
    model = ((rs.rand(M, 3) - 0.5) * np.array([0.15, 0.1, 0.08])).astype(np.float32)
    R = _rot([0.3, -1.0, 0.2], 40.0)
    t = np.array([0.02, -0.03, 0.8])
    posed = model @ R.T + t
    vis = np.where(posed[:, 2] < np.median(posed[:, 2]))[0]        # the half facing the camera
    N = len(vis)
    cld = np.zeros((B, 9, N), np.float32)
    RT0 = np.zeros((B, 3, 4), np.float32)
    gt = np.zeros((B, 3, 4), np.float32)
    for b in range(B):
        cld[b, :3] = (posed[vis] + 0.001 * rs.randn(N, 3)).T
        dR = _rot(rs.randn(3), 5.0)
        dt = rs.randn(3)
        dt *= 0.01 / np.linalg.norm(dt)
        RT0[b, :, :3], RT0[b, :, 3] = dR @ R, t + dt
        gt[b, :, :3], gt[b, :, 3] = R, t
    mask = np.ones((B, N), np.uint8)
    mask[3] = 0
    mask[3, :3] = 1                                                # crop 3: fewer than min_points pairs
    valid = torch.tensor([1, 1, 0, 1], dtype=torch.bool, device="cuda")   # crop 2: invalid
    m = torch.from_numpy(model).cuda()
    RT, iters, resid = pose.refine_icp(torch.from_numpy(RT0).cuda(), valid, torch.from_numpy(cld).cuda(),
                                       torch.from_numpy(mask).cuda(), m, iters=40, tolerance=1e-6)
    add = pose.add_metric(RT, torch.from_numpy(gt).cuda(), m).cpu()
    add0 = pose.add_metric(torch.from_numpy(RT0).cuda(), torch.from_numpy(gt).cuda(), m).cpu()
    assert bool((add[:2] < 0.002).all()), (add, add0)
    assert bool((add0[:2] > 0.005).all())
    it = iters.cpu().tolist()
    assert it[0] >= 2 and it[1] >= 2 and it[2] == 0 and it[3] == 0
    assert torch.equal(RT[2:], torch.from_numpy(RT0[2:]).cuda())  # frozen crops are left as they came
    assert bool(torch.isfinite(resid).all()) and float(resid[0]) < 0.003


@pytest.fixture(scope="module")
def small_model():
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    M = 512
    model = GeoMatch(make_model_cfg(n_mesh_node=M), 1, model_points=synthetic.make_model_points(1, M))
    keys = json.load(open(os.path.join(G, "geomatch_state.json")))
    sd = synthetic.synthetic_state_dict({k: torch.zeros(v) for k, v in keys.items()}, seed=0)
    model.load_state_dict(sd, strict=False)
    return model.cuda().eval()


def _batch(seed, B=2, N=1024):
    b = synthetic.make_batch(seed=seed, batch=B, n_points=N)
    return {k: torch.from_numpy(b[k]).cuda() for k in ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")}


ROBUST = dict(pose_fit="ransac", icp_iters=3)


def test_pipeline_robust_pose_is_deterministic_and_captures(small_model):
    b0, b1 = _batch(81), _batch(82)
    with torch.no_grad():
        e1 = infer.pipeline_step(small_model, b0, with_pose=True, **ROBUST)
        e2 = infer.pipeline_step(small_model, b0, with_pose=True, **ROBUST)
        ok, bad = infer.outputs_equal(e1, e2)
        assert ok, bad
        assert {"RT", "valid", "icp_iters", "icp_resid"} <= set(e1)
        # the defaults are today's step, bit for bit
        plain = infer.pipeline_step(small_model, b0, with_pose=True)
        same = infer.pipeline_step(small_model, b0, with_pose=True, pose_fit="kabsch", icp_iters=0)
        assert set(plain) == set(same)
        ok, bad = infer.outputs_equal(plain, same)
        assert ok, bad
        gp = infer.GraphedPipeline(small_model, b0, with_pose=True, **ROBUST)
        assert gp.check and all(c.get("bit_identical") for c in gp.check.values()), gp.check
        got = {k: v.clone() for k, v in gp(b1).items()}
        want = infer.pipeline_step(small_model, b1, with_pose=True, **ROBUST)
    ok, bad = infer.outputs_equal(want, got)
    assert ok, bad


def _check_poses(RT, valid):
    assert bool(torch.isfinite(RT).all())
    for i in torch.nonzero(valid.bool()).flatten().tolist():
        R = RT[i, :, :3].double()
        assert torch.allclose(R @ R.T, torch.eye(3, dtype=torch.float64, device=R.device), atol=1e-5)


def test_run_multi_object_and_test_entry_point_with_robust_pose(small_model):
    out = infer.run_multi_object({1: small_model}, _batch(83, B=3), [1, 1, 1], pose_fit="ransac", icp_iters=2)
    assert out["RT"].shape == (3, 3, 4) and out["icp_iters"].shape == (3,)
    _check_poses(out["RT"], out["valid"])
    from geometric_aware_dense_matching_amd import train_lm
    argv = ("--gpus=0 -state=test -cls_id=1 --single-object --batch-size 2 --n-points 1024 --n-mesh 512 --synthetic-items 4 "
            "--pose-fit ransac --icp-iters 2").split()
    train_lm.main(argv)
    res = train_lm.test(train_lm.build_parser().parse_args(argv))
    assert len(res) == 2
    for r in res:
        _check_poses(r["RT"], r["valid"])
