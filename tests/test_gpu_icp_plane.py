"""GPU: point-to-plane ICP (csrc/gdm_pose_robust.hip icp_plane_update_kernel) against the fp64 restatement
(pose.icp_plane_step_numpy / icp_plane_numpy) on the inputs of tests/icp_plane_cases.py, whose conditioning
tests/test_icp_plane_cpu.py asserts.

Per iteration the restatement takes the device's own nn / d2 (after checking that nn IS a nearest vertex), so a near tie between two
vertices cannot part the two; what is left is the fp32 query (coordinates below 1 m: a few 1e-8 m) against the restatement's fp64 one.
Bounds: pair count, status, active, iters exact; err within 1e-6 m; RT within 1e-5 (the bound of the point-to-point tests; the largest
deviations seen on the MI355X over all cases were 9.6e-10 m and 1.4e-7).  Over a free run of n iterations the
per-iteration bound is added linearly: n x 1e-5 -- a Gauss-Newton step near the optimum contracts the previous step's error rather
than amplifying it, so the sum is an upper bound."""
import json
import os

import numpy as np
import pytest
import torch

import icp_plane_cases as C
from geometric_aware_dense_matching_amd import _lib, infer, ops, pose, synthetic
from geometric_aware_dense_matching_amd._lib import check
from geometric_aware_dense_matching_amd.config import make_model_cfg

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-4


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _state(B, valid=None, err0=None):
    return dict(active=_t(np.ones(B, np.uint8) if valid is None else np.asarray(valid, np.uint8)),
                iters=torch.zeros(B, dtype=torch.int32, device="cuda"), status=torch.zeros(B, dtype=torch.int32, device="cuda"),
                err=_t(np.zeros(B) if err0 is None else np.asarray(err0, np.float64)),
                n_pairs=torch.full((B,), -1, dtype=torch.int32, device="cuda"))


def _iteration(cld, RT, st, mask, model, nrm, opt, point_major=False, min_points=6, pivot_min=1e-6):
    """The three launches of one iteration through the C ABI; RT and st are updated in place.  -> nn i32[B,N], d2 f32[B,N]."""
    B, _, N = cld.shape
    M = model.shape[0]
    if point_major:
        xyz, sn = cld[:, :3].transpose(1, 2).contiguous(), cld[:, 6:9].transpose(1, 2).contiguous()
        xyz_p, sn_p, sb, ps, cs = xyz.data_ptr(), sn.data_ptr(), 3 * N, 3, 1
    else:
        xyz_p, sn_p, sb, ps, cs = cld.data_ptr(), cld.data_ptr() + 6 * N * 4, cld.stride(0), 1, N
    query = torch.empty((B, N, 3), dtype=torch.float32, device="cuda")
    nn = torch.empty((B, N, 1), dtype=torch.int32, device="cuda")
    d2 = torch.empty((B, N, 1), dtype=torch.float32, device="cuda")
    job = (_lib.KnnJob * 1)()
    job[0].support, job[0].query, job[0].idx, job[0].d2 = model.data_ptr(), query.data_ptr(), nn.data_ptr(), d2.data_ptr()
    job[0].support_bstride, job[0].query_bstride = 0, N * 3
    job[0].S, job[0].Q, job[0].K, job[0].grid_w = M, N, 1, 0
    L = _lib.lib()
    gate = opt["normal_gate"]
    check(L.gdm_icp_transform_hip(xyz_p, sb, ps, cs, RT.data_ptr(), B, N, query.data_ptr(), ops._stream()), "transform")
    check(L.gdm_knn_jobs_ws_hip(job, 1, B, None, 0, ops._stream()), "knn")
    check(L.gdm_icp_plane_update_hip(None if gate is None else sn_p, sb, ps, cs, query.data_ptr(), model.data_ptr(), nrm.data_ptr(),
                                     nn.data_ptr(), d2.data_ptr(), mask.data_ptr(), B, N, M,
                                     -1.0 if opt["reject_dist"] is None else opt["reject_dist"], 0.0 if gate is None else gate,
                                     0.0 if opt["huber"] is None else opt["huber"], TOL, min_points, pivot_min, RT.data_ptr(),
                                     st["active"].data_ptr(), st["iters"].data_ptr(), st["err"].data_ptr(), st["status"].data_ptr(),
                                     st["n_pairs"].data_ptr(), ops._stream()), "gdm_icp_plane_update_hip")
    torch.cuda.synchronize()
    return nn[:, :, 0].cpu().numpy(), d2[:, :, 0].cpu().numpy()


def _check_one_iteration(case, start, opt_name, tag):
    """One iteration of every crop of `case` from the fp32 poses `start` on the device against the restatement fed the device's
    search.  Crops with an odd index + N start from a previous mean 5e-5 away from theirs, so that both stop outcomes occur."""
    opt = C.OPTIONS[opt_name]
    B, _, N = case["cld"].shape
    own = []
    for b in range(B):
        sc, sn = C.scene_of(case, b)
        own.append(pose.icp_plane_step_numpy(sc, sn, case["model"], case["model_nrm"], start[b], case["mask"][b], **opt))
    err0 = np.array([own[b]["mean"] + 5e-5 if (N + b) % 2 else 0.0 for b in range(B)])
    cld, RT, st = _t(case["cld"]), _t(start), _state(B, err0=err0)
    nn, d2 = _iteration(cld, RT, st, _t(case["mask"]), _t(case["model"]), _t(case["model_nrm"]), opt)
    RT = RT.cpu().numpy()
    worst = dict(err=0.0, RT=0.0, nn=0.0)
    for b in range(B):
        sc, sn = C.scene_of(case, b)
        R64, t64 = start[b][:, :3].astype(np.float64), start[b][:, 3].astype(np.float64)
        x = (sc - t64) @ R64
        sel = case["mask"][b] != 0
        gap = np.linalg.norm(x - case["model"][nn[b]].astype(np.float64), axis=1) - own[b]["dist_ref"]
        worst["nn"] = max(worst["nn"], float(gap[sel].max()))
        assert gap[sel].max() <= 1e-6                               # the device's nn is a nearest vertex
        s = pose.icp_plane_step_numpy(sc, sn, case["model"], case["model_nrm"], start[b], case["mask"][b], nn=nn[b], d2=d2[b], **opt)
        assert s["status"] == 0
        assert int(st["n_pairs"][b]) == s["n"]
        worst["err"] = max(worst["err"], abs(float(st["err"][b]) - s["mean"]))
        worst["RT"] = max(worst["RT"], float(np.abs(RT[b] - s["RT"]).max()))
        stop = abs(err0[b] - s["mean"]) < TOL
        assert (int(st["status"][b]), int(st["active"][b]), int(st["iters"][b])) == (1 if stop else 0, 0 if stop else 1, 1)
    print("%s: max |err - ref| %.2e m, max |RT - ref| %.2e, max nn gap %.2e m" % (tag, worst["err"], worst["RT"], worst["nn"]))
    assert worst["err"] <= 1e-6
    assert worst["RT"] <= 1e-5


@pytest.mark.parametrize("opt", sorted(C.OPTIONS))
@pytest.mark.parametrize("B,N,M", C.ONE_ITER_SHAPES)
def test_one_iteration_every_shape(B, N, M, opt):
    case = C.one_iteration_case(B, N, M, opt)
    _check_one_iteration(case, case["RT_start"], opt, "B=%d N=%d M=%d %s" % (B, N, M, opt))


# ---- status paths ----
def _run_frozen(case, opt, valid=None, iters=2):
    B = case["cld"].shape[0]
    RT0 = _t(case["RT0"])
    valid = torch.ones(B, dtype=torch.bool, device="cuda") if valid is None else _t(valid)
    RT, n_iter, resid, status = pose.refine_icp_plane(RT0, valid, _t(case["cld"]), _t(case["mask"]), _t(case["model"]),
                                                      _t(case["model_nrm"]), iters=iters, tolerance=TOL, **opt)
    return RT0, RT, n_iter.cpu().numpy(), status.cpu().numpy()


def test_starved_crops_stop_unchanged():
    case = C.make_case("ellipsoid", 512, 257, [4, 5])
    case["mask"][0] = 0
    case["mask"][0, [3, 40, 77, 150, 256]] = [1, 2, 255, 1, 1]      # 5 selected points
    keep = [5, 60, 61, 200, 255]                                   # crop 1: the gate rejects all but 5 (the others' normals turned away: cosine < 0)
    flip = np.setdiff1d(np.arange(257), keep)
    case["cld"][1, 6:9, flip] *= -1.0
    RT0, RT, n_iter, status = _run_frozen(case, dict(normal_gate=0.0))
    assert status.tolist() == [2, 2] and n_iter.tolist() == [0, 0]
    assert torch.equal(RT, RT0)
    # six points are enough: the same crop with one more runs
    case["mask"][0, 100] = 1
    _, RT, n_iter, status = _run_frozen(case, dict(normal_gate=0.0), iters=1)
    assert status[0] != 2 and status[1] == 2


@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_degenerate_models_are_frozen_and_flagged(kind):
    case = C.make_case(kind, 512, 257, [1, 2, 3])
    RT0, RT, n_iter, status = _run_frozen(case, {})
    assert status.tolist() == [3, 3, 3] and n_iter.tolist() == [0, 0, 0]
    assert torch.equal(RT, RT0)


def test_invalid_crops_are_untouched_and_converged_crops_stay_frozen():
    case = C.make_case("ellipsoid", 512, 257, list(C.WHOLE_RUN_SEEDS))
    RT0, RT, n_iter, status = _run_frozen(case, C.OPTIONS["all"], valid=np.array([True, False, True]), iters=10)
    assert n_iter[1] == 0 and status[1] == 0 and torch.equal(RT[1], RT0[1])
    assert status[0] == 1 and status[2] == 1 and max(n_iter) < 7
    _, RT7, n7, s7 = _run_frozen(case, C.OPTIONS["all"], valid=np.array([True, False, True]), iters=7)
    assert torch.equal(RT7, RT) and n7.tolist() == n_iter.tolist() and s7.tolist() == status.tolist()


# ---- whole run ----
def _device_add(RT, case):
    return [C.add_error(RT[b].double().cpu().numpy(), case["RT_gt"][b], case["model"]) for b in range(RT.shape[0])]


def test_whole_run_against_the_free_running_restatement():
    case = C.make_case("ellipsoid", 512, 257, list(C.WHOLE_RUN_SEEDS))
    opt = C.OPTIONS["all"]
    B = 3
    valid = torch.ones(B, dtype=torch.bool, device="cuda")
    cld, mask, model, nrm, RT0 = (_t(case[k]) for k in ("cld", "mask", "model", "model_nrm", "RT0"))
    RT, n_iter, resid, status = pose.refine_icp_plane(RT0, valid, cld, mask, model, nrm, iters=10, tolerance=TOL, **opt)
    RTp, _, _ = pose.refine_icp(RT0, valid, cld, mask, model, iters=20, tolerance=0.0)
    add_dev, add_pt = _device_add(RT, case), _device_add(RTp, case)
    for b in range(B):
        sc, sn = C.scene_of(case, b)
        ref = pose.icp_plane_numpy(sc, sn, case["model"], case["model_nrm"], case["RT0"][b], iters=10, tolerance=TOL, **opt)
        assert (int(n_iter[b]), int(status[b])) == (ref["iters"], ref["status"])
        allow = ref["iters"] * 1e-5                                 # the per-iteration bound, added linearly over the iterations run
        dev = float(np.abs(RT[b].cpu().numpy() - ref["RT"]).max())
        add_ref = C.add_error(ref["RT"], case["RT_gt"][b], case["model"])
        print("crop %d: %d iterations, |RT - ref| %.2e, |resid - ref| %.2e, ADD device %.3e ref %.3e point x20 %.3e m"
              % (b, ref["iters"], dev, abs(float(resid[b]) - ref["resid"]), add_dev[b], add_ref, add_pt[b]))
        assert dev <= allow
        assert add_dev[b] <= add_ref + allow
        assert add_dev[b] < 0.5 * add_pt[b]


# ---- the product shape, once ----
def test_product_shape():
    case = C.make_case("ellipsoid", 8192, 2048, list(C.PRODUCT_SEEDS))
    _check_one_iteration(case, case["RT0"], "all", "B=16 N=2048 M=8192 all")
    B = 16
    valid = torch.ones(B, dtype=torch.bool, device="cuda")
    cld, mask, model, nrm, RT0 = (_t(case[k]) for k in ("cld", "mask", "model", "model_nrm", "RT0"))
    RT, n_iter, _, status = pose.refine_icp_plane(RT0, valid, cld, mask, model, nrm, iters=5, tolerance=0.0)
    RTp, _, _ = pose.refine_icp(RT0, valid, cld, mask, model, iters=20, tolerance=0.0)
    assert n_iter.tolist() == [5] * B and status.tolist() == [0] * B
    a_pl, a_pt = _device_add(RT, case), _device_add(RTp, case)
    print("ADD plane x5 / point x20:", " ".join("%.3f" % (p / q) for p, q in zip(a_pl, a_pt)))
    assert all(p < 0.5 * q for p, q in zip(a_pl, a_pt))


# ---- layouts and plumbing ----
def test_point_major_scene_equals_channel_major():
    case = C.make_case("ellipsoid", 512, 257, [4, 5, 6])
    case["mask"][1] = C.partial_mask(257, 9)
    outs = []
    for pm in (False, True):
        RT, st = _t(case["RT0"]), _state(3)
        _iteration(_t(case["cld"]), RT, st, _t(case["mask"]), _t(case["model"]), _t(case["model_nrm"]), C.OPTIONS["all"], point_major=pm)
        outs.append((RT, st))
    assert torch.equal(outs[0][0], outs[1][0])
    assert all(torch.equal(outs[0][1][k], outs[1][1][k]) for k in outs[0][1])
    assert not torch.equal(outs[0][0], _t(case["RT0"]))


def _fit_inputs():
    """A case with matching output: best_idx = the nearest vertex under the planted pose, so that the Kabsch fit is a rough start."""
    case = C.make_case("ellipsoid", 512, 257, [4, 5, 6])
    idx = np.zeros((3, 257), np.int32)
    for b in range(3):
        sc, _ = C.scene_of(case, b)
        x = (sc - case["RT_gt"][b][:, 3]) @ case["RT_gt"][b][:, :3]
        idx[b] = pose._nearest_two(x, case["model"].astype(np.float64))[0]
    res = dict(mask=_t(case["mask"]), best_idx=_t(idx))
    return case, res, _t(case["cld"]), _t(case["model"]), _t(case["model_nrm"])


PLANE_OPTS = dict(icp_metric="plane", icp_huber=C.HUBER, icp_normal_gate=C.GATE, icp_reject_dist=C.REJECT)


def test_estimate_poses_plane_equals_refine_icp_plane():
    case, res, cld, model, nrm = _fit_inputs()
    out = pose.estimate_poses(res, cld, model, icp_iters=4, pose_opts=PLANE_OPTS, model_nrm=nrm)
    assert {"RT", "valid", "icp_iters", "icp_resid", "icp_status"} <= set(out)
    RT0, valid = pose.solve_poses(res, cld, model)
    RT, n_iter, resid, status = pose.refine_icp_plane(RT0, valid, cld, res["mask"], model, nrm, iters=4, tolerance=1e-4,
                                                      reject_dist=C.REJECT, normal_gate=C.GATE, huber=C.HUBER, min_points=5)
    assert torch.equal(out["RT"], RT) and torch.equal(out["icp_iters"], n_iter) and torch.equal(out["icp_status"], status)
    assert torch.equal(out["icp_resid"], resid) and int(n_iter.min()) >= 1
    with pytest.raises(ValueError, match="model_nrm"):
        pose.estimate_poses(res, cld, model, icp_iters=4, pose_opts=PLANE_OPTS)


def test_defaults_and_point_metric_are_refine_icp_bit_for_bit():
    case, res, cld, model, nrm = _fit_inputs()
    RT0, valid = pose.solve_poses(res, cld, model)
    RT, n_iter, resid = pose.refine_icp(RT0, valid, cld, res["mask"], model, 3, 0.001, None, 5)
    for kw in (dict(), dict(pose_opts=dict(icp_metric="point")), dict(pose_opts=dict(icp_metric="point"), model_nrm=nrm)):
        out = pose.estimate_poses(res, cld, model, icp_iters=3, **kw)
        assert set(out) == {"RT", "valid", "icp_iters", "icp_resid"}
        assert torch.equal(out["RT"], RT) and torch.equal(out["icp_iters"], n_iter) and torch.equal(out["icp_resid"], resid)


@pytest.fixture(scope="module")
def small_model():
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    M = 512
    model = GeoMatch(make_model_cfg(n_mesh_node=M), 1, model_points=synthetic.make_model_points(1, M))
    keys = json.load(open(os.path.join(G, "geomatch_state.json")))
    sd = synthetic.synthetic_state_dict({k: torch.zeros(v) for k, v in keys.items()}, seed=0)
    model.load_state_dict(sd, strict=False)
    return model.cuda().eval()


def test_pipeline_step_returns_icp_status(small_model):
    b = synthetic.make_batch(seed=81, batch=2, n_points=1024)
    batch = {k: torch.from_numpy(b[k]).cuda() for k in ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")}
    with torch.no_grad():
        out = infer.pipeline_step(small_model, batch, with_pose=True, icp_iters=4, pose_opts=dict(icp_metric="plane", icp_huber=0.005))
        again = infer.pipeline_step(small_model, batch, with_pose=True, icp_iters=4, pose_opts=dict(icp_metric="plane", icp_huber=0.005))
    assert out["icp_status"].shape == (2,) and out["icp_status"].dtype == torch.int32
    assert set(out["icp_status"].tolist()) <= {0, 1, 2, 3}
    n = small_model.model_emb.unit_normals()
    assert n is small_model.model_emb.unit_normals()               # normalised once per model
    assert torch.allclose(n.norm(dim=1), torch.ones_like(n[:, 0]), atol=1e-6)
    ok, bad = infer.outputs_equal(out, again)
    assert ok, bad


# ---- capture ----
def test_plane_metric_captures_and_is_deterministic():
    case, res, cld, model, nrm = _fit_inputs()

    def run():
        return pose.estimate_poses(res, cld, model, icp_iters=6, pose_opts=PLANE_OPTS, model_nrm=nrm)
    e1, e2 = run(), run()
    assert all(torch.equal(e1[k], e2[k]) for k in e1)              # fixed reduction order
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(out[k], e1[k]) for k in e1)
    assert int(e1["icp_iters"].min()) >= 2
