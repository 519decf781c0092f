"""Batched pose solve on the GPU from the dense correspondences, and the ADD / ADI pose errors.

Mirrors, for a whole batch at once and without leaving the device:
  /root/reference/evaluator.py:60-102 cal_frame_poses  (points with seg arg-max == 1, matched vertex = arg-max column;
      fewer than 5 correspondences -> the sentinel pose [I | (0,0,-1000)])
  /root/reference/utils/pvn3d_eval_utils_kpls.py:43-77 best_fit_transform (Kabsch with the reflection fix)
  /root/reference/lib/pysixd/pose_error.py:297-337 add, adi (ADI's nearest neighbour = the HIP kNN kernel, K=1)
The reference does this on `bs` host threads with numpy (ThreadPoolExecutor, evaluator.py:294-303).
Opt-in robust variants (csrc/gdm_pose_robust.hip), also on the device and capturable in a hipGraph:
  utils/pvn3d_eval_utils_kpls.py:79-124 best_fit_transform_with_RANSAC   solve_poses(method="ransac") / ransac_poses
  utils/pvn3d_eval_utils_kpls.py:126-212 icp (point to point)              refine_icp
"""
import numpy as np
import torch

from . import _lib, ops
from ._lib import check


def kabsch_stats(res, cld_rgb_nrm, model_xyz):
    """res: matching.match_frames output; cld_rgb_nrm f32[B,9,N] (rows 0-2 = xyz); model_xyz f32[M,3] -> f64[B,16]."""
    mask, best_idx = res["mask"], res["best_idx"]
    B, N = mask.shape
    cld = ops._dev(cld_rgb_nrm, torch.float32, "cld_rgb_nrm")
    model_xyz = ops._dev(model_xyz, torch.float32, "model_xyz")
    out = torch.empty((B, 16), dtype=torch.float64, device=mask.device)
    check(_lib.lib().gdm_kabsch_stats_hip(cld.data_ptr(), cld.stride(0), 1, N, model_xyz.data_ptr(), best_idx.data_ptr(),
                                          mask.data_ptr(), B, N, model_xyz.shape[0], out.data_ptr(), ops._stream()),
          "gdm_kabsch_stats_hip")
    return out


def solve_poses(res, cld_rgb_nrm, model_xyz, min_points=5, method="kabsch", ransac_iters=20, inlier_dist=0.015, fix_percent=0.7,
                seed=0, weights="none", targets="vertex"):
    """-> RT f32[B,3,4] mapping model coordinates to the camera frame, valid bool[B].  Two launches (statistics, fit), no
    host synchronisation.  method="ransac": the reference's RANSAC (ransac_poses) with max_iter = ransac_iters hypotheses,
    match_err = inlier_dist (m) and fix_percent; `seed` selects the hashed samples.
    method="kabsch" only: weights="conf" weighs every pair by res["conf"], targets="soft" pairs the scene point with
    res["soft_xyz"] instead of its arg-max vertex (both from soft matching, matching.match_frames(soft=...)); either takes the
    weighted entries (solve_poses_weighted).  The defaults are the unweighted launches."""
    if weights not in ("none", "conf") or targets not in ("vertex", "soft"):
        raise ValueError("solve_poses: weights must be 'none' or 'conf' and targets 'vertex' or 'soft', got %r, %r" % (weights, targets))
    soft = weights != "none" or targets != "vertex"
    if method == "ransac":
        if soft:
            raise ValueError("solve_poses: weights=%r / targets=%r are for method='kabsch'; RANSAC keeps the hard pairs" % (weights, targets))
        RT, valid, _, _ = ransac_poses(res, cld_rgb_nrm, model_xyz, ransac_iters, inlier_dist, fix_percent, seed, min_points)
        return RT, valid
    if method != "kabsch":
        raise ValueError("solve_poses: method must be 'kabsch' or 'ransac', got %r" % (method,))
    if soft:
        need = [k for k, on in (("conf", weights == "conf"), ("soft_xyz", targets == "soft")) if on and k not in res]
        if need:
            raise ValueError("solve_poses: weights=%r / targets=%r need the soft matching outputs %s in res" % (weights, targets, need))
        w = res["conf"] if weights == "conf" else torch.ones(res["mask"].shape, dtype=torch.float32, device=res["mask"].device)
        return solve_poses_weighted(res, cld_rgb_nrm, model_xyz, w, res["soft_xyz"] if targets == "soft" else None, min_points)
    st = kabsch_stats(res, cld_rgb_nrm, model_xyz)
    B = st.shape[0]
    RT = torch.empty((B, 3, 4), dtype=torch.float32, device=st.device)
    valid = torch.empty((B,), dtype=torch.uint8, device=st.device)
    check(_lib.lib().gdm_kabsch_solve_hip(st.data_ptr(), B, int(min_points), RT.data_ptr(), valid.data_ptr(), ops._stream()),
          "gdm_kabsch_solve_hip")
    return RT, valid.bool()


def kabsch_stats_weighted(res, cld_rgb_nrm, model_xyz, weight, target=None):
    """The 16 weighted statistics (include/gdm.h gdm_kabsch_stats_w_hip): weight f32[B,N]; the model-side point of a pair is
    target[b, i] (f32[B,N,3]) when given, else model_xyz[best_idx].  -> stats f64[B,16], count i32[B] (masked points with a finite
    weight > 0; the others are skipped)."""
    mask, best_idx = res["mask"], res["best_idx"]
    B, N = mask.shape
    cld = ops._dev(cld_rgb_nrm, torch.float32, "cld_rgb_nrm")
    model_xyz = ops._dev(model_xyz, torch.float32, "model_xyz")
    weight = ops._dev(weight, torch.float32, "weight")
    if tuple(weight.shape) != (B, N):
        raise ValueError("kabsch_stats_weighted: weight is %s, expected %s" % (tuple(weight.shape), (B, N)))
    if target is not None:
        target = ops._dev(target, torch.float32, "target")
        if tuple(target.shape) != (B, N, 3):
            raise ValueError("kabsch_stats_weighted: target is %s, expected %s" % (tuple(target.shape), (B, N, 3)))
    out = torch.empty((B, 16), dtype=torch.float64, device=mask.device)
    count = torch.empty((B,), dtype=torch.int32, device=mask.device)
    check(_lib.lib().gdm_kabsch_stats_w_hip(cld.data_ptr(), cld.stride(0), 1, N, model_xyz.data_ptr(), best_idx.data_ptr(),
                                            None if target is None else target.data_ptr(), weight.data_ptr(), mask.data_ptr(), B, N,
                                            model_xyz.shape[0], out.data_ptr(), count.data_ptr(), ops._stream()),
          "gdm_kabsch_stats_w_hip")
    return out, count


def solve_poses_weighted(res, cld_rgb_nrm, model_xyz, weight, target=None, min_points=5):
    """The weighted least-squares fit: kabsch_stats_weighted, then the fit with n = sum w.  valid = at least min_points usable pairs
    and sum w > 0, else the sentinel pose.  -> RT f32[B,3,4], valid bool[B].  Two launches, no host synchronisation."""
    st, count = kabsch_stats_weighted(res, cld_rgb_nrm, model_xyz, weight, target)
    B = st.shape[0]
    RT = torch.empty((B, 3, 4), dtype=torch.float32, device=st.device)
    valid = torch.empty((B,), dtype=torch.uint8, device=st.device)
    check(_lib.lib().gdm_kabsch_solve_w_hip(st.data_ptr(), count.data_ptr(), B, int(min_points), RT.data_ptr(), valid.data_ptr(),
                                            ops._stream()), "gdm_kabsch_solve_w_hip")
    return RT, valid.bool()


def kabsch_weighted_numpy(A, B, w):
    """fp64 restatement of the weighted fit: A [n,3] model-side points, B [n,3] scene points, w [n] weights >= 0 -> RT [3,4] with
    B ~ R A + t minimising sum w |R A + t - B|^2 (weighted centroids, SVD of sum w (A - cA)(B - cB)^T, reflection fix as
    best_fit_transform)."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    sw = w.sum()
    cA = (w[:, None] * A).sum(0) / sw
    cB = (w[:, None] * B).sum(0) / sw
    H = (w[:, None] * (A - cA)).T @ (B - cB)
    U, _, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        Vt[2, :] *= -1
        R = Vt.T @ U.T
    return np.concatenate([R, (cB - R @ cA)[:, None]], axis=1)


def _mix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def ransac_sample_indices(counts, H, seed=0):
    """The RANSAC samples of include/gdm.h, restated on the CPU (numpy): counts = the selected-pair count n of every crop [B] ->
    i64[B,H,4], row h = the 4 indices (into the crop's selected pairs, in point order) that hypothesis h fits; row 0 (the fit of all
    pairs, no draw) is -1.  mix = lowbias32; r = mix(mix(mix(seed ^ 0x9e3779b9) ^ b) ^ (4 h + s)); index = (uint64(r) * n) >> 32."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    B = counts.shape[0]
    with np.errstate(over="ignore"):
        b = np.arange(B, dtype=np.uint32)[:, None, None]
        hs = (4 * np.arange(H, dtype=np.uint32)[None, :, None] + np.arange(4, dtype=np.uint32)[None, None, :]).astype(np.uint32)
        r = _mix32(_mix32(_mix32(np.uint32(seed & 0xffffffff) ^ np.uint32(0x9e3779b9)) ^ b) ^ hs)
    idx = ((r.astype(np.uint64) * counts.astype(np.uint64)[:, None, None]) >> np.uint64(32)).astype(np.int64)
    idx[:, 0, :] = -1
    return idx


def _scene_args(cld_rgb_nrm):
    """The (pointer, batch stride, point stride, channel stride) of the xyz rows of cld_rgb_nrm f32[B,9,N]."""
    cld = ops._dev(cld_rgb_nrm, torch.float32, "cld_rgb_nrm")
    return cld, cld.stride(0), 1, cld.shape[2]


def ransac_poses(res, cld_rgb_nrm, model_xyz, iters=20, inlier_dist=0.015, fix_percent=0.7, seed=0, min_points=5):
    """Batched best_fit_transform_with_RANSAC (pvn3d_eval_utils_kpls.py:79-124; include/gdm.h gdm_ransac_pose_hip) over the same
    correspondences as solve_poses.  -> RT f32[B,3,4], valid bool[B], counts i32[B,iters] (inliers of every hypothesis), winner
    i32[B] (the hypothesis that decided, -1 for the sentinel).  Five launches, no host synchronisation."""
    H = int(iters)
    if not 1 <= H <= _lib.GDM_RANSAC_MAX_H:
        raise ValueError("ransac_poses: iters=%d not in [1, %d]" % (H, _lib.GDM_RANSAC_MAX_H))
    mask, best_idx = res["mask"], res["best_idx"]
    B, N = mask.shape
    st = kabsch_stats(res, cld_rgb_nrm, model_xyz)
    cld, sb, ps, cs = _scene_args(cld_rgb_nrm)
    model_xyz = ops._dev(model_xyz, torch.float32, "model_xyz")
    L = _lib.lib()
    nbytes = int(L.gdm_ransac_workspace_bytes(B, N, H))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=mask.device)
    RT = torch.empty((B, 3, 4), dtype=torch.float32, device=mask.device)
    valid = torch.empty((B,), dtype=torch.uint8, device=mask.device)
    counts = torch.empty((B, H), dtype=torch.int32, device=mask.device)
    winner = torch.empty((B,), dtype=torch.int32, device=mask.device)
    check(L.gdm_ransac_pose_hip(cld.data_ptr(), sb, ps, cs, model_xyz.data_ptr(), best_idx.data_ptr(), mask.data_ptr(), st.data_ptr(),
                                B, N, model_xyz.shape[0], H, float(inlier_dist), float(fix_percent), int(seed) & 0xffffffff,
                                int(min_points), ws.data_ptr(), nbytes, RT.data_ptr(), valid.data_ptr(), counts.data_ptr(),
                                winner.data_ptr(), ops._stream()), "gdm_ransac_pose_hip")
    return RT, valid.bool(), counts, winner


def refine_icp(RT, valid, cld_rgb_nrm, mask, model_xyz, iters=20, tolerance=0.001, reject_dist=None, min_points=5):
    """Point-to-point ICP from the poses RT f32[B,3,4] (pvn3d_eval_utils_kpls.py:126-212, run scene -> model: the selected scene
    points (mask u8/bool [B,N]) are mapped into the model frame, matched to their nearest model vertex by the exact kNN (K = 1, one
    model cloud f32[M,3] shared by every crop) and the absolute pose is refit from those pairs; pairs farther than reject_dist (m)
    are dropped when it is given).  Exactly `iters` iterations are enqueued (the step captures in a hipGraph); a crop stops on the
    device by the reference's rule (|prev_error - mean| < tolerance, prev_error starting at 0), or when it is invalid or has fewer
    than min_points pairs.  -> RT f32[B,3,4] (a new tensor), iterations run i32[B], final mean residual f32[B] (the mean pair
    distance of the last iteration run; 0 for a crop that ran none)."""
    B, N = mask.shape
    dev = mask.device
    cld, sb, ps, cs = _scene_args(cld_rgb_nrm)
    model_xyz = ops._dev(model_xyz, torch.float32, "model_xyz")
    M = model_xyz.shape[0]
    mask = mask if mask.dtype == torch.uint8 else mask.to(torch.uint8)
    mask = ops._dev(mask, torch.uint8, "mask")
    RT = ops._dev(RT, torch.float32, "RT").clone()
    active = valid.to(torch.uint8).contiguous().clone()
    n_iter = torch.zeros((B,), dtype=torch.int32, device=dev)
    err = torch.zeros((B,), dtype=torch.float64, device=dev)
    if int(iters) <= 0:
        return RT, n_iter, err.float()
    query = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    nn = torch.empty((B, N, 1), dtype=torch.int32, device=dev)
    d2 = torch.empty((B, N, 1), dtype=torch.float32, device=dev)
    job = (_lib.KnnJob * 1)()
    job[0].support, job[0].query, job[0].idx, job[0].d2 = model_xyz.data_ptr(), query.data_ptr(), nn.data_ptr(), d2.data_ptr()
    job[0].support_bstride, job[0].query_bstride = 0, N * 3
    job[0].S, job[0].Q, job[0].K, job[0].grid_w = M, N, 1, 0
    L = _lib.lib()
    reject = -1.0 if reject_dist is None else float(reject_dist)
    for _ in range(int(iters)):
        check(L.gdm_icp_transform_hip(cld.data_ptr(), sb, ps, cs, RT.data_ptr(), B, N, query.data_ptr(), ops._stream()),
              "gdm_icp_transform_hip")
        check(L.gdm_knn_jobs_ws_hip(job, 1, B, None, 0, ops._stream()), "gdm_knn_jobs_ws_hip")
        check(L.gdm_icp_update_hip(cld.data_ptr(), sb, ps, cs, model_xyz.data_ptr(), nn.data_ptr(), d2.data_ptr(), mask.data_ptr(), B, N,
                                   M, reject, float(tolerance), int(min_points), RT.data_ptr(), active.data_ptr(), n_iter.data_ptr(),
                                   err.data_ptr(), ops._stream()), "gdm_icp_update_hip")
    return RT, n_iter, err.float()


def estimate_poses(res, cld_rgb_nrm, model_xyz, pose_fit="kabsch", icp_iters=0, pose_opts=None):
    """The pose stage of the pipeline: solve_poses with `pose_fit` ("kabsch" | "ransac"), then `icp_iters` ICP iterations when > 0.
    pose_opts (optional dict): ransac_iters, ransac_inlier_dist, ransac_fix_percent, seed, icp_tolerance, icp_reject_dist,
    min_points, and for pose_fit="kabsch" weights ("none" | "conf") and targets ("vertex" | "soft") (solve_poses; RANSAC and ICP
    keep the hard pairs).  -> dict(RT, valid[, icp_iters, icp_resid])."""
    o = dict(pose_opts or {})
    unknown = set(o) - {"ransac_iters", "ransac_inlier_dist", "ransac_fix_percent", "seed", "icp_tolerance", "icp_reject_dist",
                        "min_points", "weights", "targets"}
    if unknown:
        raise ValueError("estimate_poses: unknown pose_opts %s" % sorted(unknown))
    min_points = o.get("min_points", 5)
    if pose_fit == "kabsch":
        RT, valid = solve_poses(res, cld_rgb_nrm, model_xyz, min_points, weights=o.get("weights", "none"),
                                targets=o.get("targets", "vertex"))
    else:
        RT, valid = solve_poses(res, cld_rgb_nrm, model_xyz, min_points, method=pose_fit, ransac_iters=o.get("ransac_iters", 20),
                                inlier_dist=o.get("ransac_inlier_dist", 0.015), fix_percent=o.get("ransac_fix_percent", 0.7),
                                seed=o.get("seed", 0), weights=o.get("weights", "none"), targets=o.get("targets", "vertex"))
    out = dict(RT=RT, valid=valid)
    if icp_iters > 0:
        out["RT"], out["icp_iters"], out["icp_resid"] = refine_icp(RT, valid, cld_rgb_nrm, res["mask"], model_xyz, icp_iters,
                                                                   o.get("icp_tolerance", 0.001), o.get("icp_reject_dist"), min_points)
    return out


def transform(pts, RT):
    """pts f32[M,3], RT f32[B,3,4] -> f32[B,M,3]."""
    return pts[None] @ RT[:, :, :3].transpose(1, 2) + RT[:, None, :, 3]


def add_metric(RT_est, RT_gt, model_xyz):
    """pose_error.py:297-312 for a batch: mean vertex distance, f32[B]."""
    return (transform(model_xyz, RT_est) - transform(model_xyz, RT_gt)).norm(dim=2).mean(dim=1)


def adi_metric(RT_est, RT_gt, model_xyz):
    """pose_error.py:315-337: for every GT-posed vertex the nearest estimated-pose vertex (exact 1-NN, HIP)."""
    pe, pg = transform(model_xyz, RT_est).contiguous(), transform(model_xyz, RT_gt).contiguous()
    _, d2 = ops.knn_batch(pe, pg, 1, return_d2=True)
    return d2[:, :, 0].clamp(min=0).sqrt().mean(dim=1)
