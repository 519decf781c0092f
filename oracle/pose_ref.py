"""ORACLE -- test infrastructure only; never imported by the product package.

numpy restatements of /root/reference/utils/pvn3d_eval_utils_kpls.py:43-77 (best_fit_transform) and
/root/reference/lib/pysixd/pose_error.py:297-337 (add, adi; misc.transform_pts_Rt :895-905).
Pinned by tests/golden/pose.npz, which the golden script produced by executing those functions from the
reference's own source text.

ransac / icp restate best_fit_transform_with_RANSAC (:79-124) and icp (:126-212) of the same file, with the draws passed in and the
per-hypothesis / per-iteration tables the tests need returned beside the answer.  Pinned by tests/golden/pose_robust.npz (made by
the real reference): tests/test_pose_robust_cpu.py."""
import numpy as np
from scipy import spatial


def best_fit_transform(A, B):
    m = A.shape[1]
    cA, cB = np.mean(A, axis=0), np.mean(B, axis=0)
    H = np.dot((A - cA).T, B - cB)
    U, S, Vt = np.linalg.svd(H)
    R = np.dot(Vt.T, U.T)
    if np.linalg.det(R) < 0:
        Vt[m - 1, :] *= -1
        R = np.dot(Vt.T, U.T)
    T = np.zeros((3, 4))
    T[:, :3] = R
    T[:, 3] = cB.T - np.dot(R, cA.T)
    return T


def transform_pts_Rt(pts, R, t):
    return (R.dot(pts.T) + t.reshape((3, 1))).T


def add(R_est, t_est, R_gt, t_gt, pts):
    return np.linalg.norm(transform_pts_Rt(pts, R_est, t_est) - transform_pts_Rt(pts, R_gt, t_gt), axis=1).mean()


def adi(R_est, t_est, R_gt, t_gt, pts):
    pe, pg = transform_pts_Rt(pts, R_est, t_est), transform_pts_Rt(pts, R_gt, t_gt)
    d, _ = spatial.cKDTree(pe).query(pg, k=1)
    return d.mean()


def best_fit_transforms(A, B):
    """best_fit_transform for a stack: A, B f64[K,n,3] -> T f64[K,3,4], s f64[K,3] (singular values of H), sign f64[K] (+1 / -1:
    whether the reflection fix was applied).  The rotation is unique iff (s2 + sign * s3) / s1 > 0."""
    cA, cB = A.mean(1), B.mean(1)
    H = (A - cA[:, None]).transpose(0, 2, 1) @ (B - cB[:, None])
    U, S, Vt = np.linalg.svd(H)
    sign = np.where(np.linalg.det(np.einsum("kji,kmj->kim", Vt, U)) < 0, -1.0, 1.0)
    Vt = Vt.copy()
    Vt[:, 2, :] *= sign[:, None]
    R = np.einsum("kji,kmj->kim", Vt, U)
    T = np.zeros((A.shape[0], 3, 4))
    T[:, :, :3] = R
    T[:, :, 3] = cB - np.einsum("kij,kj->ki", R, cA)
    return T, S, sign


def check_fit(RT, A, B, unique):
    """The assertions on a pose fit against the SVD answer (tests/test_pose_fit_cpu.py states the bounds), for one stack: RT f32[K,3,4] (the fragment's or the kernel's), A, B [K,n,3].  -> the smallest
    uniqueness gap seen."""
    A, B = A.astype(np.float64), B.astype(np.float64)
    T, s, sign = best_fit_transforms(A, B)
    assert np.isfinite(RT).all()
    R, t = RT[:, :, :3].astype(np.float64), RT[:, :, 3].astype(np.float64)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 2e-7
    assert np.abs(np.linalg.det(R) - 1.0).max() <= 2e-7
    H = (A - A.mean(1, keepdims=True)).transpose(0, 2, 1) @ (B - B.mean(1, keepdims=True))
    obj = np.einsum("kij,kji->k", R, H)
    best = np.einsum("kij,kji->k", T[:, :, :3], H)
    assert (obj >= best - 2e-7 * s[:, 0]).all(), float((best - obj - 2e-7 * s[:, 0]).max())
    gap = (s[:, 1] + sign * s[:, 2]) / np.maximum(s[:, 0], 1e-300)
    if unique:
        assert gap.min() > 1e-3, gap.min()                             # no case may be skipped: pick another seed instead
        assert np.abs(R - T[:, :, :3]).max() <= 1e-7, float(np.abs(R - T[:, :, :3]).max())
        tol = 2.0 ** -23 * np.maximum(1.0, np.abs(T[:, :, 3]).max(1))
        assert (np.abs(t - T[:, :, 3]).max(1) <= tol).all(), float((np.abs(t - T[:, :, 3]).max(1) / tol).max())
    return float(gap.min())


def residuals(T, A, B):
    """|R a + t - b| of every pair under every pose: T [K,3,4], A, B [n,3] -> f64[K,n]."""
    return np.linalg.norm(np.einsum("kij,nj->kni", T[:, :, :3], A) + T[:, None, :, 3] - B[None], axis=2)


def ransac_decide(counts, n, fix_percent):
    """The reference's sequential rule on the inlier counts of the hypotheses in draw order (:102-110): the first h whose count
    exceeds fix_percent * n wins and is refit; otherwise the largest count (the earliest on ties) wins as it is; no inlier at all ->
    winner -1 (the reference returns zeros).  -> (winner, refit)."""
    counts = np.asarray(counts)
    over = np.nonzero(counts > fix_percent * n)[0]
    if len(over):
        return int(over[0]), True
    if counts.max() <= 0:
        return -1, False
    return int(np.argmax(counts)), False


def ransac(A, B, samples, match_err=0.015, fix_percent=0.7, near_margin=1e-5, degenerate_sv=1e-4, chunk=256):
    """A = matched model vertices, B = scene points, f64[n,3] (the selected pairs in point order); samples i64[H,4] = the draws of
    every hypothesis (row 0 is ignored: hypothesis 0 is the fit of all pairs).  -> dict
      poses f64[H,3,4], counts i64[H] (pairs with error <= match_err), near i64[H] (pairs with |error - match_err| < near_margin),
      degenerate bool[H] (second singular value of the sample's centred model points <= degenerate_sv: no unique rotation),
      winner, refit, RT (f64[3,4], None when winner is -1).
    The H x n residual matrix is evaluated `chunk` hypotheses at a time."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    samples = np.asarray(samples)
    H = samples.shape[0]
    poses = np.zeros((H, 3, 4))
    degenerate = np.zeros(H, bool)
    poses[0] = best_fit_transform(A, B)
    degenerate[0] = np.linalg.svd(A - A.mean(0), compute_uv=False)[1] <= degenerate_sv
    if H > 1:
        sA = A[samples[1:]]
        poses[1:] = best_fit_transforms(sA, B[samples[1:]])[0]
        degenerate[1:] = np.linalg.svd(sA - sA.mean(1, keepdims=True), compute_uv=False)[:, 1] <= degenerate_sv
    counts, near = np.zeros(H, np.int64), np.zeros(H, np.int64)
    for h0 in range(0, H, chunk):
        err = residuals(poses[h0:h0 + chunk], A, B)
        counts[h0:h0 + chunk] = (err <= match_err).sum(1)
        near[h0:h0 + chunk] = (np.abs(err - match_err) < near_margin).sum(1)
    out = dict(poses=poses, counts=counts, near=near, degenerate=degenerate)
    out["winner"], out["refit"] = ransac_decide(counts, A.shape[0], fix_percent)
    out["RT"] = ransac_pose(A, B, poses, out["winner"], out["refit"], match_err)
    return out


def ransac_pose(A, B, poses, winner, refit, match_err):
    """The pose the rule returns for a decision: the winner's pose, refit on its inliers when it exited early."""
    if winner < 0:
        return None
    if not refit:
        return poses[winner].copy()
    inl = residuals(poses[winner:winner + 1], A, B)[0] <= match_err
    return best_fit_transform(A[inl], B[inl])


def icp_step(scene, model, RT, reject_dist=None, tie_margin=1e-6):
    """One iteration from the pose RT (model -> scene) over the given scene points: they are mapped into the model frame, paired
    with their nearest model vertex, pairs farther than reject_dist dropped, and the absolute pose refit from (vertex, scene point).
    (The reference updates the mapped points by the increment T and refits at the end; the increment composed with the current
    pose is the least-squares fit of the same pairs.)  -> dict RT (None when no pair is kept), n (pairs kept), mean (their
    mean distance), ties (indices of the queries whose two nearest vertices are within tie_margin), tie_shift (sum over those of
    |v1 - v2|), query f64[n0,3], nn, dist."""
    R, t = RT[:, :3], RT[:, 3]
    query = (scene - t) @ R
    dist, nn = spatial.cKDTree(model).query(query, k=2)
    ties = np.nonzero(dist[:, 1] - dist[:, 0] < tie_margin)[0]
    tie_shift = float(np.linalg.norm(model[nn[ties, 0]] - model[nn[ties, 1]], axis=1).sum())
    keep = np.ones(len(scene), bool) if reject_dist is None else dist[:, 0] <= reject_dist
    n = int(keep.sum())
    new = best_fit_transform(model[nn[keep, 0]], scene[keep]) if n >= 1 else None
    mean = float(dist[keep, 0].mean()) if n >= 1 else 0.0
    return dict(RT=new, n=n, mean=mean, ties=ties, tie_shift=tie_shift, query=query, nn=nn[:, 0], dist=dist[:, 0], keep=keep)


def icp(scene, model, RT0, mask=None, iters=20, tol=0.001, reject_dist=None, min_points=5):
    """Point-to-point ICP, scene -> model, as geometric_aware_dense_matching_amd.pose.refine_icp documents it: scene f64[N,3],
    model f64[M,3], RT0 f64[3,4] (model -> scene), mask [N] (the scene points that take part).  Stops after the update of the
    iteration whose mean distance differs from the previous one (0 before the first) by less than tol, or, unchanged, at an
    iteration with fewer than min_points pairs.  -> dict RT (final), RTs (the pose after every iteration run), resid (the mean
    distance of every iteration run), iters, ties (per iteration, icp_step's list), tie_shift, n (pairs per iteration),
    stop_margin (the smallest | |prev - mean| - tol | over the iterations run), starved (stopped for lack of pairs)."""
    scene, model = np.asarray(scene, np.float64), np.asarray(model, np.float64)
    sel = np.ones(len(scene), bool) if mask is None else np.asarray(mask) != 0
    pts = scene[sel]
    RT = np.asarray(RT0, np.float64).copy()
    out = dict(RTs=[], resid=[], ties=[], tie_shift=[], n=[], stop_margin=np.inf, starved=False)
    prev = 0.0
    for _ in range(iters):
        if len(pts) < 1:
            out["starved"] = True
            break
        s = icp_step(pts, model, RT, reject_dist)
        if s["n"] < min_points:
            out["starved"] = True
            break
        RT = s["RT"]
        out["RTs"].append(RT)
        out["resid"].append(s["mean"])
        out["ties"].append(np.nonzero(sel)[0][s["ties"]])
        out["tie_shift"].append(s["tie_shift"])
        out["n"].append(s["n"])
        out["stop_margin"] = min(out["stop_margin"], abs(abs(prev - s["mean"]) - tol))
        if abs(prev - s["mean"]) < tol:
            break
        prev = s["mean"]
    out["RT"], out["iters"] = RT, len(out["RTs"])
    return out
