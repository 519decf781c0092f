#!/usr/bin/env python3
"""Generates tests/golden/pose_robust.npz from the REAL reference's robust pose fitting.

Runs ONLY where the reference tree is mounted (the build container); nothing here travels to the GPU box except the .npz it writes.
It imports utils/pvn3d_eval_utils_kpls.py of the reference -- best_fit_transform_with_RANSAC (:79-124), best_fit_transform (:43-77)
and icp (:126-212) -- with empty stand-in modules for what that module imports but these functions never use (cv2, common,
utils.basic_utils, utils.meanshift_pytorch, numpy.lib.function_base), and runs them unchanged, with two seams patched:

  np.random.seed       does nothing
  np.random.randint    returns the crop's samples of pose.ransac_sample_indices (the counter-based hash of include/gdm.h), in draw
                       order: the reference's i-th draw is hypothesis i + 1
  best_fit_transform   (module global) is wrapped to record every hypothesis pose the reference fits, and which hypothesis it refit
  nearest_neighbor     (module global) is wrapped to count ICP iterations, record each iteration's mean distance and check that the
                       data has no nearest-neighbour near-ties

RANSAC cases (one crop each, shared model cloud, H = max_iter = 20, match_err = 0.015, fix_percent = 0.7, seed 0):
  0  exits early on a drawn hypothesis (25 % gross outliers: the fit of all pairs has too few inliers)
  1  no hypothesis exceeds fix_percent (45 % outliers): the best hypothesis, no refit
  2  fewer than 5 selected points: the evaluator's sentinel (evaluator.py:94-96)
  3  zero inliers for every hypothesis (no consistent pose): the reference returns zeros, the product the sentinel
  4  exits at hypothesis 0 (5 % outliers): the refit of the all-pairs fit's inliers
ICP cases: equal-count clouds (icp asserts A.shape == B.shape): the scene is the model posed + 1 mm noise, started 5 deg and 1 cm
off.  icp(A=scene, B=model, init=RT0^-1) is the inverse of the product's refine_icp(RT0) (scene -> model).

Data are regenerated (next data seed) until they are tie-free: no point within 1e-5 m of match_err for the winning hypothesis, every
4-point sample non-degenerate (second singular value of the centred model points > 1e-4: a unique rotation; draws are
with replacement, so a sample may hold only 3 distinct points), no ICP nearest-neighbour pair within
1e-6 m of the second nearest, no ICP |prev_error - mean| within 1e-5 of the tolerance.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)

from geometric_aware_dense_matching_amd.pose import ransac_sample_indices  # noqa: E402

H, MATCH_ERR, FIX, SEED = 20, 0.015, 0.7, 0
N, M = 256, 400
ICP_N, ICP_ITERS, ICP_TOL = 400, 20, 0.001


def load_reference():
    assert os.path.isdir(REF), "reference tree not mounted"
    sys.path.insert(0, REF)

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    stub("cv2", imshow=None, waitKey=None)
    stub("common", Config=object)
    stub("numpy.lib.function_base", append=np.append)
    import utils  # noqa: F401  (namespace package of the reference)
    stub("utils.basic_utils", Basic_Utils=object, check_match_distance=None)
    stub("utils.meanshift_pytorch", MeanShiftTorch=object)
    import utils.pvn3d_eval_utils_kpls as K
    return K


def rand_rot(rs, deg=None):
    if deg is None:
        q, _ = np.linalg.qr(rs.randn(3, 3))
        return q * np.sign(np.linalg.det(q))
    ax = rs.randn(3)
    ax /= np.linalg.norm(ax)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def ransac_data(rs):
    model = ((rs.rand(M, 3) - 0.5) * 0.2).astype(np.float32)
    B = 5
    cld = np.zeros((B, 9, N), np.float32)
    idx = rs.randint(0, M, size=(B, N)).astype(np.int32)
    mask = np.zeros((B, N), np.uint8)
    n_sel = [200, 220, 3, 120, 180]
    outlier = [0.25, 0.45, 0.0, 1.0, 0.05]
    for b in range(B):
        R, t = rand_rot(rs), np.array([0.03 * b, -0.02, 0.8])
        pts = model[idx[b]].astype(np.float64) @ R.T + t + 0.001 * rs.randn(N, 3)
        sel = np.sort(rs.choice(N, n_sel[b], replace=False))
        mask[b, sel] = 1
        bad = sel[rs.rand(len(sel)) < outlier[b]]
        if outlier[b] >= 1.0:
            pts = rs.rand(N, 3) * 2.0 - 1.0 + np.array([0, 0, 2.0])         # no consistent pose at all
        else:
            pts[bad] += (0.08 + 0.2 * rs.rand(len(bad), 1)) * rs.randn(len(bad), 3) / 1.7
        cld[b, :3] = pts.T.astype(np.float32)
        cld[b, 3:] = rs.rand(6, N)
    return dict(model=model, idx=idx, mask=mask, cld=cld)


def run_ransac(K, d):
    B = d["mask"].shape[0]
    n = d["mask"].sum(1).astype(np.int64)
    samples = ransac_sample_indices(n, H + 1, SEED)        # the reference draws once more after its last scored hypothesis
    RT = np.zeros((B, 3, 4))
    valid = np.zeros(B, np.uint8)
    winner = np.full(B, -1, np.int32)
    counts = np.zeros((B, H), np.int32)
    near = np.zeros((B, H), np.int32)
    hyps = np.zeros((B, H, 3, 4))
    orig_fit = K.best_fit_transform
    for b in range(B):
        sel = d["mask"][b] != 0
        A = d["model"][d["idx"][b][sel]].astype(np.float64)
        Bp = d["cld"][b, :3, sel].astype(np.float64)
        if n[b] < 5:                                                   # evaluator.py:94-96: the sentinel before any fit
            RT[b] = np.hstack([np.eye(3), [[0], [0], [-1000]]])
            continue
        for h in range(1, H):
            s = A[samples[b, h]]
            if np.linalg.svd(s - s.mean(0), compute_uv=False)[1] <= 1e-4:
                return None
        # every hypothesis (the reference only scores those up to its exit): the reference's own fit of the same pairs
        for h in range(H):
            sl = slice(None) if h == 0 else samples[b, h]
            T = orig_fit(A[sl], Bp[sl])
            hyps[b, h] = T
            err = np.linalg.norm(A @ T[:, :3].T + T[:, 3] - Bp, axis=1)
            counts[b, h] = int((err <= MATCH_ERR).sum())
            near[b, h] = int((np.abs(err - MATCH_ERR) < 1e-5).sum())
        # the reference's run, with its draws answered by our samples and its fits recorded
        draws = iter(samples[b, 1:])
        state = {"draws": 0, "expect_sample": False, "refit_of": None, "calls": 0}

        def randint(lo, hi, size):
            assert lo == 0 and hi == n[b] and size == 4
            state["draws"] += 1
            state["expect_sample"] = True
            return next(draws)

        def fit(a, bb):
            if state["calls"] > 0 and not state["expect_sample"]:
                state["refit_of"] = state["draws"]
            state["expect_sample"] = False
            state["calls"] += 1
            return orig_fit(a, bb)

        saved = (np.random.seed, np.random.randint)
        np.random.seed, np.random.randint = (lambda *a, **k: None), randint
        K.best_fit_transform = fit
        try:
            out = K.best_fit_transform_with_RANSAC(A, Bp, max_iter=H, match_err=MATCH_ERR, fix_percent=FIX)
        finally:
            np.random.seed, np.random.randint = saved
            K.best_fit_transform = orig_fit
        if state["refit_of"] is not None:
            w = state["refit_of"]
        elif counts[b].max() > 0:
            w = int(np.argmax(counts[b]))
            assert np.allclose(out, hyps[b, w])
        else:
            w = -1
            assert not out.any()                                       # the reference's zero matrix
        if w >= 0:
            if near[b, w] != 0:
                return None
            RT[b], valid[b], winner[b] = out, 1, w
        else:
            RT[b] = np.hstack([np.eye(3), [[0], [0], [-1000]]])        # the documented deviation: the sentinel
    return dict(r_samples=samples[:, :H], r_counts=counts, r_near=near, r_RT=RT, r_valid=valid, r_winner=winner)


def icp_data(rs):
    model = ((rs.rand(ICP_N, 3) - 0.5) * np.array([0.16, 0.12, 0.08])).astype(np.float32)
    B = 2
    cld = np.zeros((B, 9, ICP_N), np.float32)
    RT0 = np.zeros((B, 3, 4), np.float32)
    for b in range(B):
        R, t = rand_rot(rs), np.array([0.02 * b, 0.01, 0.7])
        pts = model.astype(np.float64) @ R.T + t + 0.001 * rs.randn(ICP_N, 3)
        cld[b, :3] = rs.permutation(pts).T.astype(np.float32)          # no point-order correspondence
        cld[b, 3:] = rs.rand(6, ICP_N)
        dR = rand_rot(rs, 5.0)
        dt = rs.randn(3)
        dt *= 0.01 / np.linalg.norm(dt)
        RT0[b, :, :3], RT0[b, :, 3] = dR @ R, t + dt
    return dict(model=model, cld=cld, RT0=RT0)


def run_icp(K, d):
    from sklearn.neighbors import NearestNeighbors
    B = d["RT0"].shape[0]
    model = d["model"].astype(np.float64)
    RT = np.zeros((B, 3, 4))
    iters = np.zeros(B, np.int32)
    resid = np.zeros(B)
    orig_nn = K.nearest_neighbor
    for b in range(B):
        scene = d["cld"][b, :3].T.astype(np.float64)
        R0, t0 = d["RT0"][b, :, :3].astype(np.float64), d["RT0"][b, :, 3].astype(np.float64)
        init = np.eye(4)
        init[:3, :3], init[:3, 3] = R0.T, -R0.T @ t0
        means = []
        ok = [True]

        def nn(src, dst):
            dist, ind = orig_nn(src, dst)
            d2, _ = NearestNeighbors(n_neighbors=2).fit(dst).kneighbors(src)
            if (d2[:, 1] - d2[:, 0]).min() < 1e-6:
                ok[0] = False
            means.append(float(np.mean(dist)))
            return dist, ind

        K.nearest_neighbor = nn
        try:
            T = K.icp(scene, model, init_pose=init, max_iterations=ICP_ITERS, tolerance=ICP_TOL)
        finally:
            K.nearest_neighbor = orig_nn
        prev = [0.0] + means[:-1]
        if not ok[0] or min(abs(abs(p - m) - ICP_TOL) for p, m in zip(prev, means)) < 1e-5:
            return None
        Rm, tm = T[:, :3], T[:, 3]                                     # scene -> model; the product reports model -> scene
        RT[b, :, :3], RT[b, :, 3] = Rm.T, -Rm.T @ tm
        iters[b], resid[b] = len(means), means[-1]
    return dict(i_RT=RT, i_iters=iters, i_resid=resid)


def main():
    K = load_reference()
    for data_seed in range(100):
        rs = np.random.RandomState(1000 + data_seed)
        rd = ransac_data(rs)
        rr = run_ransac(K, rd)
        if rr is None or not (rr["r_winner"][0] > 0 and rr["r_winner"][4] == 0):      # cases 0 and 4 as described above
            continue
        idd = icp_data(rs)
        ir = run_icp(K, idd)
        if ir is None:
            continue
        break
    else:
        raise RuntimeError("no tie-free data found")
    w = rr["r_winner"]
    assert w[0] > 0 and w[4] == 0 and rr["r_valid"][2] == 0 and w[3] == -1 and rr["r_counts"][3].max() == 0
    assert rr["r_counts"][1].max() <= FIX * rd["mask"][1].sum()
    out = dict(data_seed=np.int64(1000 + data_seed), H=np.int64(H), match_err=np.float64(MATCH_ERR), fix_percent=np.float64(FIX),
               seed=np.int64(SEED), r_model=rd["model"], r_idx=rd["idx"], r_mask=rd["mask"], r_cld=rd["cld"],
               i_model=idd["model"], i_cld=idd["cld"], i_RT0=idd["RT0"], i_max_iters=np.int64(ICP_ITERS), i_tol=np.float64(ICP_TOL))
    out.update(rr)
    out.update(ir)
    np.savez_compressed(os.path.join(HERE, "pose_robust.npz"), **out)
    print("pose_robust.npz: data seed %d, winners %s, counts max %s, icp iterations %s" %
          (1000 + data_seed, w.tolist(), rr["r_counts"].max(1).tolist(), ir["i_iters"].tolist()))


if __name__ == "__main__":
    main()
