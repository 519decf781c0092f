"""Seeded correspondence sets for the consensus fit (tests/test_consensus_cpu.py, tests/test_gpu_consensus.py,
tools/pose_consensus_profile.py): model points in a 0.1 m cube, a random rotation and a translation near (0, 0, 0.8), an inlier share
f, Gaussian noise of SIGMA = 0.5 mm on the scene points, and wrong pairs whose vertex is drawn uniformly over the model.  Every crop is
a dict(model f32[M,3], idx i32[N], scene f32[N,3], mask u8[N], RT f64[3,4] (the true pose), inlier bool[N]); batch() stacks crops over
one model, reference() is pose.consensus_poses_numpy of every crop of a named batch, computed once per process."""
import functools
import zlib

import numpy as np

SIGMA = 5e-4
EXTENT = 0.1
MIN_POINTS = 5
NEAR_MARGIN = 1e-5             # the RANSAC tests' convention: a pair this close to the inlier distance may fall either way


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def rotation(rs):
    q, r = np.linalg.qr(rs.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def make_model(M, seed=0):
    return (EXTENT * _rs("model", M, seed).rand(M, 3)).astype(np.float32)


def make_mask(kind, N, rs):
    """"ones" | "half" (about 50 %) | "most" (about 60 %) | "zero" | "few" (MIN_POINTS - 1 points)."""
    m = np.zeros(N, np.uint8)
    if kind == "ones":
        m[:] = 1
    elif kind in ("half", "most"):
        on = rs.rand(N) < (0.5 if kind == "half" else 0.6)
        m = np.where(on, np.array([1, 2, 255], np.uint8)[rs.randint(0, 3, N)], 0).astype(np.uint8)          # any non-zero byte selects
    elif kind == "few":
        m[rs.choice(N, min(MIN_POINTS - 1, N), replace=False)] = 1
    elif kind != "zero":
        raise ValueError(kind)
    return m


def make_crop(model, N, f, seed, mask="ones", extra=None):
    """One crop over `model`.  extra: None | "clamp" (a tenth of the indices outside [0, M): -1, M, 2^31 - 1, -2^31 -- the clamp makes
    them vertex 0 or M - 1) | "repeat" (the true vertices are only 12, used many times each: b2 = 0 between copies) | "twins" (scene
    points 1, 3, 5, ... of the first 16 copy their left neighbour bit for bit: a2 = 0) | "clump" (90 wrong pairs, or N // 5 in a small
    crop, collapsed onto one vertex and one scene spot)."""
    rs = _rs("crop", len(model), N, f, seed, mask, extra)
    M = len(model)
    R, t = rotation(rs), np.array([0.05 * rs.randn(), 0.05 * rs.randn(), 0.8 + 0.05 * rs.randn()])
    true = rs.randint(0, M, N)
    if extra == "repeat":
        true = rs.choice(M, 12, replace=False)[rs.randint(0, 12, N)]
    scene = (model[true].astype(np.float64) @ R.T + t + SIGMA * rs.randn(N, 3)).astype(np.float32)
    inlier = np.zeros(N, bool)
    inlier[rs.permutation(N)[:int(round(f * N))]] = True
    idx = np.where(inlier, true, rs.randint(0, M, N)).astype(np.int64)
    if extra == "repeat":
        idx = np.where(inlier, true, rs.randint(0, M, N))
    if extra == "clamp":
        odd = rs.rand(N) < 0.1
        idx[odd] = np.array([-1, M, 2 ** 31 - 1, -2 ** 31])[rs.randint(0, 4, int(odd.sum()))]
    if extra == "twins":
        k = min(16, N - N % 2)
        scene[1:k:2] = scene[0:k:2]
    if extra == "clump":
        c = min(90, N // 5)
        pos = np.nonzero(~inlier)[0][:c]
        spot = t + EXTENT * (rs.rand(3) - 0.5)
        scene[pos] = (spot + SIGMA * rs.randn(len(pos), 3)).astype(np.float32)
        idx[pos] = rs.randint(0, M)
    inlier &= idx == true
    return dict(model=model, idx=idx.astype(np.int32), scene=scene, mask=make_mask(mask, N, rs), RT=np.concatenate([R, t[:, None]], 1),
                inlier=inlier)


def matched(crop):
    """The model point of every scene point as the kernels take it: model[clamp(idx, 0, M - 1)], f32[N,3]."""
    return crop["model"][np.clip(crop["idx"].astype(np.int64), 0, len(crop["model"]) - 1)]


def add_error(RT, crop):
    """ADD in metres: the mean distance of the model's vertices under RT and under the true pose."""
    m = crop["model"].astype(np.float64)
    RT, gt = np.asarray(RT, np.float64), crop["RT"]
    return float(np.linalg.norm((m @ RT[:, :3].T + RT[:, 3]) - (m @ gt[:, :3].T + gt[:, 3]), axis=1).mean())


def kabsch_all(crop):
    """Plain least squares over every selected pair, fp64 -> RT [3,4]."""
    from geometric_aware_dense_matching_amd import pose
    sel = crop["mask"] != 0
    return pose.kabsch_weighted_numpy(matched(crop)[sel], crop["scene"][sel], np.ones(int(sel.sum())))


# The committed batches: name -> (N, M, data seed, [(f, mask kind, extra), ...] one per crop).  The shapes are the smallest with a
# partial and a full 64-bit word, more than one 64-row tile and a masked tail; the last is the workload's 32 words per row.  The data
# seeds are ones at which the restatement alone excuses nothing (tests/test_consensus_cpu.py asserts it): no hypothesis fails the
# conditioning gate and no decision hangs on a pair within NEAR_MARGIN of the inlier distance.
BATCHES = {
    "1x5": (5, 40, 1, [(1.0, "ones", None)]),
    "2x63": (63, 300, 2, [(0.5, "ones", None), (0.6, "half", "clamp")]),
    "2x64": (64, 300, 33, [(0.5, "ones", "twins"), (0.5, "ones", "repeat")]),
    "3x65": (65, 300, 4, [(0.5, "ones", None), (0.5, "zero", None), (0.5, "few", None)]),
    "2x130": (130, 300, 5, [(0.3, "ones", None), (0.5, "half", "clamp")]),
    "1x257": (257, 300, 6, [(0.2, "ones", "twins")]),
    "2x513": (513, 300, 7, [(0.1, "ones", None), (0.15, "ones", "clump")]),
    "2x2048": (2048, 8192, 8, [(0.3, "most", None), (0.2, "most", "clamp")]),
}
RECOVERY = [(65, 0.5), (130, 0.3), (257, 0.2), (513, 0.1)]
RECOVERY_SEEDS = range(8)
CLUMP_SEEDS = range(6)


@functools.lru_cache(maxsize=None)
def batch(name):
    """-> dict(model f32[M,3], idx i32[B,N], cld f32[B,9,N] (rows 0..2 = the scene points, the rest random), mask u8[B,N], crops)."""
    N, M, seed, rows = BATCHES[name]
    model = make_model(M, seed)
    crops = [make_crop(model, N, f, (seed, b), kind, extra) for b, (f, kind, extra) in enumerate(rows)]
    cld = _rs("cld", name).rand(len(crops), 9, N).astype(np.float32)
    for b, c in enumerate(crops):
        cld[b, :3] = c["scene"].T
    return dict(model=model, idx=np.stack([c["idx"] for c in crops]), cld=cld, mask=np.stack([c["mask"] for c in crops]), crops=crops)


@functools.lru_cache(maxsize=None)
def recovery_crop(n, f, seed):
    return make_crop(make_model(300), n, f, ("recovery", seed))


@functools.lru_cache(maxsize=None)
def clump_crop(seed):
    return make_crop(make_model(300), 513, 0.15, ("clump", seed), extra="clump")


@functools.lru_cache(maxsize=None)
def reference(name, seeds=8, tau=0.005, inlier_dist=0.015):
    """consensus_poses_numpy of every crop of batch(name), once per process; the callers leave it unchanged."""
    from geometric_aware_dense_matching_amd import pose
    return [pose.consensus_poses_numpy(c["scene"], matched(c), c["mask"], tau, seeds, inlier_dist, MIN_POINTS, NEAR_MARGIN)
            for c in batch(name)["crops"]]


def fit_gap(ref, crop, t):
    """The conditioning gate of the fit tests (oracle/pose_ref.py check_fit): (s1 + sign s2) / s0 of the weighted covariance of
    hypothesis t -- the fit is unique, and pinned to the SVD answer, only when this exceeds 1e-3."""
    w = ref["weights"][t]
    pos = w > 0
    A = matched(crop)[ref["sel"]][pos].astype(np.float64)
    P = crop["scene"][ref["sel"]][pos].astype(np.float64)
    w = w[pos]
    cA, cP = (w[:, None] * A).sum(0) / w.sum(), (w[:, None] * P).sum(0) / w.sum()
    H = (w[:, None] * (A - cA)).T @ (P - cP)
    U, s, Vt = np.linalg.svd(H)
    sign = np.sign(np.linalg.det(Vt.T @ U.T))
    return float((s[1] + sign * s[2]) / max(s[0], 1e-300))


def winner_pinned(ref, min_points=MIN_POINTS):
    """Could a pair within NEAR_MARGIN of the inlier distance change the decision of this crop, or the refit's inlier set?  With
    lo = c - near and hi = c + near per hypothesis: the winner w is pinned when every other live t has hi_t < lo_w, or both counts are
    exact (near = 0: the rule itself decides the tie); the validity threshold likewise; and the winner's own inlier set must be exact."""
    c, near = ref["counts"], ref["near"]
    live = c >= 0
    if not live.any():
        return True
    w = int(np.argmax(c))
    for t in np.nonzero(live)[0]:
        if t != w and not (c[t] + near[t] < c[w] - near[w] or (near[t] == 0 and near[w] == 0)):
            return False
    if near[w] and (c[w] - near[w] < min_points <= c[w] + near[w]):
        return False
    return not (ref["valid"] and near[w])
