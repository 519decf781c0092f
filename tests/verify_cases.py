"""The scenes shared by tests/test_pose_verify_cpu.py and tests/test_gpu_depth_verify.py (pose.verify_poses): small
meshes made of render.demo_mesh plus hand-made triangles, a 96 x 80 frame, candidate poses and observed depth.  Pure numpy, seeded;
every observed depth image is made by evaluation.render_depth_numpy, so the scenes need no GPU."""
import functools

import numpy as np

from geometric_aware_dense_matching_amd import evaluation, render

H, W = 80, 96
K0 = np.array([[150.0, 0.0, 47.3], [0.0, 148.0, 39.6], [0.0, 0.0, 1.0]])
NEAR = 0.05
DELTA_EDGE = 2.0 ** -6


def rot(angle, axis):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx.dot(Kx)


def pose(R, t):
    return np.hstack([R, np.asarray(t, dtype=np.float64)[:, None]])


@functools.lru_cache(maxsize=None)
def mixed_mesh(level=1):
    """demo_mesh(level) (80 faces at level 1, 320 at level 2) in the object frame plus, expressed in the same frame so that one pose moves all of it: a
    triangle 0.7 across behind the object (under the poses below it covers all four tiles of the frame: the cooperative path), a
    triangle whose third vertex lies 0.5 in front (behind `near` once posed at z = 0.45) and a degenerate triangle.  At level 2 the
    large triangle is face 320: the second trip of a 256-thread face loop, thread 64, so wave 1."""
    m = render.demo_mesh(level=level, seed=4)
    v, f = m["verts"], m["faces"]
    extra = np.array([[-0.45, -0.3, 0.12], [0.45, -0.28, 0.15], [0.02, 0.42, 0.1],            # the large one
                      [0.03, 0.03, 0.0], [0.05, 0.03, 0.0], [0.04, 0.05, -0.5],                # reaches behind near
                      [0.01, 0.0, -0.06], [0.02, 0.0, -0.06], [0.03, 0.0, -0.06]])             # collinear: snapped area 0
    n0 = len(v)
    ef = np.arange(9, dtype=np.int32).reshape(3, 3) + n0
    return np.concatenate([v, extra]), np.concatenate([f, ef]).astype(np.int32)


def _candidates(n, C, seed):
    """RT f64[n,C,3,4]: per instance a base pose near (0, 0, 0.45) and C - 1 perturbations of it (millimetres and degrees)."""
    rs = np.random.RandomState(seed)
    RT = np.zeros((n, C, 3, 4))
    for i in range(n):
        R = rot(0.3 + 0.5 * i, (1.0, 0.4 * i, 0.2))
        t = np.array([0.01 * i - 0.01, 0.005 * i, 0.45 + 0.02 * i])
        RT[i, 0] = pose(R, t)
        for c in range(1, C):
            dR = rot(0.05 * rs.randn(), rs.randn(3))
            RT[i, c] = pose(dR.dot(R), t + rs.randn(3) * np.array([0.004, 0.004, 0.006]))
    return RT


def _observed(verts, faces, RT0, K, seed):
    """Observed depth f32[n,H,W]: candidate 0 rendered, a flat background at 0.9 where nothing is drawn, millimetre noise, then a
    block of zeros, a block of NaN, a block of negative values and an occluder (0.2) block."""
    n = RT0.shape[0]
    d = evaluation.render_depth_numpy(verts, faces, RT0, K, H, W, NEAR)
    rs = np.random.RandomState(seed)
    d = np.where(d > 0, d, np.float32(0.9)).astype(np.float32) + (0.004 * rs.randn(n, H, W)).astype(np.float32)
    d[:, 30:40, 35:50] = 0.0
    d[:, 42:50, 40:60] = np.nan
    d[:, 20:28, 50:58] = -1.0
    d[:, 34:60, 20:34] = 0.2
    return d


BIG_LATE = "n1 C5 f32, 323 faces"    # mixed_mesh(2): the large triangle on a later trip of the face loop, in a wave other than 0


def mixed_case(name):
    """One of the mixed scenes, as the keyword arguments of verify_poses / verify_poses_numpy."""
    verts, faces = mixed_mesh(2 if name == BIG_LATE else 1)
    if name == "n3 C5 f32 K,depth per instance":
        n, C, dtype, kper, dper = 3, 5, np.float32, True, True
        window = np.array([[3, 5, 72, 49], [0, 0, 95, 79], [44, 36, 44, 36]], dtype=np.int32)
    elif name == "n3 C5 f64 K,depth shared":
        n, C, dtype, kper, dper = 3, 5, np.float64, False, False
        window = np.array([[-20, -10, 50, 200], [200, 200, 300, 300], [60, 50, 95, 79]], dtype=np.int32)     # outside, gone, corner
    elif name == "n1 C1 f32 whole frame":
        n, C, dtype, kper, dper, window = 1, 1, np.float32, False, True, None
    elif name == "n1 C5 f64 whole frame":
        n, C, dtype, kper, dper, window = 1, 5, np.float64, True, False, None
    elif name == BIG_LATE:
        n, C, dtype, kper, dper, window = 1, 5, np.float32, False, True, None
    else:
        raise KeyError(name)
    RT = _candidates(n, C, seed=len(name))
    K = np.stack([K0 + np.array([[2.0 * i, 0, 0.7 * i], [0, -1.5 * i, -0.4 * i], [0, 0, 0]]) for i in range(n)]) if kper else K0
    depth = _observed(verts.astype(dtype), faces, RT[:, 0], K, seed=7)
    cand_valid = np.ones((n, C), dtype=bool)
    if C > 1:
        cand_valid[0, 0] = False                                           # the perfect candidate of instance 0 is ruled out
    return dict(verts=verts.astype(dtype), faces=faces, RT=RT, depth=depth if dper else depth[0], K=K, window=window, delta=0.01,
                near=NEAR, front_weight=0.25, min_px=16, cand_valid=cand_valid)


MIXED = ("n3 C5 f32 K,depth per instance", "n3 C5 f64 K,depth shared", "n1 C1 f32 whole frame", "n1 C5 f64 whole frame", BIG_LATE)

# ---- the exact edges of the rule ------------------------------------------------------------------------------------------------
EDGE_VALUES = np.array([1.0, 1.0 + DELTA_EDGE, np.nextafter(np.float32(1.0 + DELTA_EDGE), np.float32(2)),
                        1.0 - DELTA_EDGE, np.nextafter(np.float32(1.0 - DELTA_EDGE), np.float32(0)), 0.0, -1.0, np.nan], dtype=np.float32)
#                     AGREE q 0, AGREE q 256, BEHIND, AGREE q 256, FRONT, NODEPTH, NODEPTH, NODEPTH


def edge_case(dtype=np.float32):
    """A fronto-parallel triangle at z = 1 under the identity (it renders exactly 1.0f); column x of the observed depth holds
    EDGE_VALUES[x % 8]."""
    verts = np.array([[-0.25, -0.2, 1.0], [0.27, -0.22, 1.0], [0.01, 0.24, 1.0]], dtype=dtype)
    faces = np.array([[0, 1, 2]], dtype=np.int32)
    RT = pose(np.eye(3), np.zeros(3))[None, None]
    depth = np.tile(EDGE_VALUES[np.arange(W) % 8][None, :], (H, 1))
    return dict(verts=verts, faces=faces, RT=RT, depth=depth, K=K0, window=None, delta=DELTA_EDGE, near=NEAR, front_weight=0.25,
                min_px=16, cand_valid=None)


def edge_expected(case):
    """counts i32[6] of edge_case from the covered pixels alone."""
    cov = evaluation.render_depth_numpy(case["verts"], case["faces"], case["RT"][0], case["K"], H, W, NEAR)[0]
    assert set(np.unique(cov).tolist()) == {0.0, 1.0}
    per = np.array([(cov[:, k::8] == 1.0).sum() for k in range(8)])
    return np.array([per.sum(), per[0] + per[1] + per[3], per[4], per[2], per[5] + per[6] + per[7], 256 * (per[1] + per[3])], dtype=np.int32)


# ---- ranking: the true pose, 3 mm off along z, flipped ----------------------------------------------------------------------------
RANK_DELTA = 0.006
RANK_NAMES = ("true", "shifted", "flipped")


@functools.lru_cache(maxsize=None)
def ranking_case():
    """demo_mesh(level=2) at a true pose, seen unoccluded (instance 0) and with a quad at z = 0.3 over the left half of it (instance
    1), a flat background at 1.2 behind.  Candidates: the true pose, the true pose 3 mm farther along z, the true pose turned by 180
    degrees about the camera's y axis through the object centre."""
    m = render.demo_mesh(level=2, seed=2)
    verts, faces = m["verts"].astype(np.float32), m["faces"]
    R, t = rot(0.7, (0.3, 1.0, 0.2)), np.array([0.004, -0.003, 0.5])
    true = pose(R, t)
    shifted = pose(R, t + np.array([0.0, 0.0, 0.003]))
    flipped = pose(rot(np.pi, (0, 1, 0)).dot(R), t)
    clean = evaluation.render_depth_numpy(verts, faces, true[None], K0, H, W, NEAR)[0]
    obs = np.where(clean > 0, clean, np.float32(1.2)).astype(np.float32)
    xs = np.where((clean > 0).any(axis=0))[0]
    mid = int((xs.min() + xs.max()) // 2)
    occluded = obs.copy()
    occluded[:, :mid + 1] = 0.3
    RT = np.tile(np.stack([true, shifted, flipped])[None], (2, 1, 1, 1))
    return dict(verts=verts, faces=faces, RT=RT, depth=np.stack([obs, occluded]), K=K0, window=None, delta=RANK_DELTA, near=NEAR,
                front_weight=0.25, min_px=16, cand_valid=None)


def call_args(case):
    """(positional, keyword) arguments of verify_poses / verify_poses_numpy for a case dict."""
    kw = {k: case[k] for k in ("window", "delta", "near", "front_weight", "min_px", "cand_valid")}
    return (case["verts"], case["faces"], case["RT"], case["depth"], case["K"]), kw
