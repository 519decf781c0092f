"""Shared by tests/test_icp_plane_cpu.py and tests/test_gpu_icp_plane.py: seeded inputs for point-to-plane ICP.  numpy
only; nothing here imports the HIP library.

The model is an ellipsoid with unequal radii (10 / 6 / 3.5 cm): M vertices on a golden-angle spiral with their analytic unit normals,
both rounded to fp32.  The scene points are NOT posed vertices -- that input cannot tell point-to-point from point-to-plane.  They are
drawn on the continuous surface of the camera-facing half (n_z < -0.1 in the camera frame) with 1 mm of isotropic noise, and carry
their analytic normals in rows 6..8.  RT0 is the planted pose turned by 5-20 degrees about the object and moved 1 cm.

Two degenerate models: the exact plane patch (all normals equal: no noise or pose makes it well-posed) and the exact sphere.  The
sphere is degenerate only where every query lies on the normal through its vertex, so its scene points are posed vertices moved ALONG
their normals and its start is the planted pose: a tangential offset from the vertex (a surface sample between vertices, or a wrong
start) makes the vertex-plane residual depend on the rotation -- spuriously, at the scale of the vertex spacing -- and the pivot test,
rightly for the sums it is given, lets it pass."""
import numpy as np

RADII = (0.10, 0.06, 0.035)
NOISE = 0.001
# the seeds of the accuracy claim (5 plane iterations against 20 point iterations), six at each shape
SEEDS_SMALL = (1, 2, 3, 4, 5, 6)            # M = 512, N = 257
SEEDS_LARGE = (11, 12, 13, 14, 15, 16)      # M = 8192, N = 2048
GATE, REJECT, HUBER = 0.5, 0.03, 0.002      # the option values of the accuracy cases: cosine, metres, metres


def spiral_dirs(M):
    """M unit vectors on a golden-angle spiral."""
    k = np.arange(M) + 0.5
    z = 1.0 - 2.0 * k / M
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def axis_angle(axis, ang):
    a = unit(np.asarray(axis, np.float64))
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(ang) * K + (1.0 - np.cos(ang)) * (K @ K)


def rand_rot(rs):
    q, _ = np.linalg.qr(rs.randn(3, 3))
    return q * np.sign(np.linalg.det(q))


def model_of(kind, M, radii=RADII):
    """-> xyz f32[M,3], unit normals f32[M,3].  kind: "ellipsoid" | "sphere" (radius 5 cm) | "plane" (16 cm square at z = 0)."""
    u = spiral_dirs(M)
    if kind == "ellipsoid":
        xyz, nrm = u * np.asarray(radii), unit(u / np.asarray(radii))
    elif kind == "sphere":
        xyz, nrm = 0.05 * u, u
    elif kind == "plane":
        rs = np.random.RandomState(7)
        xyz = np.concatenate([(rs.rand(M, 2) - 0.5) * 0.16, np.zeros((M, 1))], axis=1)
        nrm = np.tile([0.0, 0.0, -1.0], (M, 1))
    else:
        raise ValueError(kind)
    return xyz.astype(np.float32), nrm.astype(np.float32)


def _surface(kind, rs, n, radii, model):
    """n points of the continuous surface and their unit normals, model frame, fp64.  The sphere: vertices moved along their normals."""
    if kind == "ellipsoid":
        u = unit(rs.randn(n, 3))
        return u * np.asarray(radii), unit(u / np.asarray(radii))
    if kind == "sphere":
        j = rs.randint(0, len(model[0]), n)
        nrm = model[1][j].astype(np.float64)
        return model[0][j].astype(np.float64) + NOISE * rs.randn(n, 1) * nrm, nrm
    xyz = np.concatenate([(rs.rand(n, 2) - 0.5) * 0.16, NOISE * rs.randn(n, 1)], axis=1)
    return xyz, np.tile([0.0, 0.0, -1.0], (n, 1))


def make_case(kind, M, N, seeds, radii=RADII):
    """One crop per seed.  -> dict model f32[M,3], model_nrm f32[M,3], cld f32[B,9,N] (rows 0..2 xyz, 6..8 unit normals, the rest
    noise), mask u8[B,N] (all ones), RT_gt f64[B,3,4], RT0 f32[B,3,4], valid bool[B]."""
    model = model_of(kind, M, radii)
    B = len(seeds)
    cld = np.zeros((B, 9, N), np.float32)
    RT_gt, RT0 = np.zeros((B, 3, 4)), np.zeros((B, 3, 4), np.float32)
    for b, seed in enumerate(seeds):
        rs = np.random.RandomState(1000 + seed)
        cld[b, 3:6] = rs.rand(3, N)
        R = rand_rot(rs) if kind != "plane" else axis_angle(rs.randn(3), np.deg2rad(20.0))
        t = np.array([0.05 * rs.randn(), 0.05 * rs.randn(), 0.6 + 0.2 * rs.rand()])
        p, n = _surface(kind, rs, 6 * N, radii, model)
        nc = n @ R.T
        front = np.nonzero(nc[:, 2] < -0.1)[0][:N]
        assert len(front) == N
        pc = p[front] @ R.T + t
        if kind == "ellipsoid":
            pc = pc + NOISE * rs.randn(N, 3)
        cld[b, :3], cld[b, 6:9] = pc.T, nc[front].T
        RT_gt[b] = np.concatenate([R, t[:, None]], axis=1)
        if kind == "sphere":
            RT0[b] = RT_gt[b]
        else:
            deg = 5.0 + 15.0 * rs.rand()
            RT0[b, :, :3] = axis_angle(rs.randn(3), np.deg2rad(deg)) @ R
            RT0[b, :, 3] = t + 0.01 * unit(rs.randn(3))
    return dict(model=model[0], model_nrm=model[1], cld=cld, mask=np.ones((B, N), np.uint8), RT_gt=RT_gt, RT0=RT0,
                valid=np.ones(B, bool))


def partial_mask(N, seed, frac=0.7):
    """A mask that selects about `frac` of the points with the bytes 1, 2 and 255."""
    rs = np.random.RandomState(seed)
    m = np.zeros(N, np.uint8)
    sel = rs.rand(N) < frac
    m[sel] = np.array([1, 2, 255], np.uint8)[rs.randint(0, 3, int(sel.sum()))]
    return m


def add_error(RT_a, RT_b, model):
    """ADD: the mean distance of the model vertices under the two poses [3,4]."""
    v = np.asarray(model, np.float64)
    a, b = np.asarray(RT_a, np.float64), np.asarray(RT_b, np.float64)
    return float(np.linalg.norm((v @ a[:, :3].T + a[:, 3]) - (v @ b[:, :3].T + b[:, 3]), axis=1).mean())


def scene_of(case, b):
    """-> scene f64[N,3], scene normals f64[N,3] of crop b."""
    return case["cld"][b, :3].T.astype(np.float64), case["cld"][b, 6:9].T.astype(np.float64)


def point_icp(scene, model, RT0, iters=20):
    """Point-to-point ICP in fp64 (oracle.pose_ref.icp_step, the restatement refine_icp is pinned to), `iters` iterations with no
    stop rule -> RT [3,4]."""
    from oracle import pose_ref
    RT = np.asarray(RT0, np.float64)
    m = np.asarray(model, np.float64)
    for _ in range(iters):
        RT = pose_ref.icp_step(scene, m, RT)["RT"]
    return RT


# ---- the single-iteration accuracy cases of the GPU test: every (B, N, M), with no option and with all three ----
ONE_ITER_SHAPES = [(B, N, M) for B in (1, 3) for N in (33, 63, 64, 65, 255, 256, 257, 515) for M in (64, 512)]
OPTIONS = {"plain": dict(reject_dist=None, normal_gate=None, huber=None),
           "all": dict(reject_dist=REJECT, normal_gate=GATE, huber=HUBER)}
WHOLE_RUN_SEEDS = (4, 5, 6)                  # the free-running case: M = 512, N = 257, B = 3
PRODUCT_SEEDS = tuple(range(11, 27))         # the product shape: M = 8192, N = 2048, B = 16


def one_iteration_case(B, N, M, opt):
    """The inputs of one single-iteration case: make_case on seeds derived from the shape, crop b masked by partial_mask when N + b is
    odd, and as the start of crop b the fp32 pose after (N + M // 64 + b) % 3 free iterations of the restatement with the same
    options (so the step under test is the first, second or third of a run).  -> the case dict with RT_start f32[B,3,4] added."""
    from geometric_aware_dense_matching_amd import pose
    case = make_case("ellipsoid", M, N, [N + M + 7 * b for b in range(B)])
    case["RT_start"] = case["RT0"].copy()
    for b in range(B):
        if (N + b) % 2:
            case["mask"][b] = partial_mask(N, N + b)
        sc, sn = scene_of(case, b)
        k = (N + M // 64 + b) % 3
        if k:
            run = pose.icp_plane_numpy(sc, sn, case["model"], case["model_nrm"], case["RT0"][b], case["mask"][b], iters=k, tolerance=0.0,
                                       **OPTIONS[opt])
            case["RT_start"][b] = run["RT"].astype(np.float32)
    return case
