"""ORACLE -- test infrastructure only; never imported by the product package.

Seeded inputs for the pose-stage tests (tests/test_pose_fit_cpu.py, tests/test_gpu_pose_shapes.py): the geometry families the
pose-fit fragment is checked on, and the product-shape RANSAC and ICP batches.  numpy only."""
import numpy as np

EXTENT = np.array([0.2, 0.12, 0.07])                 # an object-sized, anisotropic cloud (m)
T0 = np.array([0.03, -0.02, 0.8])

UNIQUE = ("generic", "identity", "identity_t", "half_axis", "half_random", "near_half", "planar", "planar_noise", "mirrored", "mm",
          "far", "tiny", "dup3")
AMBIGUOUS = ("collinear", "dup2", "dup1", "dup3_any")  # no unique rotation: only the invariants and the objective are checked
FAMILIES = UNIQUE + AMBIGUOUS
SIZES = (5, 6, 17, 200, 2048)


def rand_rot(rs, K):
    q, r = np.linalg.qr(rs.randn(K, 3, 3))
    q = q * np.sign(np.einsum("kii->ki", r))[:, None, :]
    return q * np.linalg.det(q)[:, None, None]


def axis_angle(ax, th):
    ax = ax / np.linalg.norm(ax, axis=-1, keepdims=True)
    Kx = np.zeros(ax.shape[:-1] + (3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -ax[..., 2], ax[..., 1], ax[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -ax[..., 0], -ax[..., 1], ax[..., 0]
    th = np.asarray(th)[..., None, None]
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def family(name, rs, K, n):
    """K cases of n pairs -> A (model points), B (scene points) f32[K,n,3].  dup* ignore n: they are 4-point samples drawn with
    replacement that hold 3, 2 and 1 distinct pairs.  The three points of dup3 are a triangle built with corners 120 +- 29 degrees
    apart at 3-8 cm from its centre, so that its rotation is well determined by construction; dup3_any takes any three points
    (among 2000 such triples some are collinear to 1e-4 of their extent, and their rotation is not pinned)."""
    if name.startswith("dup"):
        n = 4
    A = (rs.rand(K, n, 3) - 0.5) * EXTENT
    R = rand_rot(rs, K)
    t = T0 + 0.05 * rs.randn(K, 3)
    noise, unit = 0.001, 1.0
    if name in ("identity", "identity_t"):
        R = np.broadcast_to(np.eye(3), (K, 3, 3))
        noise = 0.0
        if name == "identity":
            t = np.zeros((K, 3))
    elif name == "half_axis":
        d = np.array([[1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)[np.arange(K) % 3]
        R = d[:, :, None] * np.eye(3)
        noise = 0.0
    elif name == "half_random":
        ax = rs.randn(K, 3)
        ax /= np.linalg.norm(ax, axis=1, keepdims=True)
        R = 2 * ax[:, :, None] * ax[:, None, :] - np.eye(3)
        noise = 0.0
    elif name == "near_half":
        R = axis_angle(rs.randn(K, 3), np.pi - rs.uniform(-1e-4, 1e-4, K))
    elif name in ("planar", "planar_noise"):
        A[:, :, 2] = 0.0
        noise = 0.0 if name == "planar" else 0.001
    elif name == "collinear":
        A = A[:, :1] + (rs.rand(K, n, 1) - 0.5) * 0.2 * rand_rot(rs, K)[:, :1, :]
        noise = 0.0
    elif name == "mm":
        unit = 1000.0
    elif name == "far":
        t = 1000.0 * rand_rot(rs, K)[:, 0]
    elif name == "tiny":
        unit = 1e-5
    elif name in ("dup3", "dup3_any"):
        if name == "dup3":
            ang = np.array([0.0, 2.0, 4.0]) * np.pi / 3 + rs.uniform(-0.5, 0.5, (K, 3))
            tri = rs.uniform(0.03, 0.08, (K, 3, 1)) * np.stack([np.cos(ang), np.sin(ang), np.zeros_like(ang)], axis=2)
            A[:, :3] = np.einsum("kij,knj->kni", rand_rot(rs, K), tri) + A[:, 3:]
        A[:, 3] = A[:, 1]
    elif name == "dup2":
        A[:, 2], A[:, 3] = A[:, 0], A[:, 1]
    elif name == "dup1":
        A[:] = A[:, :1]
    src = A * np.array([1.0, 1.0, -1.0]) if name == "mirrored" else A
    B = np.einsum("kij,knj->kni", R, src) + t[:, None] + noise * rs.randn(K, n, 3)
    if name in ("dup3", "dup3_any"):
        B[:, 3] = B[:, 1]
    elif name == "dup2":
        B[:, 2], B[:, 3] = B[:, 0], B[:, 1]
    elif name == "dup1":
        B[:] = B[:, :1]
    return (A * unit).astype(np.float32), (B * unit).astype(np.float32)


# ---- RANSAC at the product shape ---------------------------------------------------------------------------------------------------
RANSAC_N, RANSAC_M = 2048, 8192
RANSAC_COUNTS = (2048, 2047, 1793, 1025, 1024, 513, 257, 256, 255, 65, 64, 63, 6, 5, 4, 0)
RANSAC_OUTLIERS = (0.0, 0.1, 0.25, 0.4, 0.45, 1.0, 0.5, 0.6, 0.3, 0.2, 0.4, 0.0, 0.0, 0.2, 0.0, 0.0)     # 1.0: no consistent pose at all
MATCH_ERR, FIX_PERCENT = 0.015, 0.7


def ransac_case(data_seed, counts=RANSAC_COUNTS, outliers=RANSAC_OUTLIERS, N=RANSAC_N, M=RANSAC_M):
    """-> dict model f32[M,3], idx i32[B,N], mask u8[B,N] (counts[b] selected points at random positions; the selected bytes are 1,
    2 or 255), cld f32[B,9,N].  Selected pairs: the model posed + 1 mm noise, a share outliers[b] of them thrown 0.05-0.3 m off."""
    rs = np.random.RandomState(data_seed)
    B = len(counts)
    model = ((rs.rand(M, 3) - 0.5) * EXTENT).astype(np.float32)
    idx = rs.randint(0, M, size=(B, N)).astype(np.int32)
    mask = np.zeros((B, N), np.uint8)
    cld = rs.rand(B, 9, N).astype(np.float32)
    R = rand_rot(rs, B)
    for b in range(B):
        t = T0 + np.array([0.03 * b, 0.0, 0.0])
        pts = model[idx[b]].astype(np.float64) @ R[b].T + t + 0.001 * rs.randn(N, 3)
        sel = np.sort(rs.choice(N, counts[b], replace=False))
        mask[b, sel] = np.array([1, 2, 255], np.uint8)[rs.randint(0, 3, len(sel))]
        if outliers[b] >= 1.0:
            pts = rs.rand(N, 3) * 20.0 - 10.0 + np.array([0.0, 0.0, 12.0])
        else:
            bad = sel[rs.rand(len(sel)) < outliers[b]]
            pts[bad] += (0.08 + 0.2 * rs.rand(len(bad), 1)) * rs.randn(len(bad), 3) / 1.7
        cld[b, :3] = pts.T.astype(np.float32)
    return dict(model=model, idx=idx, mask=mask, cld=cld)


def selected_pairs(case, b):
    """The crop's selected pairs in point order, f64: A = matched model vertices, B = scene points."""
    sel = case["mask"][b] != 0
    M = case["model"].shape[0]
    j = np.clip(case["idx"][b][sel].astype(np.int64), 0, M - 1)
    return case["model"][j].astype(np.float64), case["cld"][b, :3][:, sel].T.astype(np.float64)


def decision_pinned(counts, near, degenerate, n, fix_percent):
    """Whether the reference's rule gives the same (winner, refit) for every count vector within +-near of `counts` on the
    non-degenerate hypotheses (the degenerate ones are taken as given)."""
    counts = np.asarray(counts, np.int64)
    near = np.where(degenerate, 0, near)
    lo, hi = counts - near, counts + near
    lim = fix_percent * n
    over = np.nonzero(counts > lim)[0]
    if len(over):
        w = over[0]
        return bool(lo[w] > lim and (hi[:w] <= lim).all())
    if (hi > lim).any():
        return False
    if counts.max() <= 0:
        return bool((hi <= 0).all())
    w = int(np.argmax(counts))
    return bool(lo[w] > 0 and (hi[:w] < lo[w]).all() and (hi[w + 1:] <= lo[w]).all())


# ---- ICP at the product shape ------------------------------------------------------------------------------------------------------
ICP_SELECTED = (2048, 2048, 1500, 1000, 600, 300, 100, 64, 20, 14, 12, 10, 9, 8, 3, 700)
ICP_INVALID = 15                                     # this crop comes with valid = 0
ICP_STARVED = 14                                     # and this one with fewer than min_points selected points


def icp_case(data_seed, selected=ICP_SELECTED, N=2048, M=8192):
    """-> dict model f32[M,3], cld f32[B,9,N] (model vertices posed + 1 mm noise, in no particular order), mask u8[B,N]
    (selected[b] points at random positions), RT0 f32[B,3,4] (the true pose turned 5-20 degrees and moved 1-3 cm; for the crops
    with 20 or fewer selected points 30 degrees and 5 mm, a start from which the few pairs within a rejection distance come and go
    from one iteration to the next), valid bool[B]."""
    rs = np.random.RandomState(data_seed)
    B = len(selected)
    model = ((rs.rand(M, 3) - 0.5) * EXTENT).astype(np.float32)
    cld = rs.rand(B, 9, N).astype(np.float32)
    mask = np.zeros((B, N), np.uint8)
    RT0 = np.zeros((B, 3, 4), np.float32)
    R = rand_rot(rs, B)
    for b in range(B):
        t = T0 + np.array([0.0, 0.02 * b, 0.0])
        v = model[rs.choice(M, N, replace=False)].astype(np.float64)
        cld[b, :3] = (v @ R[b].T + t + 0.001 * rs.randn(N, 3)).T.astype(np.float32)
        mask[b, rs.choice(N, selected[b], replace=False)] = 1
        dt = rs.randn(3)
        deg, shift = (30.0, 0.005) if selected[b] <= 20 else (5.0 + 5.0 * (b % 4), 0.01 + 0.01 * (b % 3))
        RT0[b, :, :3] = axis_angle(rs.randn(3), np.deg2rad(deg)) @ R[b]
        RT0[b, :, 3] = t + shift * dt / np.linalg.norm(dt)
    valid = np.ones(B, bool)
    valid[ICP_INVALID] = False
    return dict(model=model, cld=cld, mask=mask, RT0=RT0, valid=valid)
