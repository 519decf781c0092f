"""Seeded inputs for the two-way matching and cycle-filter tests (CPU and GPU): every seed is zlib.crc32 of the case's name.

  SHAPES / MASKS         the launch shapes and mask kinds of tests/test_gpu_match_twoway.py
  descriptors(...)       scene f32[B,128,N], model f32[128,M]
  mask(...)              u8[B,N] of one of the MASKS
  planted_rows(...)      scene rows that copy model columns, for the planted-winner test
  cycle_case(...)        xyz / best_idx / col_idx / mask with an out-of-range best_idx and a NaN coordinate
  filter_case(...)       the planted inlier / outlier scene of the filter test (B = 2, N = 256, M = 512, or scaled)
"""
import zlib

import numpy as np

SHAPES = [(2, 70, 200), (1, 256, 256), (3, 128, 8193), (2, 300, 513)]
# beyond the issue's four: five crops inside one row block of 256 (crops past the kernel's LDS slots) and a crop shorter than a wave tile
EXTRA_SHAPES = [(5, 40, 100), (9, 20, 64)]
MASKS = ["random", "ones", "empty_crop", "single_row"]


def rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


def descriptors(B, N, M, name="random"):
    rs = rng("match_twoway desc %d %d %d %s" % (B, N, M, name))
    scene = (rs.randn(B, 128, N) * rs.rand(B, 1, N) * 3).astype(np.float32)
    model = rs.randn(128, M).astype(np.float32)
    return scene, model


def mask(B, N, kind):
    rs = rng("match_twoway mask %d %d %s" % (B, N, kind))
    if kind == "random":
        return (rs.rand(B, N) < 0.6).astype(np.uint8)
    if kind == "ones":
        return np.ones((B, N), np.uint8)
    m = (rs.rand(B, N) < 0.6).astype(np.uint8)
    b = B - 1                                                  # the last crop: behind the crop boundary of a shared row block
    m[b] = 0
    if kind == "single_row":
        m[b, rs.randint(N)] = 1
    else:
        assert kind == "empty_crop", kind
    return m


def planted_rows(model, B, N):
    """Scene row r (counted over the whole batch) = model column r mod M, exactly: scene f32[B,128,N]."""
    M = model.shape[1]
    cols = np.arange(B * N) % M
    return np.ascontiguousarray(model[:, cols].reshape(128, B, N).transpose(1, 0, 2)), cols


def cycle_case(B, N, M):
    """A [B,9,N] cloud (rows 0-2 = xyz within a 10 cm cube), best_idx with one entry out of range on either side, a col_idx that
    points back to the point itself, to a near point, to a far point or nowhere (-1), a mask, and one NaN coordinate."""
    rs = rng("match_cycle %d %d %d" % (B, N, M))
    cld = rs.uniform(-0.05, 0.05, (B, 9, N)).astype(np.float32)
    best_idx = rs.randint(0, M, (B, N)).astype(np.int32)
    col_idx = rs.randint(0, N, (B, M)).astype(np.int32)
    for b in range(B):
        for i in range(N):
            kind = rs.randint(4)
            j = best_idx[b, i]
            if kind == 0:
                col_idx[b, j] = i                              # mutual
            elif kind == 1 and N > 1:                          # a neighbour 1 to 4 mm away
                k = (i + 1) % N
                cld[b, :3, k] = cld[b, :3, i] + rs.uniform(-1, 1, 3).astype(np.float32) * np.float32(0.003)
                col_idx[b, j] = k
            elif kind == 2:
                col_idx[b, j] = -1
    msk = (rs.rand(B, N) < 0.7).astype(np.uint8)
    msk[0, 0] = 1
    best_idx[0, 0] = M                                         # out of range above
    if N > 2:
        msk[B - 1, 1] = msk[B - 1, 2] = 1
        best_idx[B - 1, 1] = -3                                # and below
        cld[B - 1, 1, 2] = np.nan                              # a NaN y of a masked point that its own vertex picks back
        col_idx[B - 1, best_idx[B - 1, 2]] = 2
    return cld, best_idx, col_idx, msk


def _unit(x, axis):
    return x / np.linalg.norm(x, axis=axis, keepdims=True)


FILTER_SEED = "match_twoway filter 0"


def filter_case(B=2, N=256, M=512, name=FILTER_SEED):
    """Random model descriptors [128,M] and vertices in a 20 cm cube; per crop a rigid RT.  Three quarters of the points are inliers:
    point i carries the descriptor of its own distinct vertex j exactly and lies at RT x_j.  A quarter are outliers: each carries
    normalize(d_j + 0.3 u) (u a random unit vector) for the vertex j of some inlier of its crop and lies more than 5 cm from that
    inlier.  -> dict(scene f32[B,128,N], model f32[128,M], model_xyz f32[M,3], cld f32[B,9,N], inlier u8[B,N], RT f32[B,3,4])."""
    rs = rng(name)
    model = _unit(rs.randn(128, M), 0).astype(np.float32)
    xyz = rs.uniform(-0.1, 0.1, (M, 3)).astype(np.float32)
    n_out = N // 4
    scene = np.zeros((B, 128, N), np.float32)
    cld = np.zeros((B, 9, N), np.float32)
    inlier = np.ones((B, N), np.uint8)
    RT = np.zeros((B, 3, 4), np.float32)
    for b in range(B):
        q, _ = np.linalg.qr(rs.randn(3, 3))
        q = q * np.sign(np.linalg.det(q))
        RT[b, :, :3], RT[b, :, 3] = q, rs.uniform(-0.2, 0.2, 3) + np.array([0, 0, 0.8])
        out = np.sort(rs.choice(N, n_out, replace=False))
        inlier[b, out] = 0
        inl = np.flatnonzero(inlier[b])
        vert = rs.choice(M, len(inl), replace=False)             # one distinct vertex per inlier
        scene[b][:, inl] = model[:, vert]
        pts = xyz[vert].astype(np.float64) @ RT[b, :, :3].astype(np.float64).T + RT[b, :, 3]
        cld[b, :3, inl] = pts.astype(np.float32)
        for i in out:
            a = rs.randint(len(inl))                           # the inlier whose vertex this outlier claims
            d = model[:, vert[a]].astype(np.float64) + 0.3 * _unit(rs.randn(128), 0)
            scene[b][:, i] = _unit(d, 0).astype(np.float32)
            while True:
                p = pts[a] + rs.uniform(-0.15, 0.15, 3)
                if np.linalg.norm(p - pts[a]) > 0.05:
                    break
            cld[b, :3, i] = p.astype(np.float32)
        cld[b, 3:] = rs.rand(6, N).astype(np.float32)
    return dict(scene=scene, model=model, model_xyz=xyz, cld=cld, inlier=inlier, RT=RT)
