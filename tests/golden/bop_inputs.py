"""The small scene shared by make_golden_bop.py, tests/test_bop_errors_cpu.py and tests/test_gpu_bop_errors.py: a squashed icosphere,
a ground-truth pose, three estimates, a 61 x 45 camera and a test depth image with an occluder and a band of missing depth.  Pure numpy,
seeded; nothing here is read from anywhere."""
import numpy as np

H, W = 45, 61                                                         # no multiple of any tile
K = np.array([[70.0, 0.0, 29.3], [0.0, 70.0, 22.1], [0.0, 0.0, 1.0]])
NEAR = 0.01
DELTA = 0.015
TAUS = [round(0.05 * i, 2) for i in range(1, 11)]
LM_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])

MODEL_INFOS = {                                                        # models_info.json entries (mm)
    "none": {"diameter": 100.0},
    "discrete": {"diameter": 100.0, "symmetries_discrete": [[-1.0, 0.0, 0.0, 3.0, 0.0, -1.0, 0.0, -2.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]]},
    "continuous": {"diameter": 100.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [1.5, -2.0, 0.5]}]},
    "both": {"diameter": 100.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}],
             "symmetries_discrete": [[1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 4.0, 0.0, 0.0, 0.0, 1.0]]},
}
SYM_CASES = ("none", "discrete", "continuous", "both")                # S = 1, 2, 314, 628


def rot(angle, axis):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def icosphere(subdivisions=2, radius=0.05):
    """162 vertices / 320 faces at 2 subdivisions."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    v = [np.asarray(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v) * radius, np.asarray(f, dtype=np.int32)


def mesh():
    """The icosphere of radius 0.05 scaled x1.6 in x and x0.7 in z: front and back faces overlap in every view."""
    v, f = icosphere(2, 0.05)
    return v * np.array([1.6, 1.0, 0.7]), f


def diameter(verts):
    d = verts[:, None, :] - verts[None, :, :]
    return float(np.sqrt((d * d).sum(-1)).max())


def poses():
    """RT_gt f64[3,3,4] (the same ground truth three times) and RT_est f64[3,3,4]: near, far, clipped."""
    Rg, tg = rot(0.7, (1, 2, 3)), np.array([0.01, -0.005, 0.35])
    est = [(rot(0.05, (0, 1, 0)) @ Rg, tg + np.array([0.002, 0.001, 0.004])),
           (rot(0.6, (1, 0, 0)) @ Rg, tg + np.array([0.02, -0.01, 0.03])),
           (Rg, tg + np.array([0.16, 0.0, 0.0]))]
    RT_gt = np.stack([np.hstack([Rg, tg[:, None]])] * 3)
    RT_est = np.stack([np.hstack([R, t[:, None]]) for R, t in est])
    return RT_est, RT_gt


def make_test_depth(depth_gt):
    """The ground-truth render + 4 mm on the object and 0.6 elsewhere; the object pixels of columns 0-21 brought 50 mm nearer (an
    occluder); rows 10-13 set to 0 (missing depth)."""
    obj = depth_gt > 0
    d = np.where(obj, depth_gt + np.float32(0.004), np.float32(0.6)).astype(np.float32)
    occ = obj.copy()
    occ[:, 22:] = False
    d[occ] -= np.float32(0.05)
    d[10:14, :] = 0.0
    return d


def full_quad(z=0.5, margin=2.0):
    """Two triangles that cover the whole H x W image at constant depth z (in camera coordinates: RT = identity)."""
    def back(u, v):
        return [(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z]
    verts = np.array([back(-margin, -margin), back(W - 1 + margin, -margin), back(W - 1 + margin, H - 1 + margin),
                      back(-margin, H - 1 + margin)])
    return verts, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


def identity_pose(n=1):
    return np.stack([np.hstack([np.eye(3), np.zeros((3, 1))])] * n)


def mssd_inputs(M=1000, n=5, seed=11):
    """pts f64[M,3] (metres, an elongated cloud), RT_est / RT_gt f64[n,3,4]: the estimates 2-40 degrees and 2-40 mm off."""
    rs = np.random.RandomState(seed)
    pts = (rs.rand(M, 3) - 0.5) * np.array([0.12, 0.08, 0.2])
    RT_est, RT_gt = np.zeros((n, 3, 4)), np.zeros((n, 3, 4))
    for i in range(n):
        Rg = rot(rs.rand() * 3.0, rs.randn(3))
        tg = np.array([0.1 * rs.randn(), 0.1 * rs.randn(), 0.6 + 0.4 * rs.rand()])
        Re = rot(0.035 * (1 + 4 * i), rs.randn(3)) @ Rg
        te = tg + 0.002 * (1 + 4 * i) * rs.randn(3)
        RT_gt[i], RT_est[i] = np.hstack([Rg, tg[:, None]]), np.hstack([Re, te[:, None]])
    return pts, RT_est, RT_gt
