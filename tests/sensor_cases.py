"""Depth frames for the depth sensor tests (tests/test_depth_sensor_cpu.py, tests/test_gpu_depth_sensor.py), built in numpy: no
renderer is needed, THE SENSOR RULE of include/gdm.h is a function of the depth frame alone.  Every case is f32[2,H,W] in metres and
clips itself to the frame, so it can be asked for at any size."""
import numpy as np

BACK, FRONT = 1.0, 0.5


def make_K(fx, fy=None, cx=None, cy=None, H=1, W=1):
    fy = fx if fy is None else fy
    cx = 0.5 * (W - 1) if cx is None else cx
    cy = 0.5 * (H - 1) if cy is None else cy
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32)


def _plane(H, W, z=BACK):
    return np.full((2, H, W), z, dtype=np.float32)


def _box(d, b, r0, r1, c0, c1, z=FRONT):
    H, W = d.shape[1:]
    d[b, max(r0, 0):max(min(r1, H), 0), max(c0, 0):max(min(c1, W), 0)] = z


def box_scene(H, W, c0=None, c1=None):
    """A back plane at 1.0 m with a box at 0.5 m in front (columns c0 .. c1-1, the middle third by default; all rows in frame 0, the
    lower rows in frame 1)."""
    d = _plane(H, W)
    c0 = W // 3 if c0 is None else c0
    c1 = max(2 * W // 3, c0 + 1) if c1 is None else c1
    _box(d, 0, 0, H, c0, c1)
    _box(d, 1, H // 2, H, c0, c1)
    return d


def tilted_plane(H, W, K, degrees, z0=BACK):
    """A plane through (0, 0, z0) tilted by `degrees` about the vertical axis, the same in both frames: z = z0 / (1 - u tan(a)) along
    the ray (u, v, 1); no depth where that is not positive."""
    K = np.asarray(K, dtype=np.float64)
    u = (np.arange(W, dtype=np.float64) - K[0, 2]) / K[0, 0]
    den = 1.0 - u * np.tan(np.deg2rad(float(degrees)))
    z = np.where(den > 1e-3, z0 / np.maximum(den, 1e-3), 0.0)
    return np.broadcast_to(z[None, None, :], (2, H, W)).astype(np.float32).copy()


def invalid_frame(H, W):
    """A plane at 1.0 m with zeros, negatives, NaN, a region nearer than any z_min in use (0.1 m) and one farther than z_max (9 m),
    at other places in the two frames."""
    d = _plane(H, W)
    for b in range(2):
        s = 3 * b
        _box(d, b, 0, H // 2, s + 2, s + 6, 0.0)
        _box(d, b, H // 3, H, s + 9, s + 12, -1.0)
        _box(d, b, 1, H - 1, s + 15, s + 17, np.nan)
        _box(d, b, 0, H, W // 2 + s, W // 2 + s + 9, 0.1)
        _box(d, b, H // 2, H, W - 20 - s, W - 8 - s, 9.0)
        _box(d, b, 0, 2, W - 6, W, np.inf)
    return d


def shadow_across_tiles(H, W, tile_w, tile_h):
    """Occluders whose shadows cross a tile boundary: one starting 3 columns right of the first vertical boundary (a positive baseline
    throws its shadow left, over the boundary), one ending 5 columns left of the second (a negative baseline throws it right), in rows
    that straddle the first horizontal boundary."""
    d = _plane(H, W)
    for b in range(2):
        _box(d, b, tile_h - 3 - b, tile_h + 2, tile_w + 3, tile_w + 40 + b)
        _box(d, b, tile_h - 2, H, 2 * tile_w - 30 - b, 2 * tile_w - 5)
    return d


def shadow_leaves_frame(H, W):
    """Occluders at the left and the right edge of the frame: the shadow of one of them leaves the frame whatever the baseline's
    sign."""
    d = _plane(H, W)
    for b in range(2):
        _box(d, b, 0, H - b, 2, min(20, W // 2))
        _box(d, b, b, H, max(W - 20, W // 2 + 1), W - 1)
    return d


def mixed(H, W, seed=0):
    """Boxes at hash-free pseudo-random places and depths over a slightly sloped back plane, with a few invalid pixels: the case for
    sizes too small for the others."""
    rs = np.random.RandomState(seed)
    d = _plane(H, W) + np.linspace(0.0, 0.3, W, dtype=np.float32)[None, None, :]
    for b in range(2):
        for _ in range(4):
            r0, c0 = rs.randint(0, H), rs.randint(0, W)
            _box(d, b, r0, r0 + rs.randint(1, 6), c0, c0 + rs.randint(1, 30), float(rs.uniform(0.3, 1.2)))
        for _ in range(3):
            d[b, rs.randint(0, H), rs.randint(0, W)] = rs.choice([0.0, -2.0, np.nan, 7.0])
    return d.astype(np.float32)


def all_cases(H, W, K, tile_w, tile_h):
    """name -> f32[2,H,W], every case of this module at one size."""
    return {"box": box_scene(H, W), "tilted-30": tilted_plane(H, W, K, 30.0), "tilted-80": tilted_plane(H, W, K, 80.0),
            "tilted-89.5": tilted_plane(H, W, K, 89.5), "invalid": invalid_frame(H, W),
            "shadow-across-tiles": shadow_across_tiles(H, W, tile_w, tile_h), "shadow-leaves-frame": shadow_leaves_frame(H, W),
            "mixed": mixed(H, W, 1)}
