"""Named, seeded kNN inputs on which a pruned search can go wrong without anything faulting: supports far from the origin (a cell
a few ulps wide), neighbours that race a point just beyond a window edge, points exactly on cell edges, one overfull cell,
degenerate axes, the sizes at which the library changes kernel or grid; and organised maps with a wide or off-axis pinhole, a
fronto-parallel wall without noise, holes that race the K-th distance, dead columns and rows, and the smallest and largest grids.

make(name) -> Case.  Every case has B = 3 crops with a DIFFERENT placement each (the per-crop cell boxes and ratio ranges are
indexed by crop), S <= 8192 and Q <= 512, and is seeded by zlib.crc32 of its name.  want(name, K) is the oracle's answer,
computed once per (name, K) and shared by the tests that need it; callers must not write to it.

The generators of edge_race and edge_points take the cell edges from tests/knn_prune_model.py (cells_box, edge): they aim at the
rule as it is restated there.
"""
import functools
import zlib
from dataclasses import dataclass, field

import numpy as np

import knn_prune_model as pm

f32 = np.float32
B = 3
KS = (16, 1, 32)                                            # every case runs with K = 16, and once each with 1 and 32


@dataclass
class Case:
    name: str
    sup: np.ndarray                                         # f32[B,S,3]
    qry: np.ndarray                                         # f32[B,Q,3]
    W: int = 0                                              # grid_w of an organised support, else 0
    degenerate: bool = False                                # an unorganised case whose coverage condition does not apply
    min_pruned: float = 0.5                                 # organised: least fraction of queries with a window below the grid
    info: dict = field(default_factory=dict)                # what a test needs to know about the construction


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()) % (2 ** 31))


def _step(v, n):
    """v moved n float32 values up (n > 0) or down."""
    v = f32(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, f32(np.inf) if n > 0 else f32(-np.inf))
    return v


# three placements: sign pattern of the centre, extent, direction weights (no power of two, so nothing aligns by accident)
_SIGNS = np.array([[1, 1, 1], [-1, 1, -1], [1, -1, 1]], np.float64)
_EXTENT = [1.0, 0.37, 9.7]
_DIRW = np.array([1.0, 0.83, 0.9])


def _centre(b, ratio):
    return _SIGNS[b] * _DIRW * ratio * _EXTENT[b]


def _queries_on_and_beside(rs, sup, Q, beside):
    """Half of the queries ON support points, half beside them (offset `beside` x extent, then rounded with the point)."""
    out = []
    for b in range(B):
        S = sup[b].shape[0]
        pick = rs.randint(0, S, Q)
        q = sup[b][pick].astype(np.float64)
        q[Q // 2:] += rs.randn(Q - Q // 2, 3) * beside * _EXTENT[b]
        out.append(q.astype(f32))
    return np.stack(out)


# ---- unorganised ------------------------------------------------------------------------------------------------------------
def _shape(rs, kind, S):
    """[S,3] float64 in a unit extent around 0."""
    if kind == "sheet":
        xy = rs.rand(S, 2) - 0.5
        z = 0.05 * np.sin(7 * xy[:, :1]) * np.cos(5 * xy[:, 1:])
        return np.concatenate([xy, z], axis=1)
    if kind == "cube":
        return rs.rand(S, 3) - 0.5
    if kind == "clustered":
        c = rs.rand(8, 3) - 0.5
        return c[rs.randint(0, 8, S)] + 0.004 * rs.randn(S, 3)
    if kind == "dups":
        base = rs.rand(S - S // 2, 3) - 0.5
        return np.concatenate([base, base[: S // 2]], axis=0)
    raise KeyError(kind)


def _offset(name):
    _, kind, p = name.split("_")                            # offset_sheet_2p20
    ratio = 2.0 ** int(p[2:])
    rs = _rs(name)
    S, Q = 2048, 200
    sup = np.stack([(_shape(rs, kind, S) * _EXTENT[b] + _centre(b, ratio)).astype(f32) for b in range(B)])
    return Case(name, sup, _queries_on_and_beside(rs, sup, Q, 0.01))


def _sizes(name):
    _, s, kind = name.split("_")                            # sizes_8191_sheet
    S = int(s)
    rs = _rs(name)
    Q = 96 if S > 4096 else 200
    sup = np.stack([(_shape(rs, kind, S) * _EXTENT[b] + _centre(b, 3.0)).astype(f32) for b in range(B)])
    return Case(name, sup, _queries_on_and_beside(rs, sup, Q, 0.01))


def _heavy_cell(name):
    """Half of the support inside ONE cell of the 16 x 16 grid (1024 points: a row of the window has far more than 64 new points),
    the rest spread over the box.  Queries inside the heavy cell, beside it and elsewhere."""
    rs = _rs(name)
    S, Q = 2048, 240
    sup, qry = [], []
    for b in range(B):
        cell = [(5, 9), (0, 15), (15, 0)][b]                # an interior cell, two corner cells
        spread = rs.rand(S // 2, 3) - 0.5
        spread[:4, :2] = [[-0.5, -0.5], [0.5, -0.5], [-0.5, 0.5], [0.5, 0.5]]      # the box does not depend on the draw
        lo = (np.array(cell) + 0.05) / 16 - 0.5
        heavy = np.concatenate([lo + rs.rand(S // 2, 2) * 0.9 / 16, rs.rand(S // 2, 1) * 0.2 - 0.1], axis=1)
        pts = (np.concatenate([spread, heavy]) * _EXTENT[b] + _centre(b, 5.0)).astype(f32)
        pts = pts[rs.permutation(S)]
        sup.append(pts)
        q = np.concatenate([heavy[: Q // 3], heavy[Q // 3: 2 * Q // 3] + rs.randn(Q // 3, 3) * 0.03,
                            rs.rand(Q - 2 * (Q // 3), 3) - 0.5])
        qry.append((q * _EXTENT[b] + _centre(b, 5.0)).astype(f32))
    return Case(name, np.stack(sup), np.stack(qry))


def _line(name):
    """A degenerate axis (every x, or every y, the same float32 value: cell width 0) far from the origin."""
    axis = 0 if name == "line_x" else 1
    rs = _rs(name)
    S, Q = 2048, 200
    sup = np.stack([(_shape(rs, "cube", S) * _EXTENT[b] + _centre(b, 2.0 ** 12)).astype(f32) for b in range(B)])
    for b in range(B):
        sup[b, :, axis] = sup[b, 0, axis]
    qry = _queries_on_and_beside(rs, sup, Q, 0.01)
    return Case(name, sup, qry, degenerate=True)


def _edge_points(name):
    """Support points and queries exactly on the corners, sides and interior edges of the cell grid: f == 0, integer f, f == G
    (the clamp), and the float32 values next to each edge on either side.  S = 1024: the 16 x 16 grid."""
    rs = _rs(name)
    S, G = 1024, 16
    place = [(0.0, 1.0, 0.0, 1.0), (-3.7, 0.9, 5.1, 1.3), (1000.3, 2.7, -777.7, 0.61)]     # xlo, x extent, ylo, y extent
    sup, qry = [], []
    for b in range(B):
        xlo, lx, ylo, ly = (f32(t) for t in place[b])
        xhi, yhi = f32(xlo + lx), f32(ylo + ly)
        cw, ch = f32((xhi - xlo) / f32(G)), f32((yhi - ylo) / f32(G))
        ex = np.minimum(np.append(pm.edge(xlo, np.arange(G), cw), xhi), xhi).astype(f32)   # 17 edges, none beyond the box
        ey = np.minimum(np.append(pm.edge(ylo, np.arange(G), ch), yhi), yhi).astype(f32)
        gx, gy = np.meshgrid(ex, ey)
        lattice = np.stack([gx.ravel(), gy.ravel(), (rs.rand(gx.size) * 0.1).astype(f32)], axis=1).astype(f32)   # 289 points
        near = lattice[rs.randint(0, len(lattice), 300)].copy()                            # one float32 value off an edge
        for p in near:
            p[0] = np.clip(_step(p[0], rs.choice([-1, 1])), xlo, xhi)
            p[1] = np.clip(_step(p[1], rs.choice([-1, 1, 0])), ylo, yhi)
        rest = np.stack([xlo + rs.rand(S - 589) * lx, ylo + rs.rand(S - 589) * ly, rs.rand(S - 589) * 0.1], axis=1).astype(f32)
        rest[:, 0] = np.clip(rest[:, 0], xlo, xhi)
        rest[:, 1] = np.clip(rest[:, 1], ylo, yhi)
        pts = np.concatenate([lattice, near, rest])[rs.permutation(S)]
        assert pm.cells_box(pts, G)[:4] == (xlo, ylo, cw, ch)
        sup.append(pts)
        qry.append(np.concatenate([lattice, near[:200]]))                                  # 489 queries
    return Case(name, np.stack(sup), np.stack(qry))


def _edge_race(name):
    """A K-th neighbour inside the window races a point just beyond the window's edge.  The 16 x 16 grid is fixed by four anchor
    points.  Every configuration lives on its own z level (levels 10 box sides apart, so configurations share cells but never
    neighbours): a query at 0.75 of its cell, K - 1 = 15 points close around it, an OUTSIDE point at the first float32 values on
    either side of the window edge bx0 + n * cw, and an INSIDE candidate on the other side of the query at the same distance,
    moved across it in single-ulp steps of the coordinate: 5 x 5 combinations.
      * 3 x 3 window (n = cell + 2): all 25 combinations in every crop, in the cell rows 4, 9 and 14.
      * 5 x 5 window (n = cell + 3): the first ring must end WITHOUT a K-th distance, so the 3 x 3 cells around such a query hold
        its 15 points and nothing else, on any level: one configuration per site (2, 7, 12)^2, nine combinations per crop (the
        three crops cover all 25), and the filler keeps to the cell rows 0, 5, 10 and 15.
    Built for K = 16; with another K there is no race, only a search.  info['outside'][b, q] is the outside point's index: the
    oracle has it among the K for some configurations and not for others."""
    rs = _rs(name)
    S, G, K = 2048, 16, 16
    place = [(0.0, 1.0), (-41.3, 0.37), (6037.1, 9.7)]      # box origin (x = y), side
    combos = [(so, si) for so in (-2, -1, 0, 1, 2) for si in (-2, -1, 0, 1, 2)]
    sup, qry, outside = [], [], []
    for b in range(B):
        o, L = f32(place[b][0]), f32(place[b][1])
        hi = f32(o + L)
        anchors = np.array([[o, o, 0], [hi, o, 0], [o, hi, 0], [hi, hi, 0]], f32)
        bx0, by0, cw, ch = o, o, f32((hi - o) / f32(G)), f32((hi - o) / f32(G))
        cfgs = [(1, (2, 7, 12)[i % 3], (4, 9, 14)[i // 3 % 3], so, si) for i, (so, si) in enumerate(combos)]
        cfgs += [(2, (2, 7, 12)[i % 3], (2, 7, 12)[i // 3], *combos[(8 * b + i) % 25]) for i in range(9)]
        pts, q, out_idx = [anchors], [], []
        n_pts = 4
        for lvl, (ring, cx, cy, so, si) in enumerate(cfgs):
            qz = f32((lvl + 1) * 10.0 * float(L))
            qx = f32(bx0 + f32(cx + 0.75) * cw)
            qy = f32(by0 + f32(cy + 0.5) * ch)
            x_out = _step(pm.edge(bx0, cx + 1 + ring, cw), so)
            x_in = _step(f32(qx - f32(x_out - qx)), si)
            around = np.stack([np.full(K - 1, qx), qy + (np.arange(K - 1) - 7) * 0.01 * float(ch), np.full(K - 1, qz)],
                              axis=1).astype(f32)
            pts.append(np.concatenate([around, [[x_in, qy, qz]], [[x_out, qy, qz]]]).astype(f32))
            out_idx.append(n_pts + K)
            n_pts += K + 1
            q.append([qx, qy, qz])
        fill = S - n_pts                                     # far below every level, inside the box, in rows 0, 5, 10, 15
        fy = by0 + (rs.choice([0, 5, 10, 15], fill) + 0.1 + 0.8 * rs.rand(fill)) * float(ch)
        filler = np.stack([o + rs.rand(fill) * float(L), fy, -30.0 * float(L) - rs.rand(fill)], axis=1)
        filler = np.clip(filler.astype(f32), [o, o, -np.inf], [hi, hi, np.inf]).astype(f32)
        pts = np.concatenate(pts + [filler]).astype(f32)
        assert pts.shape == (S, 3) and pm.cells_box(pts, G)[:4] == (bx0, by0, cw, ch)
        sup.append(pts)
        qry.append(np.array(q, f32))
        outside.append(out_idx)
    return Case(name, np.stack(sup), np.stack(qry), info={"outside": np.array(outside), "ring2": slice(25, 34)})


# ---- organised --------------------------------------------------------------------------------------------------------------
def _pinhole(rs, H, W, fx, ppx, ppy, b, holes=0.0, noise=2e-3, step_edge=True, scale=1.0, wall=None, amp=0.1):
    """xyz map [H*W,3] of a pinhole depth image: a smooth surface, a depth step, noise, holes (points at the origin)."""
    v, u = np.mgrid[:H, :W].astype(np.float64)
    if wall is not None:
        z = np.full((H, W), wall)
    else:
        z = 0.8 + amp * np.sin(u / 7.0 + b) * np.cos(v / 5.0) + (rs.rand(H, W) - 0.5) * noise
        if step_edge:
            z[:, W // 2:] += 0.35
    z = z.astype(f32)
    z[rs.rand(H, W) < holes] = 0.0
    x = ((u - ppx).astype(f32) * z / f32(fx)).astype(f32)
    y = ((v - ppy).astype(f32) * z / f32(fx)).astype(f32)
    m = np.stack([x, y, z], axis=2) * (z > 0)[:, :, None]
    return (m.reshape(-1, 3) * f32(scale)).astype(f32)


def _surface_queries(rs, sup, Q, sigma, exact=0.25):
    """Queries around valid support points: the first `exact` share exactly on them, the rest sigma x depth beside."""
    out = []
    for b in range(B):
        valid = np.flatnonzero(sup[b][:, 2] > 0)
        p = sup[b][valid[rs.randint(0, len(valid), Q)]].astype(np.float64)
        n = int(Q * exact)
        p[n:] += rs.randn(Q - n, 3) * sigma * p[n:, 2:3]
        out.append(p.astype(f32))
    return np.stack(out)


def _wide_fov(name):
    rs = _rs(name)
    H, W = 48, 64
    cam = [(3.2, 32.0, 24.0), (4.1, 30.3, 20.9), (3.0, 35.6, 26.2)]            # |x/z| up to about 10
    sup = np.stack([_pinhole(rs, H, W, *cam[b], b, holes=0.02) for b in range(B)])
    return Case(name, sup, _surface_queries(rs, sup, 200, 0.01), W=W)


def _off_axis(name):
    """The principal point thousands of pixels outside the image.  A depth change moves a point ALONG its ray, here almost
    parallel to the image plane, so the surface is kept nearly flat: the pixel pitch, not the relief, sets the K-th distance."""
    rs = _rs(name)
    H, W = 48, 128
    cam = [(900.0, 4000.4, 3000.2), (700.0, -5000.7, 2500.1), (1200.0, 3500.3, -6000.6)]  # every ratio of a crop has one sign
    sup = np.stack([_pinhole(rs, H, W, *cam[b], b, holes=0.02, noise=1e-5, step_edge=False, amp=1e-3) for b in range(B)])
    return Case(name, sup, _surface_queries(rs, sup, 200, 0.002), W=W, min_pruned=0.1)


def _flat_wall(name):
    """Fronto-parallel, zero noise: a column's x / z is one value (lo == hi).  Queries exactly on support points, and exactly on
    their rays (the point halved or doubled: the same ratio, bit for bit)."""
    rs = _rs(name)
    H, W = 48, 64
    cam = [(76.8, 32.37, 23.79), (61.0, 30.0, 24.0), (90.3, 35.5, 20.25)]
    sup = np.stack([_pinhole(rs, H, W, *cam[b], b, wall=[0.8, 1.37, 2.0][b]) for b in range(B)])
    qry = []
    for b in range(B):
        p = sup[b][rs.randint(0, H * W, 210)]
        qry.append(np.concatenate([p[:130], p[130:170] * f32(0.5), p[170:] * f32(2.0)]).astype(f32))
    c = Case(name, sup, np.stack(qry), W=W)
    for b in range(B):
        lo, hi = pm.grid_ranges(sup[b], W)[:2]
        assert np.array_equal(lo, hi)
    return c


def _ulp_wall(name):
    """A 256 x 8 wall whose pixel pitch is a few ulps of the coordinate: the plane bounds of neighbouring columns differ by less
    than their own rounding error, which only the slack covers.  Queries on support points of the middle rows."""
    rs = _rs(name)
    H, W = 8, 256
    sup, qry = [], []
    for b in range(B):
        z0 = f32([0.8, 0.77, 1.3][b])
        x0, y0 = f32([0.07, -0.1, 0.11][b]), f32([0.09, 0.065, -0.12][b])
        s = [2, 1, 3][b]                                    # pitch in ulps of the coordinate
        ux, uy = np.spacing(x0) * s, np.spacing(y0) * s
        x = (x0 + np.arange(W) * ux).astype(f32)
        y = (y0 + np.arange(H) * uy).astype(f32)
        gx, gy = np.meshgrid(x, y)
        m = np.stack([gx, gy, np.full_like(gx, z0)], axis=2).reshape(-1, 3).astype(f32)
        sup.append(m)
        rows = rs.randint(2, 6, 200)
        cols = rs.randint(0, W, 200)
        qry.append(m[rows * W + cols])
    return Case(name, np.stack(sup), np.stack(qry), W=W)


def _scaled(name):
    scale = float(name.split("_", 1)[1])                    # scale_1e-3
    rs = _rs("scale")                                       # ONE map at three scales
    H, W = 64, 64
    cam = [(76.8, 32.37, 31.79), (70.0, 28.1, 35.3), (90.0, 40.2, 30.6)]
    sup = np.stack([_pinhole(rs, H, W, *cam[b], b, holes=0.03) for b in range(B)])
    qry = _surface_queries(rs, sup, 200, 0.004)
    return Case(name, (sup * f32(scale)).astype(f32), (qry * f32(scale)).astype(f32), W=W)


def _kth_valid(sup, q, K):
    """The K-th smallest float32 squared distance from q to the points of sup that are not holes."""
    valid = sup[(sup != 0).any(axis=1)]
    return np.partition(pm.dist2(q[None], valid)[0], K - 1)[K - 1]


def _hole_race(name):
    """Maps with holes.  Forty queries sit close to the origin (the holes ARE their nearest neighbours); 140 lie on a
    ray t * p: at the float32 values of t around the one where |q|^2 crosses the K-th distance to the surface (K = 16), so that
    the origin is just inside or just outside the K, and around the larger t where |q|^2 * 0.999 crosses the first phase's K-th
    distance (the rule's own boundary, found with tests/knn_prune_model.py); the rest are ordinary surface queries, for which holes do not matter.
    Crop 1 has its two leftmost columns dead, crop 2 its two top rows: holes that no window reaches by plane bounds alone."""
    rs = _rs(name)
    H, W, K = 48, 64, 16
    cam = [(76.8, 32.37, 23.79), (66.0, 28.1, 27.3), (88.0, 37.2, 22.6)]
    sup = np.stack([_pinhole(rs, H, W, *cam[b], b, holes=0.05, step_edge=False) for b in range(B)])
    sup[1].reshape(H, W, 3)[:, :2] = 0
    sup[2].reshape(H, W, 3)[:2, :] = 0
    qry = []
    for b in range(B):
        valid = np.flatnonzero(sup[b][:, 2] > 0)
        p = sup[b][valid[rs.randint(0, len(valid), 40)]]
        near_origin = (p * rs.uniform(0.005, 0.3, (40, 1))).astype(f32)
        race = []
        for target in sup[b][valid[rs.randint(0, len(valid), 10)]]:
            lo, hi = f32(0.05), f32(0.95)                   # |t p|^2 - kth(t p) rises through zero between them
            for _ in range(40):
                mid = f32((lo + hi) * f32(0.5))
                q = (target * mid).astype(f32)
                if pm.dist2(q[None], np.zeros((1, 3), f32))[0, 0] < _kth_valid(sup[b], q, K):
                    lo = mid
                else:
                    hi = mid
            race += [(target * _step(hi, n)).astype(f32) for n in (-3, -2, -1, 0, 1, 2, 3)]
            lo, hi = hi, f32(0.95)                          # the rule's own boundary: |q|^2 * 0.999 against the FIRST PHASE's K-th
            for _ in range(40):
                mid = f32((lo + hi) * f32(0.5))
                if pm.grid_search(sup[b], (target * mid).astype(f32)[None], K, W)["holes_matter"][0]:
                    lo = mid
                else:
                    hi = mid
            race += [(target * _step(hi, n)).astype(f32) for n in (-3, -2, -1, 0, 1, 2, 3)]
        ordinary = _surface_queries(rs, sup, 240, 0.004)[b]
        qry.append(np.concatenate([near_origin, np.array(race, f32), ordinary]))
    return Case(name, sup, np.stack(qry), W=W, info={"race": slice(40, 180)})


def _dead_lines(name):
    """Whole columns and rows without a valid pixel (empty range: bound +inf), at the border and inside.  Queries around the
    pixels next to them, and a few close to the origin."""
    rs = _rs(name)
    H, W = 48, 64
    cam = [(76.8, 32.37, 23.79), (70.0, 28.1, 27.3), (90.0, 40.2, 20.6)]
    sup = np.stack([_pinhole(rs, H, W, *cam[b], b, holes=0.01) for b in range(B)])
    dead_c, dead_r = [(0, 1, 30, 31, 63), (5, 40, 41, 42), (0, 62, 63)], [(0, 20, 47), (10, 11), (46, 47, 3)]
    qry = []
    for b in range(B):
        g = sup[b].reshape(H, W, 3)
        g[:, list(dead_c[b])] = 0
        g[list(dead_r[b]), :] = 0
        cand = []
        for c in dead_c[b]:
            cand += [r * W + cc for r in range(H) for cc in (c - 1, c + 1) if 0 <= cc < W]
        for r in dead_r[b]:
            cand += [rr * W + c for c in range(W) for rr in (r - 1, r + 1) if 0 <= rr < H]
        cand = np.array([i for i in cand if sup[b][i, 2] > 0])
        p = sup[b][cand[rs.randint(0, len(cand), 200)]].astype(np.float64)
        p[50:] += rs.randn(150, 3) * 0.004 * p[50:, 2:3]
        p[180:] *= rs.uniform(0.01, 0.2, (20, 1))
        qry.append(p.astype(f32))
    return Case(name, sup, np.stack(qry), W=W)


def _small_grids(name):
    H, W = {"grid_8x8": (8, 8), "grid_7x40": (7, 40), "grid_256x8": (256, 8)}[name]
    rs = _rs(name)
    cam = [(1.2 * W, W / 2 + 0.37, H / 2 - 0.21), (1.0 * W, W / 2 - 1.3, H / 2 + 0.4), (1.5 * W, W / 2 + 2.1, H / 2 - 3.3)]
    if name == "grid_256x8":
        cam = [(300.0, 4.37, 127.8), (250.0, 2.9, 140.4), (350.0, 6.1, 100.3)]
    sup = np.stack([_pinhole(rs, H, W, *cam[b], b, holes=0.03, step_edge=False) for b in range(B)])
    # 8 x 8: the first phase already holds the whole grid, the window can only shrink; 7 x 40 is below the 8-cell minimum: the hint
    # is declined and the search is exhaustive
    return Case(name, sup, _surface_queries(rs, sup, 120, 0.004), W=W)


def _qz_nonpositive(name):
    """A quarter of the queries at or behind the camera plane (qz <= 0: no plane bound holds, the unstructured path)."""
    rs = _rs(name)
    H, W = 48, 64
    cam = [(76.8, 32.37, 23.79), (70.0, 28.1, 27.3), (90.0, 40.2, 20.6)]
    sup = np.stack([_pinhole(rs, H, W, *cam[b], b, holes=0.02) for b in range(B)])
    qry = _surface_queries(rs, sup, 200, 0.004)
    qry[:, :25, 2] *= f32(-1)
    qry[:, 25:40, 2] = f32(0.0)
    qry[:, 40:50, 2] = f32(-0.0)
    return Case(name, sup, qry, W=W)


_OFFSETS = ["offset_%s_2p%d" % (k, p) for k in ("sheet", "cube") for p in (8, 12, 16, 20)]
_SIZES = ["sizes_%d_%s" % (s, k) for s in (1023, 1024, 8191, 8192) for k in ("sheet", "clustered", "dups")]
UNORGANISED = _OFFSETS + ["edge_race", "edge_points", "heavy_cell", "line_x", "line_y"] + _SIZES
ORGANISED = ["wide_fov", "off_axis", "flat_wall", "ulp_wall", "scale_1e-3", "scale_1", "scale_1e4", "hole_race", "dead_lines",
             "grid_8x8", "grid_7x40", "grid_256x8", "qz_nonpositive"]
NAMES = UNORGANISED + ORGANISED


@functools.lru_cache(maxsize=None)
def make(name):
    if name.startswith("offset_"):
        c = _offset(name)
    elif name.startswith("sizes_"):
        c = _sizes(name)
    elif name.startswith("scale_"):
        c = _scaled(name)
    elif name.startswith("grid_"):
        c = _small_grids(name)
    else:
        c = {"edge_race": _edge_race, "edge_points": _edge_points, "heavy_cell": _heavy_cell, "line_x": _line, "line_y": _line,
             "wide_fov": _wide_fov, "off_axis": _off_axis, "flat_wall": _flat_wall, "ulp_wall": _ulp_wall,
             "hole_race": _hole_race, "dead_lines": _dead_lines, "qz_nonpositive": _qz_nonpositive}[name](name)
    assert c.sup.dtype == np.float32 and c.qry.dtype == np.float32
    assert c.sup.shape[0] == B and c.qry.shape[0] == B and c.sup.shape[1] <= 8192 and c.qry.shape[1] <= 512
    assert np.isfinite(c.sup).all() and np.isfinite(c.qry).all()
    c.sup.setflags(write=False)
    c.qry.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def want(name, K):
    """The oracle's (idx i64[B,Q,K], d2 f32[B,Q,K]) for a case: computed once, read-only."""
    from oracle import knn as oknn
    c = make(name)
    idx, d2 = oknn.knn_batch(c.sup, c.qry, K, return_d2=True)
    idx.setflags(write=False)
    d2.setflags(write=False)
    return idx, d2
