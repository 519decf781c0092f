"""A float32 restatement, in plain numpy, of the two pruning rules of csrc/gdm_knn.hip -- the ring walk of knn_cells_kernel over
the cell list of knn_cells_bin_kernel, and the column / row window of knn_grid_kernel over the ratio ranges of
knn_grid_ranges_kernel.  Every operation is rounded to float32 in the order the kernel performs it (the library is built with
-ffp-contract=off, and hipcc rounds fp32 division and square root correctly by default, as numpy does), so what a rule decides
here is what the kernel decides.  The model never calls the library; the truth it is held to is oracle.knn.knn_batch.

What is NOT restated is the selection (KnnSelection): it keeps the K smallest (d2, index) keys of the candidates it is given,
which is what np.sort of the keys does.  The rules only decide WHICH support points become candidates.

The argument the model makes executable (csrc/gdm_knn.hip and DESIGN.md carry it in words):

  cell list.  A point v was binned by cell(v) = trunc(fl(fl(v - lo) * inv)), a query measures its distance to the edge
  E(n) = fl(lo + fl(n * cw)).  An unvisited point beyond the edge E(n) has cell(v) >= n.  Were the arithmetic exact it would lie at
  v >= lo + n * cw.  It is not exact in two ways.  (1) ABSOLUTE: lo + n * cw is rounded to the float grid at |lo|, which may be
  coarser than a cell.  But v lies on the same grid, and rounding to nearest is monotone: v >= e implies v = fl(v) >= fl(e).  So
  the rounding of the edge never puts it beyond a point that is beyond the exact edge, however large |lo| / extent is.
  (2) RELATIVE: fl(v - lo), the product with inv = fl(1 / cw), cw = fl(extent / G) and fl(n * cw) each carry half an ulp, so the
  boundary the binning drew lies within ~4 * 2^-24 * G cells = 8e-6 cells of lo + n * cw.  The edge distance m the exit test uses is
  at least one cell minus that (the window holds the query's own cell and its neighbours), so the error is below 1e-5 of m, 2e-5
  of m * m.  That is what the factor 0.999 on m * m has to cover, fifty times over.  Where the grid at |lo| is coarser than a cell,
  m comes out as 0 or as whole ulps: 0 never exits (m > 0 is required), and a whole-ulp m is exact.

  organised.  The plane bound of a column is at most |q|^2 (the planes hold the origin), its rounding error is absolute: a few
  ulps of |q| in dl = p - lo * z where p and lo * z cancel.  slack = 2e-6 |q| = 33 ulps of |q| is taken off the bound's root for
  that, the factor 0.999 covers the relative error of the division and the squares.  A point at the origin is on every plane, so
  no bound speaks for it: the |q|^2 test widens the window to the whole grid whenever an origin point could be among the K.

The two constants and two structural choices are parameters (PruneParams), so that tests can perturb the MODEL and see that the
adversarial cases notice.
"""
from dataclasses import dataclass

import numpy as np

f32 = np.float32
INF = f32(np.inf)
FLT_MAX = f32(3.402823466e+38)
IDX_EMPTY = 0x7fffffff
KEY_EMPTY = np.uint64((0x7f800000 << 32) | IDX_EMPTY)

KC_MIN_S = 1024
KG_MAXDIM = 256


def kc_grid(S):
    return 32 if S >= 8192 else 16


@dataclass(frozen=True)
class PruneParams:
    factor: float = 0.999          # on m * m, on (sqrt(bound) - slack)^2 and on |q|^2
    slack: float = 2e-6            # times |q|, off the root of a plane bound
    cell_round_up: bool = False    # cell_coord rounds f up instead of truncating it (a perturbation)
    hole_test: bool = True         # the |q|^2 test that widens the window for points at the origin


KERNEL = PruneParams()


# ---- shared: distances and keys ---------------------------------------------------------------------------------------------
def dist2(q, p):
    """((dx*dx) + dy*dy) + dz*dz, every operation rounded to float32; q [Q,3] against p [S,3] -> [Q,S]."""
    q = np.asarray(q, f32)
    p = np.asarray(p, f32)
    d0 = q[:, None, 0] - p[None, :, 0]
    d1 = q[:, None, 1] - p[None, :, 1]
    d2 = q[:, None, 2] - p[None, :, 2]
    r = d0 * d0
    r = r + d1 * d1
    r = r + d2 * d2
    assert r.dtype == np.float32
    return r


def make_keys(d2):
    """(d2, index) as one uint64 per pair: d2 >= 0, so its bits order like unsigned integers; the index breaks ties."""
    idx = np.arange(d2.shape[1], dtype=np.uint64)
    return (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[None, :]


def _smallest(keys, mask, K):
    """The K smallest keys of every row among the columns `mask` allows, ascending, padded with KEY_EMPTY."""
    k = np.where(mask, keys, KEY_EMPTY)
    if k.shape[1] < K:
        k = np.concatenate([k, np.full((k.shape[0], K - k.shape[1]), KEY_EMPTY, np.uint64)], axis=1)
    if k.shape[1] > K:
        k = np.partition(k, K - 1, axis=1)[:, :K]
    return np.sort(k, axis=1)


def _key_d2(keys):
    return (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)


def keys_to_outputs(keys):
    """What KnnSelection::store writes: an empty slot is index 0 at distance FLT_MAX."""
    idx = (keys & np.uint64(0xffffffff)).astype(np.int64)
    d2 = _key_d2(keys).copy()
    empty = idx == IDX_EMPTY
    idx[empty] = 0
    d2[np.isinf(d2)] = FLT_MAX
    return idx, d2


# ---- cell list --------------------------------------------------------------------------------------------------------------
def cell_coord(v, lo, inv, G, params=KERNEL):
    """cell_coord of the kernel: f = (v - lo) * inv; f >= 0 ? (f < G ? (int)f : G - 1) : 0."""
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        f = (v - f32(lo)) * f32(inv)
        t = np.ceil(f) if params.cell_round_up else np.trunc(f)
        c = np.where(f >= 0, np.where(f < f32(G), t, f32(G - 1)), f32(0))
        c = np.minimum(c, f32(G - 1))                    # ceil of a value just below G
    return c.astype(np.int64)


def cells_box(sup, G):
    """bx0, by0, cw, ch, icw, ich as thread 0 of knn_cells_bin_kernel forms them (min and max are exact in any order)."""
    sup = np.asarray(sup, f32)
    x, y = sup[:, 0], sup[:, 1]
    fx, fy = x[np.isfinite(x)], y[np.isfinite(y)]
    xlo, xhi = (fx.min(), fx.max()) if fx.size else (f32(0), f32(0))
    ylo, yhi = (fy.min(), fy.max()) if fy.size else (f32(0), f32(0))
    cw = (xhi - xlo) / f32(G)
    ch = (yhi - ylo) / f32(G)
    icw = f32(1) / cw if cw > 0 else f32(0)
    ich = f32(1) / ch if ch > 0 else f32(0)
    out = tuple(f32(t) for t in (xlo, ylo, cw, ch, icw, ich))
    assert all(t.dtype == np.float32 for t in out)
    return out


def edge(lo, n, c):
    """lo + (float)n * c in two roundings (no contraction)."""
    return f32(lo) + (np.asarray(n).astype(f32) * f32(c))


def cells_search(sup, qry, K, params=KERNEL):
    """knn_cells_bin_kernel + knn_cells_kernel for one crop: sup f32[S,3], qry f32[Q,3].
    -> dict: keys u64[Q,K]; rings i[Q] (rings walked); early b[Q] (left the walk through the exit test, before the window was
    the whole grid); td list of f32[Q] per ring (NaN for queries that had finished); window i[Q,4] (x0, x1, y0, y1 at the end)."""
    sup = np.ascontiguousarray(sup, f32)
    qry = np.ascontiguousarray(qry, f32)
    S, Q = sup.shape[0], qry.shape[0]
    G = kc_grid(S)
    bx0, by0, cw, ch, icw, ich = cells_box(sup, G)
    pcx = cell_coord(sup[:, 0], bx0, icw, G, params)
    pcy = cell_coord(sup[:, 1], by0, ich, G, params)
    qcx = cell_coord(qry[:, 0], bx0, icw, G, params)
    qcy = cell_coord(qry[:, 1], by0, ich, G, params)
    keys = make_keys(dist2(qry, sup))
    qx, qy = qry[:, 0], qry[:, 1]
    factor = f32(params.factor)
    cmin = min(cw if cw > 0 else INF, ch if ch > 0 else INF)

    out = np.full((Q, K), KEY_EMPTY, np.uint64)
    rings = np.zeros(Q, np.int64)
    early = np.zeros(Q, bool)
    window = np.zeros((Q, 4), np.int64)
    r = np.ones(Q, np.int64)
    act = np.arange(Q)
    td_log = []
    while act.size:
        ra = r[act]
        nx0, nx1 = np.maximum(qcx[act] - ra, 0), np.minimum(qcx[act] + ra, G - 1)
        ny0, ny1 = np.maximum(qcy[act] - ra, 0), np.minimum(qcy[act] + ra, G - 1)
        mask = ((pcx[None, :] >= nx0[:, None]) & (pcx[None, :] <= nx1[:, None]) &
                (pcy[None, :] >= ny0[:, None]) & (pcy[None, :] <= ny1[:, None]))
        best = _smallest(keys[act], mask, K)             # every ring's cells are new, so the K best of the window so far
        td = _key_d2(best[:, K - 1])                     # +inf while fewer than K are known
        out[act] = best
        rings[act] += 1
        window[act] = np.stack([nx0, nx1, ny0, ny1], axis=1)
        log = np.full(Q, np.nan, f32)
        log[act] = td
        td_log.append(log)
        whole = (nx0 == 0) & (nx1 == G - 1) & (ny0 == 0) & (ny1 == G - 1)
        with np.errstate(invalid="ignore", over="ignore"):
            exl = np.where(nx0 == 0, INF, qx[act] - edge(bx0, nx0, cw))
            exh = np.where(nx1 == G - 1, INF, edge(bx0, nx1 + 1, cw) - qx[act])
            eyl = np.where(ny0 == 0, INF, qy[act] - edge(by0, ny0, ch))
            eyh = np.where(ny1 == G - 1, INF, edge(by0, ny1 + 1, ch) - qy[act])
            m = np.fmin(np.fmin(exl, exh), np.fmin(eyl, eyh)).astype(f32)
            leave = ~whole & (m > 0) & ((m * m) * factor > td)
            early[act] = leave
            # next ring: far enough for the current K-th distance where it is known, else twice as far
            want = ra * 2
            if cmin < INF:
                known = td < INF
                w = np.fmin(f32(G), np.ceil(np.sqrt(np.where(known, td, f32(0))) / f32(cmin))).astype(np.int64) + 1
                want = np.where(known, w, want)
        r[act] = np.minimum(G, np.maximum(ra + 1, want))
        act = act[~(whole | leave)]
    return {"keys": out, "rings": rings, "early": early, "td": td_log, "window": window, "G": G}


# ---- organised --------------------------------------------------------------------------------------------------------------
def is_grid_job(S, W, K):
    return K > 1 and W > 0 and S % W == 0 and W <= KG_MAXDIM and S // W <= KG_MAXDIM and W >= 8 and S // W >= 8


def grid_ranges(sup, W):
    """knn_grid_ranges_kernel for one crop: (col_lo, col_hi, row_lo, row_hi, bad, hole).  A line without a valid pixel has
    lo = +inf, hi = -inf (key 0 on both sides).  A ratio that overflows to infinity is not recorded either (isinf -> key 0)."""
    sup = np.ascontiguousarray(sup, f32)
    H = sup.shape[0] // W
    g = sup.reshape(H, W, 3)
    x, y, z = g[..., 0], g[..., 1], g[..., 2]
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    hole = fin & (x == 0) & (y == 0) & (z == 0)
    bad = bool((~fin).any() or (fin & ~(z > 0) & ~hole).any())
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        col_ok = (z > 0) & np.isfinite(x) & np.isfinite(z)
        row_ok = fin & (z > 0)
        ac = np.where(col_ok, x / np.where(col_ok, z, f32(1)), f32(np.nan)).astype(f32)
        ar = np.where(row_ok, y / np.where(row_ok, z, f32(1)), f32(np.nan)).astype(f32)

    def rng(a, axis):
        nlo = np.fmax.reduce(np.where(np.isnan(a), -INF, -a), axis=axis)     # the kernel keeps max(-a) and max(a)
        hi = np.fmax.reduce(np.where(np.isnan(a), -INF, a), axis=axis)
        lo = np.where(np.isinf(nlo), INF, -nlo).astype(f32)                 # key 0 -> ord_val = -inf -> lo = +inf
        hi = np.where(np.isinf(hi), -INF, hi).astype(f32)
        return lo, hi

    col_lo, col_hi = rng(ac, 0)
    row_lo, row_hi = rng(ar, 1)
    return col_lo, col_hi, row_lo, row_hi, bad, bool(hole.any())


def plane_bound(p, z, lo, hi):
    """plane_bound of the kernel for queries p, z [Q] against ranges lo, hi [L] -> [Q,L]."""
    p = np.asarray(p, f32)[:, None]
    z = np.asarray(z, f32)[:, None]
    lo = np.asarray(lo, f32)[None, :]
    hi = np.asarray(hi, f32)[None, :]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = p / z
        dl = p - lo * z
        dh = p - hi * z
        b = np.fmin(dl * dl / (f32(1) + lo * lo), dh * dh / (f32(1) + hi * hi))
        b = np.where((r >= lo) & (r <= hi), f32(0), b)
        b = np.where(lo <= hi, b, INF)
    return b.astype(f32)


def grid_search(sup, qry, K, W, params=KERNEL):
    """knn_grid_ranges_kernel + knn_grid_kernel for one crop (is_grid_job must hold).
    -> dict: keys u64[Q,K]; window i[Q,4] (c0, c1, r0, r1); pruned b[Q] (the window is smaller than the grid); structured b[Q];
    holes_matter b[Q] (the |q|^2 test fired); td f32[Q] (the first phase's K-th distance; NaN where unstructured)."""
    sup = np.ascontiguousarray(sup, f32)
    qry = np.ascontiguousarray(qry, f32)
    S, Q = sup.shape[0], qry.shape[0]
    H = S // W
    assert is_grid_job(S, W, K)
    col_lo, col_hi, row_lo, row_hi, bad, has_hole = grid_ranges(sup, W)
    qx, qy, qz = qry[:, 0], qry[:, 1], qry[:, 2]
    structured = (not bad) & (qz > 0) & np.isfinite(qx) & np.isfinite(qy) & np.isfinite(qz)
    q2 = dist2(qry, np.zeros((1, 3), f32))[:, 0]
    keys = make_keys(dist2(qry, sup))
    pc = np.tile(np.arange(W), H)
    pr = np.repeat(np.arange(H), W)
    factor = f32(params.factor)

    lbc = np.where(structured[:, None], plane_bound(qx, qz, col_lo, col_hi), f32(0)).astype(f32)
    lbr = np.where(structured[:, None], plane_bound(qy, qz, row_lo, row_hi), f32(0)).astype(f32)
    # phase 1: the 8 x 8 cells around the column / row of the smallest bound (lowest index among equals)
    uc = np.clip(np.argmin(lbc, axis=1) - 4, 0, W - 8)
    vc = np.clip(np.argmin(lbr, axis=1) - 4, 0, H - 8)
    m1 = ((pc[None, :] >= uc[:, None]) & (pc[None, :] < uc[:, None] + 8) &
          (pr[None, :] >= vc[:, None]) & (pr[None, :] < vc[:, None] + 8))
    first = _smallest(keys, m1, K)
    bound_key = first[:, K - 1]
    td = _key_d2(bound_key)
    # phase 2: the columns / rows whose bound, less the allowance, can still be below the K-th distance
    with np.errstate(invalid="ignore", over="ignore"):
        slack = f32(params.slack) * np.sqrt(q2)

        def keep(lb):
            s = np.sqrt(lb) - slack[:, None]
            return (s <= 0) | ((s * s) * factor <= td[:, None])

        kc, kr = keep(lbc), keep(lbr)
        holes_matter = (q2 * factor <= td) & has_hole & params.hole_test
    anyc, anyr = kc.any(axis=1), kr.any(axis=1)
    cl = np.where(anyc, np.argmax(kc, axis=1), W)
    chh = np.where(anyc, W - 1 - np.argmax(kc[:, ::-1], axis=1), -1)
    rl = np.where(anyr, np.argmax(kr, axis=1), H)
    rh = np.where(anyr, H - 1 - np.argmax(kr[:, ::-1], axis=1), -1)
    use = structured & ~holes_matter & (chh >= cl) & (rh >= rl)
    c0, c1 = np.where(use, cl, 0), np.where(use, chh, W - 1)
    r0, r1 = np.where(use, rl, 0), np.where(use, rh, H - 1)
    m2 = ((pc[None, :] >= c0[:, None]) & (pc[None, :] <= c1[:, None]) &
          (pr[None, :] >= r0[:, None]) & (pr[None, :] <= r1[:, None]))
    # the second pass starts over with the first phase's bound, inclusive: a candidate above it is never admitted
    m2 &= ~structured[:, None] | (keys <= bound_key[:, None])
    out = _smallest(keys, m2, K)
    window = np.stack([c0, c1, r0, r1], axis=1)
    pruned = (c1 - c0 + 1) * (r1 - r0 + 1) < S
    return {"keys": out, "window": window, "pruned": pruned, "structured": structured,
            "holes_matter": structured & holes_matter, "td": np.where(structured, td, f32(np.nan))}


# ---- the ladder --------------------------------------------------------------------------------------------------------------
def search(sup, qry, K, W=0, params=KERNEL):
    """The form the library's default ladder gives a K > 1 job for one crop: 'grid', 'cells', or None (exhaustive: nothing to
    model).  -> (form, result dict or None)."""
    S = np.asarray(sup).shape[0]
    if is_grid_job(S, W, K):
        return "grid", grid_search(sup, qry, K, W, params)
    if K > 1 and S >= KC_MIN_S:
        return "cells", cells_search(sup, qry, K, params)
    return None, None
