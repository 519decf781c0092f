"""Inference-time dense matching of scene descriptors against the object model.

Mirrors the matching part of `cal_frame_poses` (/root/reference/evaluator.py:60-102, lines 78-93):
  seg_res  = argmax(seg_features, dim=0) ; cls_msk = seg_res == 1
  selected = F.normalize(rgbd_features.T[cls_msk]) ; mesh = F.normalize(mesh_features, dim=0)
  obj_pts_sim = selected @ mesh ; max_th, obj_pts_idx = max(obj_pts_sim, dim=1)

The reference runs this per crop on `bs` host threads and materialises the [n_sel, M] matrix.  Here
the whole batch is ONE fused HIP launch sequence (normalise+pack, MFMA similarity with in-register
row arg-max, optional split merge) that never writes the matrix; rows of unselected points are
computed too (the mask is data dependent) and simply ignored by `selected`.
"""
import numpy as np
import torch

from . import ops

_PREC = {"bf16x3": ops.MATCH_BF16X3, "f32": ops.MATCH_F32, 0: 0, 1: 1}


def _soft_args(soft, who):
    """soft = None | dict(gamma=..., model_xyz=f32[M,3]) -> (gamma, model_xyz) or None."""
    if soft is None:
        return None
    if set(soft) != {"gamma", "model_xyz"}:
        raise ValueError("%s: soft must be dict(gamma=..., model_xyz=...), got keys %s" % (who, sorted(soft)))
    return float(soft["gamma"]), soft["model_xyz"]


def _no_soft_twoway(sa, twoway, who):
    if twoway and sa is not None:
        raise ValueError("%s: twoway and soft exclude each other (there is no soft two-way kernel)" % who)


def _dual_args(sa, twoway, dual, who):
    """dual needs soft and takes the place of twoway (its outputs include col_idx / col_sim)."""
    if dual and sa is None:
        raise ValueError("%s: dual=True needs soft=dict(gamma=..., model_xyz=...) (the dual softmax has a temperature)" % who)
    if dual and twoway:
        raise ValueError("%s: dual=True already returns col_idx / col_sim; do not pass twoway=True with it" % who)
    return bool(dual)


def match_frames(end_points, precision="bf16x3", return_sim=False, soft=None, twoway=False, dual=False):
    """end_points: GeoMatch.forward output (seg [B,2,N], rgbd [B,128,N], mesh [1,128,M]).
    Returns dict(mask u8[B,N], count i32[B], best_idx i32[B,N], best_sim f32[B,N] [, sim f32[B,N,M]]).
    soft = dict(gamma=..., model_xyz=f32[M,3]) takes the soft kernel instead (ops.match_soft: the same best_idx / best_sim) and adds
    lse f32[B,N], conf f32[B,N], soft_xyz f32[B,N,3].
    twoway takes the two-way kernel instead (ops.match_twoway under the mask: the same best_idx / best_sim) and adds col_idx i32[B,M],
    col_sim f32[B,M]: per vertex the masked point that matches it best (include/gdm.h THE TWO-WAY RULE).
    soft together with dual=True takes the dual kernel (ops.match_dual under the mask: the soft outputs and the two-way outputs, the
    same bits) and adds col_lse f32[B,M], col_conf f32[B,M], dual f32[B,N] (include/gdm.h THE DUAL RULE)."""
    seg, rgbd, mesh = end_points["seg"], end_points["rgbd"], end_points["mesh"]
    sa = _soft_args(soft, "match_frames")
    dual = _dual_args(sa, twoway, dual, "match_frames")
    _no_soft_twoway(sa, twoway, "match_frames")
    mask, count = ops.seg_mask(seg)
    mesh = mesh[0] if mesh.dim() == 3 else mesh
    if dual:
        if return_sim:
            raise ValueError("match_frames: return_sim and dual exclude each other (the dual kernel writes no matrix)")
        out = ops.match_dual(rgbd, mesh, sa[1], mask, _PREC[precision], sa[0])
        return dict(zip(ops.DUAL_KEYS, out), mask=mask, count=count)
    if twoway:
        if return_sim:
            raise ValueError("match_frames: return_sim and twoway exclude each other (the two-way kernel writes no matrix)")
        bi, bs, ci, cs = ops.match_twoway(rgbd, mesh, mask, _PREC[precision])
        return dict(mask=mask, count=count, best_idx=bi, best_sim=bs, col_idx=ci, col_sim=cs)
    if sa is None:
        out = ops.match(rgbd, mesh, precision=_PREC[precision], return_sim=return_sim)
        res = dict(mask=mask, count=count, best_idx=out[0], best_sim=out[1])
        if return_sim:
            res["sim"] = out[2]
        return res
    if return_sim:
        raise ValueError("match_frames: return_sim and soft exclude each other (the soft kernel writes no matrix)")
    bi, bs, lse, conf, sxyz = ops.match_soft(rgbd, mesh, sa[1], _PREC[precision], sa[0])
    return dict(mask=mask, count=count, best_idx=bi, best_sim=bs, lse=lse, conf=conf, soft_xyz=sxyz)


def match_tail(end_points, B, N, M, precision=ops.MATCH_BF16X3, soft=None, twoway=False, dual=False):
    """The step's tail on packed rows (evaluator.py:78-93): seg mask, descriptor packs, N x M arg-max -> (mask, count, best_idx, best_sim).
    With settings.USE_SIDE_STREAMS the mask -- which the arg-max does not read -- is formed on a side stream beside the matching
    kernel, and the model's descriptor rows are taken from `end_points["mesh_rows"]` when GeoMatch.forward packed them inside its
    mesh fork (same kernels, same operands: same bits); the scene's rows likewise from `end_points["scene_rows"]` when the fused heads
    wrote them (bf16x3 only: the pack kernel's own code on the same values, same bytes).  soft = dict(gamma=..., model_xyz=...): the soft kernel in place of the
    arg-max kernel, and (lse, conf, soft_xyz) appended to the result.  twoway: the two-way kernel in its place, and (col_idx, col_sim)
    appended; that kernel reads the mask, so the mask is formed in front of it on the same stream and its side-stream fork is not
    taken.  soft together with dual=True: the dual kernel in its place, behind the mask like the two-way kernel, and the ten tensors
    of ops.DUAL_KEYS (the soft result, then col_idx, col_sim, col_lse, col_conf, dual) after (mask, count)."""
    from . import settings
    seg, rgbd, mesh = end_points["seg"], end_points["rgbd"], end_points["mesh"]
    sa = _soft_args(soft, "match_tail")
    dual = _dual_args(sa, twoway, dual, "match_tail")
    _no_soft_twoway(sa, twoway, "match_tail")

    def run(srows, mrows, mask=None):
        if dual:
            return ops.match_dual_packed(srows, mrows, sa[1], mask, B, N, M, precision, sa[0])
        if twoway:
            return ops.match_twoway_packed(srows, mrows, mask, B, N, M, precision)
        if sa is None:
            return ops.match_packed(srows, mrows, B, N, M, precision)
        return ops.match_soft_packed(srows, mrows, sa[1], B, N, M, precision, sa[0])

    forked = settings.USE_SIDE_STREAMS and seg.is_cuda and not torch.is_grad_enabled() and not twoway and not dual
    mrows = end_points.get("mesh_rows") if precision == ops.MATCH_BF16X3 else None
    srows = end_points.get("scene_rows") if precision == ops.MATCH_BF16X3 else None
    if mrows is None and srows is None:
        srows, mrows = ops.match_pack2(rgbd, mesh[0] if mesh.dim() == 3 else mesh, precision)      # both packs, one launch
    elif srows is None:
        srows = ops.match_pack(rgbd, precision)
    elif mrows is None:
        mrows = ops.match_pack(mesh[0] if mesh.dim() == 3 else mesh, precision)
    if forked:
        with ops.fork(seg.device, 0) as f:                   # side stream 0: behind the segmentation layers, if they are pending there
            f.use(seg)
            mask, count = ops.seg_mask(seg)
        m = run(srows, mrows)
        f.join(mask, count, seg)
    else:
        mask, count = ops.seg_mask(seg)
        m = run(srows, mrows, mask)
    return (mask, count) + tuple(m)


def match_soft_numpy(scene, model, model_xyz, gamma):
    """The soft assignment restated in fp64 (numpy).  scene f32[N,128] raw descriptors (one per row) and model f32[128,M] -- or, in
    place of the descriptors, scene = a similarity matrix [N,M] and model = None.  From descriptors: rows and columns are normalised
    (x / max(|x|, 1e-12)) and sim = rows @ columns.  -> dict(best_idx i64[N] (first maximum on ties), best_sim, lse = log sum_j
    exp(gamma sim_ij), conf = exp(gamma best_sim - lse), soft_xyz [N,3] = softmax(gamma sim) @ model_xyz), all f64."""
    if model is None:
        sim = np.asarray(scene, dtype=np.float64)
    else:
        a = np.asarray(scene, dtype=np.float64)
        b = np.asarray(model, dtype=np.float64)
        a = a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)
        b = b / np.maximum(np.linalg.norm(b, axis=0, keepdims=True), 1e-12)
        sim = a @ b
    xyz = np.asarray(model_xyz, dtype=np.float64)
    g = float(gamma)
    best_idx = sim.argmax(axis=1)                             # numpy returns the first maximum
    best_sim = sim[np.arange(sim.shape[0]), best_idx]
    e = np.exp(g * (sim - best_sim[:, None]))                 # <= 1
    Z = e.sum(axis=1)
    lse = g * best_sim + np.log(Z)
    return dict(best_idx=best_idx, best_sim=best_sim, lse=lse, conf=1.0 / Z, soft_xyz=(e @ xyz) / Z[:, None])


def match_twoway_numpy(scene, model, mask):
    """THE TWO-WAY RULE of include/gdm.h restated in fp64 (numpy) for one crop.  scene f32[N,128] raw descriptors (one per row) and
    model f32[128,M], normalised as in match_soft_numpy -- or scene = a similarity matrix [N,M] (of any float type, compared as it
    is) and model = None; mask [N], nonzero = the point counts for the columns.  -> dict(best_idx i64[N], best_sim [N]: the row
    arg-max over all columns for every row, first maximum on ties; col_idx i64[M], col_sim [M]: per column, from (-1, -inf), a masked
    row takes over iff its similarity is greater -- so the first of equal maxima stays and a NaN never wins)."""
    if model is None:
        sim = np.asarray(scene)
        sim = sim if sim.dtype.kind == "f" else sim.astype(np.float64)
    else:
        a = np.asarray(scene, dtype=np.float64)
        b = np.asarray(model, dtype=np.float64)
        a = a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)
        b = b / np.maximum(np.linalg.norm(b, axis=0, keepdims=True), 1e-12)
        sim = a @ b
    N, M = sim.shape
    keep = np.asarray(mask).reshape(N) != 0
    best_idx = np.zeros(N, dtype=np.int64)
    best_sim = np.full(N, -np.inf, dtype=sim.dtype)
    for j in range(M):                                        # ascending columns, strict '>': the first maximum (running_max)
        take = sim[:, j] > best_sim
        best_idx[take] = j
        best_sim[take] = sim[take, j]
    col_idx = np.full(M, -1, dtype=np.int64)
    col_sim = np.full(M, -np.inf, dtype=sim.dtype)
    for i in np.flatnonzero(keep):                            # ascending rows, strict '>': the lowest row on ties
        take = sim[i] > col_sim
        col_idx[take] = i
        col_sim[take] = sim[i, take]
    return dict(best_idx=best_idx, best_sim=best_sim, col_idx=col_idx, col_sim=col_sim)


def match_dual_numpy(scene, model, model_xyz, mask, gamma):
    """THE DUAL RULE of include/gdm.h restated in fp64 (numpy) for one crop.  scene f32[N,128] raw descriptors and model f32[128,M],
    normalised as in match_soft_numpy -- or scene = a similarity matrix [N,M] and model = None; model_xyz [M,3]; mask [N], nonzero =
    the point counts for the columns; gamma the temperature.  -> match_soft_numpy's five outputs, match_twoway_numpy's col_idx /
    col_sim, and col_lse [M] = log of the sum of exp(gamma sim_ij) over the masked i (-inf where there is none), col_conf [M] =
    exp(gamma col_sim - col_lse) (0 where col_idx = -1), dual [N] = conf_i exp(gamma best_sim_i - col_lse[best_idx_i]) for a masked
    point and 0 for any other, all f64."""
    if model is None:
        sim = np.asarray(scene, dtype=np.float64)
    else:
        a = np.asarray(scene, dtype=np.float64)
        b = np.asarray(model, dtype=np.float64)
        a = a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)
        b = b / np.maximum(np.linalg.norm(b, axis=0, keepdims=True), 1e-12)
        sim = a @ b
    g = float(gamma)
    N, M = sim.shape
    keep = np.asarray(mask).reshape(N) != 0
    out = match_soft_numpy(sim, None, model_xyz, g)
    two = match_twoway_numpy(sim, None, keep)
    col_idx, col_sim = two["col_idx"], two["col_sim"]
    has = col_idx >= 0
    col_lse = np.full(M, -np.inf)
    col_conf = np.zeros(M)
    if keep.any():
        top = sim[keep].max(axis=0)                              # per column: shifted by its own maximum, as the rows are
        col_lse = g * top + np.log(np.exp(g * (sim[keep] - top)).sum(axis=0))
        col_conf[has] = np.exp(g * col_sim[has] - col_lse[has])
    dual = np.zeros(N)
    j = out["best_idx"][keep]
    dual[keep] = out["conf"][keep] * np.exp(g * out["best_sim"][keep] - col_lse[j])
    out.update(col_idx=col_idx, col_sim=col_sim, col_lse=col_lse, col_conf=col_conf, dual=dual)
    return out


def selected(res, b):
    """(obj_pts_idx, max_th) of crop b for the points with seg arg-max == 1, in point order
    (evaluator.py:83-93)."""
    m = res["mask"][b].bool()
    return res["best_idx"][b][m], res["best_sim"][b][m]


def correspondences(res, cld_xyz, model_xyz, b):
    """Scene points and matched model vertices of crop b (evaluator.py:85-99), both [n_sel,3], on the device."""
    m = res["mask"][b].bool()
    return cld_xyz[b][m], model_xyz[res["best_idx"][b][m].long()]
