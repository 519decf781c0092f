"""Batched pose solve on the GPU from the dense correspondences, and the ADD / ADI pose errors.

Mirrors, for a whole batch at once and without leaving the device:
  /root/reference/evaluator.py:60-102 cal_frame_poses  (points with seg arg-max == 1, matched vertex = arg-max column;
      fewer than 5 correspondences -> the sentinel pose [I | (0,0,-1000)])
  /root/reference/utils/pvn3d_eval_utils_kpls.py:43-77 best_fit_transform (Kabsch with the reflection fix)
  /root/reference/lib/pysixd/pose_error.py:297-337 add, adi (ADI's nearest neighbour = the HIP kNN kernel, K=1)
The reference does this on `bs` host threads with numpy (ThreadPoolExecutor, evaluator.py:294-303).
Opt-in robust variants (csrc/gdm_pose_robust.hip), also on the device and capturable in a hipGraph:
  utils/pvn3d_eval_utils_kpls.py:79-124 best_fit_transform_with_RANSAC   solve_poses(method="ransac") / ransac_poses
  utils/pvn3d_eval_utils_kpls.py:126-212 icp (point to point)              refine_icp
and, with no counterpart in the reference, point-to-plane ICP with normal gating and Huber weights: refine_icp_plane.
Consensus fit from pairwise-compatible correspondences (csrc/gdm_consensus.hip; include/gdm.h THE CONSENSUS RULE),
likewise without one: consensus_poses / consensus_poses_numpy, solve_poses(method="consensus").
Verification of pose candidates against the observed depth frame (csrc/gdm_verify.hip), also without one:
  verify_poses / verify_poses_numpy, boxes_to_windows, select_verified, estimate_poses_verified.
Refinement of pose candidates against that frame by render-and-compare (csrc/gdm_refine.hip), likewise:
  refine_poses_depth / refine_poses_depth_numpy, and the "+depth" candidates of estimate_poses_verified.
"""
import numpy as np
import torch

from . import _lib, ops, pixel_rule
from ._lib import call


def _scene_args(cld_rgb_nrm):
    """The (pointer, batch stride, point stride, channel stride) of the xyz rows of cld_rgb_nrm f32[B,9,N]."""
    cld = ops._dev(cld_rgb_nrm, torch.float32, "cld_rgb_nrm")
    return cld, cld.stride(0), 1, cld.shape[2]


def _pose_outputs(B, device):
    """The outputs every fit writes: RT f32[B,3,4] and valid u8[B], uninitialised."""
    return torch.empty((B, 3, 4), dtype=torch.float32, device=device), torch.empty((B,), dtype=torch.uint8, device=device)


def kabsch_stats(res, cld_rgb_nrm, model_xyz):
    """res: matching.match_frames output; cld_rgb_nrm f32[B,9,N] (rows 0-2 = xyz); model_xyz f32[M,3] -> f64[B,16]."""
    mask, best_idx = res["mask"], res["best_idx"]
    B, N = mask.shape
    scene = _scene_args(cld_rgb_nrm)
    model_xyz = ops._dev(model_xyz, torch.float32, "model_xyz")
    out = torch.empty((B, 16), dtype=torch.float64, device=mask.device)
    call("gdm_kabsch_stats_hip", *scene, model_xyz, best_idx, mask, B, N, model_xyz.shape[0], out)
    return out


def solve_poses(res, cld_rgb_nrm, model_xyz, min_points=5, method="kabsch", ransac_iters=20, inlier_dist=0.015, fix_percent=0.7,
                seed=0, weights="none", targets="vertex", consensus_tau=0.005, consensus_seeds=8):
    """-> RT f32[B,3,4] mapping model coordinates to the camera frame, valid bool[B].  Two launches (statistics, fit), no
    host synchronisation.  method="ransac": the reference's RANSAC (ransac_poses) with max_iter = ransac_iters hypotheses,
    match_err = inlier_dist (m) and fix_percent; `seed` selects the hashed samples.  method="consensus": the consensus fit
    (consensus_poses) with consensus_tau, consensus_seeds and inlier_dist.
    method="kabsch" only: weights="conf" weighs every pair by res["conf"], targets="soft" pairs the scene point with
    res["soft_xyz"] instead of its arg-max vertex (both from soft matching, matching.match_frames(soft=...)); weights="dual" weighs
    every pair by res["dual"], the dual-softmax confidence (matching.match_frames(soft=..., dual=True)); each takes the weighted
    entries (solve_poses_weighted).  The defaults are the unweighted launches."""
    if weights not in ("none", "conf", "dual") or targets not in ("vertex", "soft"):
        raise ValueError("solve_poses: weights must be 'none', 'conf' or 'dual' and targets 'vertex' or 'soft', got %r, %r"
                         % (weights, targets))
    soft = weights != "none" or targets != "vertex"
    if method == "ransac":
        if soft:
            raise ValueError("solve_poses: weights=%r / targets=%r are for method='kabsch'; RANSAC keeps the hard pairs" % (weights, targets))
        RT, valid, _, _ = ransac_poses(res, cld_rgb_nrm, model_xyz, ransac_iters, inlier_dist, fix_percent, seed, min_points)
        return RT, valid
    if method == "consensus":
        if soft:
            raise ValueError("solve_poses: weights=%r / targets=%r are for method='kabsch'; the consensus fit keeps the hard pairs"
                             % (weights, targets))
        out = consensus_poses(res, cld_rgb_nrm, model_xyz, consensus_tau, consensus_seeds, inlier_dist, min_points)
        return out["RT"], out["valid"]
    if method != "kabsch":
        raise ValueError("solve_poses: method must be 'kabsch', 'ransac' or 'consensus', got %r" % (method,))
    if soft:
        need = [k for k, on in (("conf", weights == "conf"), ("dual", weights == "dual"), ("soft_xyz", targets == "soft"))
                if on and k not in res]
        if need:
            raise ValueError("solve_poses: weights=%r / targets=%r need the soft matching outputs %s in res" % (weights, targets, need))
        w = res[weights] if weights != "none" else torch.ones(res["mask"].shape, dtype=torch.float32, device=res["mask"].device)
        return solve_poses_weighted(res, cld_rgb_nrm, model_xyz, w, res["soft_xyz"] if targets == "soft" else None, min_points)
    st = kabsch_stats(res, cld_rgb_nrm, model_xyz)
    B = st.shape[0]
    RT, valid = _pose_outputs(B, st.device)
    call("gdm_kabsch_solve_hip", st, B, int(min_points), RT, valid)
    return RT, valid.bool()


def kabsch_stats_weighted(res, cld_rgb_nrm, model_xyz, weight, target=None):
    """The 16 weighted statistics (include/gdm.h gdm_kabsch_stats_w_hip): weight f32[B,N]; the model-side point of a pair is
    target[b, i] (f32[B,N,3]) when given, else model_xyz[best_idx].  -> stats f64[B,16], count i32[B] (masked points with a finite
    weight > 0; the others are skipped)."""
    mask, best_idx = res["mask"], res["best_idx"]
    B, N = mask.shape
    scene = _scene_args(cld_rgb_nrm)
    model_xyz = ops._dev(model_xyz, torch.float32, "model_xyz")
    weight = ops._dev(weight, torch.float32, "weight")
    if tuple(weight.shape) != (B, N):
        raise ValueError("kabsch_stats_weighted: weight is %s, expected %s" % (tuple(weight.shape), (B, N)))
    if target is not None:
        target = ops._dev(target, torch.float32, "target")
        if tuple(target.shape) != (B, N, 3):
            raise ValueError("kabsch_stats_weighted: target is %s, expected %s" % (tuple(target.shape), (B, N, 3)))
    out = torch.empty((B, 16), dtype=torch.float64, device=mask.device)
    count = torch.empty((B,), dtype=torch.int32, device=mask.device)
    call("gdm_kabsch_stats_w_hip", *scene, model_xyz, best_idx, target, weight, mask, B, N, model_xyz.shape[0], out, count)
    return out, count


def solve_poses_weighted(res, cld_rgb_nrm, model_xyz, weight, target=None, min_points=5):
    """The weighted least-squares fit: kabsch_stats_weighted, then the fit with n = sum w.  valid = at least min_points usable pairs
    and sum w > 0, else the sentinel pose.  -> RT f32[B,3,4], valid bool[B].  Two launches, no host synchronisation."""
    st, count = kabsch_stats_weighted(res, cld_rgb_nrm, model_xyz, weight, target)
    B = st.shape[0]
    RT, valid = _pose_outputs(B, st.device)
    call("gdm_kabsch_solve_w_hip", st, count, B, int(min_points), RT, valid)
    return RT, valid.bool()


def kabsch_weighted_numpy(A, B, w):
    """fp64 restatement of the weighted fit: A [n,3] model-side points, B [n,3] scene points, w [n] weights >= 0 -> RT [3,4] with
    B ~ R A + t minimising sum w |R A + t - B|^2 (weighted centroids, SVD of sum w (A - cA)(B - cB)^T, reflection fix as
    best_fit_transform)."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    sw = w.sum()
    cA = (w[:, None] * A).sum(0) / sw
    cB = (w[:, None] * B).sum(0) / sw
    H = (w[:, None] * (A - cA)).T @ (B - cB)
    U, _, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        Vt[2, :] *= -1
        R = Vt.T @ U.T
    return np.concatenate([R, (cB - R @ cA)[:, None]], axis=1)


# ---- the differentiable pose-fit loss (csrc/gdm_poseloss.hip; include/gdm.h THE POSE LOSS RULE) ------------------------
POSE_LOSS = ops._header_enums("GDM_POSE_LOSS_")          # GDM_POSE_LOSS_MAX_S, GDM_POSE_LOSS_REC
POSE_LOSS_STATE = {0: "fitted", 1: "too few usable points (or a ground-truth pose that is not finite)", 2: "ill-conditioned"}


# Registered through torch.library (custom_op + register_autograd) as ops.soft_coord_match is, not as an autograd.Function subclass:
# gdm::pose_loss_fwd is two launches and gdm::pose_loss_bwd one, on the current stream, with no host read and no allocation that
# depends on data, so a hipGraph capture records them like any other operator.  `scene` is the tensor the strides address (rows 0-2 of
# cld_rgb_nrm f32[B,C,N], or f32[B,N,3]); sb / ps / cs are the strides of _scene_args.  sym with S == 0 rows stands for "none".
@torch.library.custom_op("gdm::pose_loss_fwd", mutates_args=(), device_types="cuda")
def _pose_loss_fwd(scene: torch.Tensor, sb: int, ps: int, cs: int, target: torch.Tensor, weight: torch.Tensor, mask: torch.Tensor,
                   RT_gt: torch.Tensor, model_pts: torch.Tensor, sym: torch.Tensor, min_points: int,
                   cond_min: float) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    B, N = weight.shape
    dev = weight.device
    nbytes = call("gdm_pose_loss_record_bytes", B)
    record = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    loss = torch.empty((B,), dtype=torch.float64, device=dev)
    RT = torch.empty((B, 3, 4), dtype=torch.float32, device=dev)
    state = torch.empty((B,), dtype=torch.uint8, device=dev)
    sym_idx = torch.empty((B,), dtype=torch.int32, device=dev)
    S = sym.shape[0]
    call("gdm_pose_loss_fwd_hip", scene, sb, ps, cs, target, weight, mask, RT_gt, model_pts, sym if S else None, B, N, model_pts.shape[0],
         max(S, 1), min_points, cond_min, record, nbytes, loss, RT, state, sym_idx)
    return loss, RT, state, sym_idx, record


@_pose_loss_fwd.register_fake
def _(scene, sb, ps, cs, target, weight, mask, RT_gt, model_pts, sym, min_points, cond_min):
    B = weight.shape[0]
    return (weight.new_empty((B,), dtype=torch.float64), weight.new_empty((B, 3, 4)), weight.new_empty((B,), dtype=torch.uint8),
            weight.new_empty((B,), dtype=torch.int32), weight.new_empty((B * (16 + POSE_LOSS["GDM_POSE_LOSS_REC"]) + (B + 1) // 2,),
                                                                        dtype=torch.float64))


@torch.library.custom_op("gdm::pose_loss_bwd", mutates_args=(), device_types="cuda")
def _pose_loss_bwd(scene: torch.Tensor, sb: int, ps: int, cs: int, target: torch.Tensor, weight: torch.Tensor, mask: torch.Tensor,
                   record: torch.Tensor, grad_loss: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    B, N = weight.shape
    grad_target = torch.empty((B, N, 3), dtype=torch.float32, device=weight.device)
    grad_weight = torch.empty((B, N), dtype=torch.float32, device=weight.device)
    call("gdm_pose_loss_bwd_hip", scene, sb, ps, cs, target, weight, mask, record, record.numel() * 8, grad_loss, B, N, grad_target,
         grad_weight)
    return grad_target, grad_weight


@_pose_loss_bwd.register_fake
def _(scene, sb, ps, cs, target, weight, mask, record, grad_loss):
    return weight.new_empty(tuple(weight.shape) + (3,)), weight.new_empty(tuple(weight.shape))


def _pose_loss_setup(ctx, inputs, output):
    scene, sb, ps, cs, target, weight, mask = inputs[:7]
    ctx.save_for_backward(scene, target, weight, mask, output[4])
    ctx.strides = (sb, ps, cs)
    ctx.set_materialize_grads(False)


def _pose_loss_backward(ctx, g_loss, *unused):
    scene, target, weight, mask, record = ctx.saved_tensors
    if g_loss is None:
        return (None,) * 12
    gt, gw = _pose_loss_bwd(scene, *ctx.strides, target, weight, mask, record, g_loss.to(torch.float64).contiguous())
    return None, None, None, None, gt, gw, None, None, None, None, None, None


_pose_loss_fwd.register_autograd(_pose_loss_backward, setup_context=_pose_loss_setup)


def _pose_loss_scene(scene, B, N, who):
    """The scene of the pose loss as [B,N,3]-addressable: rows 0-2 of f32[B,C>=3,N] (cld_rgb_nrm, no copy) or f32[B,N,3].  A [B,N,3]
    tensor with N == 3 is read as points.  -> (tensor, batch stride, point stride, channel stride, is_rows)."""
    if scene.dim() != 3 or scene.shape[0] != B:
        raise ValueError("%s: the scene must be [B=%d,C>=3,N=%d] or [B,N,3], got %s" % (who, B, N, tuple(scene.shape)))
    if tuple(scene.shape[1:]) == (N, 3):
        return scene, N * 3, 3, 1, False
    if scene.shape[1] >= 3 and scene.shape[2] == N:
        return scene, scene.shape[1] * N, 1, N, True
    raise ValueError("%s: the scene must be [B=%d,C>=3,N=%d] or [B,N,3], got %s" % (who, B, N, tuple(scene.shape)))


def _pose_loss_args(who, scene, target, weight, RT_gt, model_pts, sym, mask):
    """The shape checks the operator and its reference share.  -> B, N, K, S."""
    if target.dim() != 3 or target.shape[2] != 3 or target.shape[0] < 1 or target.shape[1] < 1:
        raise ValueError("%s: target must be [B,N,3], got %s" % (who, tuple(target.shape)))
    B, N = target.shape[:2]
    if tuple(weight.shape) != (B, N):
        raise ValueError("%s: weight is %s, expected %s" % (who, tuple(weight.shape), (B, N)))
    if tuple(RT_gt.shape) != (B, 3, 4):
        raise ValueError("%s: RT_gt is %s, expected %s" % (who, tuple(RT_gt.shape), (B, 3, 4)))
    if model_pts.dim() != 2 or model_pts.shape[1] != 3 or model_pts.shape[0] < 1:
        raise ValueError("%s: model_pts must be [K,3] with K >= 1, got %s" % (who, tuple(model_pts.shape)))
    S = 1
    if sym is not None:
        if sym.dim() != 3 or tuple(sym.shape[1:]) != (3, 4) or not 1 <= sym.shape[0] <= POSE_LOSS["GDM_POSE_LOSS_MAX_S"]:
            raise ValueError("%s: sym must be [S,3,4] with 1 <= S <= %d, got %s" % (who, POSE_LOSS["GDM_POSE_LOSS_MAX_S"], tuple(sym.shape)))
        S = sym.shape[0]
    if mask is not None and tuple(mask.shape) != (B, N):
        raise ValueError("%s: mask is %s, expected %s" % (who, tuple(mask.shape), (B, N)))
    for name, t in (("the scene", scene), ("RT_gt", RT_gt), ("model_pts", model_pts), ("sym", sym)):
        if t is not None and t.requires_grad:
            raise ValueError("%s: a gradient with respect to %s is not offered (detach it); the loss is differentiable in target and "
                             "weight" % (who, name))
    return B, N, model_pts.shape[0], S


def sym_transforms(syms, device=None, dtype=torch.float32):
    """evaluation.symmetry_transformations' list of {"R": [3,3], "t": [3,1]} (call it with scale=0.001: metres) -> [S,3,4]."""
    out = np.stack([np.concatenate([np.asarray(s["R"], np.float64).reshape(3, 3), np.asarray(s["t"], np.float64).reshape(3, 1)], axis=1)
                    for s in syms])
    return torch.as_tensor(out, dtype=dtype, device=device)


def kabsch_pose_loss(cld_rgb_nrm_or_scene, target, weight, RT_gt, model_pts, sym=None, mask=None, min_points=5, cond_min=1e-3,
                     loss_dtype=torch.float32):
    """The differentiable pose-fit loss (include/gdm.h THE POSE LOSS RULE; csrc/gdm_poseloss.hip): per crop, the weighted Kabsch fit of
    the scene points onto target f32[B,N,3] (model side, e.g. the soft vertices of ops.soft_coord_match) under weight f32[B,N], and
    the mean distance of the K model points model_pts f32[K,3] between that pose and RT_gt f32[B,3,4] -- the minimum over the symmetry
    transforms sym f32[S,3,4] (sym_transforms; None = the identity alone).  The scene is cld_rgb_nrm f32[B,C>=3,N] (rows 0-2, no copy)
    or f32[B,N,3]; mask u8/bool[B,N] (None = every point).  Points with mask 0 or a weight that is NaN, infinite, zero or negative are
    skipped.  -> loss [B] (loss_dtype; the kernels' own f64 rounded once), RT f32[B,3,4] (solve_poses_weighted's, bit for bit), state
    u8[B] (POSE_LOSS_STATE; a crop that is not 0 has loss 0 and no gradient), sym_idx i32[B] (the winning transform, -1 when not
    fitted).  loss is differentiable in target and weight (own kernels, no SVD); the rest is detached.  A gradient with respect to
    the scene, RT_gt, model_pts or sym is not offered: a tensor that requires one raises.  Two launches forward and one backward, no
    host synchronisation."""
    who = "kabsch_pose_loss"
    B, N, K, S = _pose_loss_args(who, cld_rgb_nrm_or_scene, target, weight, RT_gt, model_pts, sym, mask)
    target = ops._dev(target, torch.float32, "target")
    weight = ops._dev(weight, torch.float32, "weight")
    scene, sb, ps, cs, _ = _pose_loss_scene(ops._dev(cld_rgb_nrm_or_scene, torch.float32, "scene"), B, N, who)
    RT_gt = ops._dev(RT_gt, torch.float32, "RT_gt")
    model_pts = ops._dev(model_pts, torch.float32, "model_pts")
    sym = torch.empty((0, 3, 4), dtype=torch.float32, device=target.device) if sym is None else ops._dev(sym, torch.float32, "sym")
    if mask is None:
        mask = torch.ones((B, N), dtype=torch.uint8, device=target.device)
    else:
        mask = ops._dev(mask if mask.dtype == torch.uint8 else mask.to(torch.uint8), torch.uint8, "mask")
    if not 0.0 <= float(cond_min) < 1.0:
        raise ValueError("%s: cond_min=%r not in [0, 1)" % (who, cond_min))
    loss, RT, state, sym_idx, _ = _pose_loss_fwd(scene, sb, ps, cs, target, weight, mask, RT_gt, model_pts, sym, int(min_points),
                                                 float(cond_min))
    return loss.to(loss_dtype), RT.detach(), state.detach(), sym_idx.detach()


def kabsch_pose_loss_reference(cld_rgb_nrm_or_scene, target, weight, RT_gt, model_pts, sym=None, mask=None, min_points=5, cond_min=1e-3):
    """THE POSE LOSS RULE in plain torch, any dtype (target's) and device: torch.linalg.svd with the reflection fix of
    kabsch_weighted_numpy, and autograd supplies the gradient.  Same arguments, skip rule, states and outputs as kabsch_pose_loss
    (loss in target's dtype).  What the kernels are held to; an explicit choice (loss.PoseFitLoss(match="reference")), never a
    fall-back."""
    who = "kabsch_pose_loss_reference"
    B, N, K, S = _pose_loss_args(who, cld_rgb_nrm_or_scene, target, weight, RT_gt, model_pts, sym, mask)
    dt, dev = target.dtype, target.device
    scene, _, _, _, rows = _pose_loss_scene(cld_rgb_nrm_or_scene, B, N, who)
    scene = (scene[:, :3, :].transpose(1, 2) if rows else scene).to(dt)
    weight = weight.to(dt)
    gt = RT_gt.to(dt)
    X = model_pts.to(dt)
    sym = torch.eye(3, 4, dtype=dt, device=dev)[None] if sym is None else sym.to(dt)
    usable = torch.isfinite(weight) & (weight > 0)
    if mask is not None:
        usable = usable & (mask != 0)
    losses, RTs = [], []
    state = torch.zeros(B, dtype=torch.uint8, device=dev)
    sym_idx = torch.full((B,), -1, dtype=torch.int32, device=dev)
    sentinel = torch.as_tensor(SENTINEL_RT, dtype=torch.float32, device=dev)
    for b in range(B):
        u = usable[b]
        w = weight[b][u]
        W = w.sum()
        if int(u.sum()) < int(min_points) or not float(W.detach()) > 0:
            state[b] = 1
            losses.append(torch.zeros((), dtype=dt, device=dev))
            RTs.append(sentinel)
            continue
        A, Bp = target[b][u], scene[b][u]
        cA = (w[:, None] * A).sum(0) / W
        cB = (w[:, None] * Bp).sum(0) / W
        H = (w[:, None] * (A - cA)).t() @ (Bp - cB)
        U, sv, Vt = torch.linalg.svd(H)
        sign = 1.0
        if float(torch.linalg.det((Vt.t() @ U.t()).detach())) < 0:                  # the reflection fix: the last row of V^T negated
            Vt = Vt * torch.tensor([1.0, 1.0, -1.0], dtype=dt, device=dev)[:, None]
            sign = -1.0
        R = Vt.t() @ U.t()
        t = cB - R @ cA
        RTs.append(torch.cat([R, t[:, None]], dim=1).detach().float())
        s1, s2, s3 = (float(v) for v in sv.detach())
        if not bool(torch.isfinite(gt[b]).all()):
            state[b] = 1
        elif not (s2 + sign * s3) > float(cond_min) * s1:                # the eigenvalues of sym(R H) are s1, s2, sign * s3
            state[b] = 2
        if int(state[b]) != 0:
            losses.append(torch.zeros((), dtype=dt, device=dev))
            continue
        pred = X @ R.t() + t
        best = None
        for s in range(sym.shape[0]):
            want = (X @ sym[s, :, :3].t() + sym[s, :, 3]) @ gt[b, :, :3].t() + gt[b, :, 3]
            D = torch.linalg.norm(pred - want, dim=1).mean()
            if best is None or float(D.detach()) < float(best.detach()):                 # the lowest s wins a tie
                best = D
                sym_idx[b] = s
        losses.append(best)
    return torch.stack(losses), torch.stack(RTs), state, sym_idx


def _mix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def ransac_sample_indices(counts, H, seed=0):
    """The RANSAC samples of include/gdm.h, restated on the CPU (numpy): counts = the selected-pair count n of every crop [B] ->
    i64[B,H,4], row h = the 4 indices (into the crop's selected pairs, in point order) that hypothesis h fits; row 0 (the fit of all
    pairs, no draw) is -1.  mix = lowbias32; r = mix(mix(mix(seed ^ 0x9e3779b9) ^ b) ^ (4 h + s)); index = (uint64(r) * n) >> 32."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    B = counts.shape[0]
    with np.errstate(over="ignore"):
        b = np.arange(B, dtype=np.uint32)[:, None, None]
        hs = (4 * np.arange(H, dtype=np.uint32)[None, :, None] + np.arange(4, dtype=np.uint32)[None, None, :]).astype(np.uint32)
        r = _mix32(_mix32(_mix32(np.uint32(seed & 0xffffffff) ^ np.uint32(0x9e3779b9)) ^ b) ^ hs)
    idx = ((r.astype(np.uint64) * counts.astype(np.uint64)[:, None, None]) >> np.uint64(32)).astype(np.int64)
    idx[:, 0, :] = -1
    return idx


def ransac_poses(res, cld_rgb_nrm, model_xyz, iters=20, inlier_dist=0.015, fix_percent=0.7, seed=0, min_points=5):
    """Batched best_fit_transform_with_RANSAC (pvn3d_eval_utils_kpls.py:79-124; include/gdm.h gdm_ransac_pose_hip) over the same
    correspondences as solve_poses.  -> RT f32[B,3,4], valid bool[B], counts i32[B,iters] (inliers of every hypothesis), winner
    i32[B] (the hypothesis that decided, -1 for the sentinel).  Five launches, no host synchronisation."""
    H = int(iters)
    if not 1 <= H <= _lib.GDM_RANSAC_MAX_H:
        raise ValueError("ransac_poses: iters=%d not in [1, %d]" % (H, _lib.GDM_RANSAC_MAX_H))
    mask, best_idx = res["mask"], res["best_idx"]
    B, N = mask.shape
    st = kabsch_stats(res, cld_rgb_nrm, model_xyz)
    cld, sb, ps, cs = _scene_args(cld_rgb_nrm)
    model_xyz = ops._dev(model_xyz, torch.float32, "model_xyz")
    L = _lib.lib()
    nbytes = int(L.gdm_ransac_workspace_bytes(B, N, H))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=mask.device)
    RT, valid = _pose_outputs(B, mask.device)
    counts = torch.empty((B, H), dtype=torch.int32, device=mask.device)
    winner = torch.empty((B,), dtype=torch.int32, device=mask.device)
    call("gdm_ransac_pose_hip", cld, sb, ps, cs, model_xyz, best_idx, mask, st, B, N, model_xyz.shape[0], H, float(inlier_dist),
         float(fix_percent), int(seed) & 0xffffffff, int(min_points), ws, nbytes, RT, valid, counts, winner)
    return RT, valid.bool(), counts, winner


CONSENSUS_MAX_POINTS = 4096    # N of gdm_consensus_pose_hip: a bit row is held one 64-bit word per lane
CONSENSUS_MAX_SEEDS = 64


def consensus_poses(res, cld_rgb_nrm, model_xyz, tau=0.005, seeds=8, inlier_dist=0.015, min_points=5):
    """The consensus fit (include/gdm.h THE CONSENSUS RULE, gdm_consensus_pose_hip) over the same correspondences as
    solve_poses: pairs whose scene and model distances agree within tau (m) are compatible; the pairs with the most second-order
    support seed `seeds` weighted fits, the one with the most pairs within inlier_dist (m) wins and is refit on them.  tau, seeds and
    inlier_dist are the defaults of a definition, not tuned values.  -> dict(RT f32[B,3,4], valid bool[B], score / degree i32[B,N]
    (per point, -1 where unselected), seed_idx i32[B,seeds] (point indices, -1 unused), hyp_RT f32[B,seeds,3,4], counts i32[B,seeds]
    (-1 for a skipped hypothesis), winner i32[B]).  Six launches, no host synchronisation; the only temporary is the planner's
    workspace, which holds an n x n bit matrix per crop (512 KiB at N = 2048) and no n x n float tensor."""
    S = int(seeds)
    mask, best_idx = res["mask"], res["best_idx"]
    B, N = mask.shape
    if not 1 <= S <= CONSENSUS_MAX_SEEDS:
        raise ValueError("consensus_poses: seeds=%d not in [1, %d]" % (S, CONSENSUS_MAX_SEEDS))
    if N > CONSENSUS_MAX_POINTS:
        raise ValueError("consensus_poses: N=%d > %d points per crop" % (N, CONSENSUS_MAX_POINTS))
    if int(min_points) < 3:
        raise ValueError("consensus_poses: min_points=%d must be >= 3" % int(min_points))
    cld, sb, ps, cs = _scene_args(cld_rgb_nrm)
    model_xyz = ops._dev(model_xyz, torch.float32, "model_xyz")
    dev = mask.device
    nbytes = call("gdm_consensus_workspace_bytes", B, N, S)
    if nbytes == 0:
        raise ValueError("consensus_poses: B=%d N=%d seeds=%d is beyond the entry's limits (include/gdm.h)" % (B, N, S))
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
    RT, valid = _pose_outputs(B, dev)
    out = dict(RT=RT, valid=valid,
               score=torch.empty((B, N), dtype=torch.int32, device=dev), degree=torch.empty((B, N), dtype=torch.int32, device=dev),
               seed_idx=torch.empty((B, S), dtype=torch.int32, device=dev),
               hyp_RT=torch.empty((B, S, 3, 4), dtype=torch.float32, device=dev),
               counts=torch.empty((B, S), dtype=torch.int32, device=dev), winner=torch.empty((B,), dtype=torch.int32, device=dev))
    call("gdm_consensus_pose_hip", cld, sb, ps, cs, model_xyz, best_idx, mask, B, N, model_xyz.shape[0], S, float(tau),
         float(inlier_dist), int(min_points), ws, nbytes, out["RT"], out["valid"], out["score"], out["degree"], out["seed_idx"],
         out["hyp_RT"], out["counts"], out["winner"])
    out["valid"] = out["valid"].bool()
    return out


def consensus_bits_numpy(p, q, tau):
    """Step 1 of THE CONSENSUS RULE in np.float32 operations in the written order: p, q [n,3] -> C bool[n,n]."""
    p, q = np.asarray(p, np.float32), np.asarray(q, np.float32)

    def dist2(x):
        d = x[:, None, :] - x[None, :, :]
        return ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]

    a2, b2 = dist2(p), dist2(q)
    u = (a2 + b2) - np.float32(tau) * np.float32(tau)
    with np.errstate(over="ignore", invalid="ignore"):
        C = (u <= np.float32(0)) | (u * u <= (np.float32(4) * a2) * b2)
    np.fill_diagonal(C, False)
    return C


SENTINEL_RT = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -1000]], np.float64)


def consensus_poses_numpy(scene, model_pts, mask, tau=0.005, seeds=8, inlier_dist=0.015, min_points=5, near_margin=1e-5):
    """consensus_poses for ONE crop on the host, the definition the kernels are tested against.  scene [N,3] and model_pts [N,3] (the
    matched vertex of every point, already clamped and gathered) as fp32, mask [N].  The bits come from consensus_bits_numpy; the
    intersections from a float64 product of 0/1 matrices, which is exact; the fits from kabsch_weighted_numpy and the residuals in fp64.
    -> dict(RT f64[3,4], valid, score / degree i64[N] (-1 unselected), seed_idx i64[S], hyp_RT f64[S,3,4], counts i64[S], winner;
    and for the tests: sel i64[n], C bool[n,n], weights f64[S,n] (compacted order, 0 = not in the fit), near i64[S] (pairs within
    near_margin of inlier_dist under hypothesis t), inliers bool[n] of the winner)."""
    scene, model_pts = np.asarray(scene, np.float32), np.asarray(model_pts, np.float32)
    N, S = len(scene), int(seeds)
    sel = np.nonzero(np.asarray(mask).reshape(-1) != 0)[0]
    n = len(sel)
    p, q = scene[sel], model_pts[sel]
    C = consensus_bits_numpy(p, q, tau)
    Cf = C.astype(np.float64)
    common = Cf @ Cf                                                       # |row_i & row_j|: sums of at most n ones, exact
    deg = C.sum(1).astype(np.int64)
    s = np.rint((common * Cf).sum(1)).astype(np.int64)
    score, degree = np.full(N, -1, np.int64), np.full(N, -1, np.int64)
    score[sel], degree[sel] = s, deg
    covered = np.zeros(n, bool)
    seedk = np.full(S, -1, np.int64)
    for t in range(S):
        cand = np.where(~covered & (s > 0), s, 0)
        if n == 0 or cand.max() <= 0:
            break
        g = int(np.argmax(cand))                                           # the first maximum: the smallest k on a tie
        seedk[t] = g
        covered |= C[g]
        covered[g] = True
    p64, q64 = p.astype(np.float64), q.astype(np.float64)
    hyp = np.tile(SENTINEL_RT, (S, 1, 1))
    counts, near = np.full(S, -1, np.int64), np.zeros(S, np.int64)
    weights = np.zeros((S, n))
    resid = np.zeros((S, n))
    for t in range(S):
        g = seedk[t]
        if g < 0:
            continue
        w = np.rint(common[g] * Cf[g])
        w[g] = deg[g]
        pos = w > 0
        if pos.sum() < 3:
            continue
        weights[t] = w
        hyp[t] = kabsch_weighted_numpy(q64[pos], p64[pos], w[pos])
        resid[t] = np.linalg.norm(q64 @ hyp[t][:, :3].T + hyp[t][:, 3] - p64, axis=1)
        counts[t] = int((resid[t] <= inlier_dist).sum())
        near[t] = int((np.abs(resid[t] - inlier_dist) < near_margin).sum())
    seed_idx = np.where(seedk >= 0, sel[np.clip(seedk, 0, max(n - 1, 0))] if n else -1, -1)
    out = dict(RT=SENTINEL_RT.copy(), valid=False, score=score, degree=degree, seed_idx=seed_idx, hyp_RT=hyp, counts=counts, winner=-1,
               sel=sel, C=C, weights=weights, near=near, inliers=np.zeros(n, bool))
    win = int(np.argmax(counts)) if S else -1
    if n >= min_points and win >= 0 and counts[win] >= min_points:
        inl = resid[win] <= inlier_dist
        out.update(RT=kabsch_weighted_numpy(q64[inl], p64[inl], np.ones(int(inl.sum()))), valid=True, winner=win, inliers=inl)
    return out


def _icp_setup(RT, valid, cld_rgb_nrm, mask, model_xyz):
    """What the two ICP forms share: the checked inputs (RT and the active flags as new tensors), the K = 1 result buffers nn i32[B,N,1]
    and d2 f32[B,N,1], and search(), which enqueues one iteration's transform of the scene points into the model frame and their exact
    nearest-vertex search, and returns the transformed points f32[B,N,3].
    -> (cld, batch stride, point stride, channel stride), model_xyz, mask, RT, active, nn, d2, search."""
    B, N = mask.shape
    dev = mask.device
    scene = _scene_args(cld_rgb_nrm)
    model_xyz = ops._dev(model_xyz, torch.float32, "model_xyz")
    mask = mask if mask.dtype == torch.uint8 else mask.to(torch.uint8)
    mask = ops._dev(mask, torch.uint8, "mask")
    RT = ops._dev(RT, torch.float32, "RT").clone()
    active = valid.to(torch.uint8).contiguous().clone()
    query = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    nn = torch.empty((B, N, 1), dtype=torch.int32, device=dev)
    d2 = torch.empty((B, N, 1), dtype=torch.float32, device=dev)
    job = (_lib.KnnJob * 1)()
    job[0].support, job[0].query, job[0].idx, job[0].d2 = model_xyz.data_ptr(), query.data_ptr(), nn.data_ptr(), d2.data_ptr()
    job[0].support_bstride, job[0].query_bstride = 0, N * 3
    job[0].S, job[0].Q, job[0].K, job[0].grid_w = model_xyz.shape[0], N, 1, 0

    def search():
        call("gdm_icp_transform_hip", *scene, RT, B, N, query)
        call("gdm_knn_jobs_ws_hip", job, 1, B, None, 0)
        return query

    return scene, model_xyz, mask, RT, active, nn, d2, search


def refine_icp(RT, valid, cld_rgb_nrm, mask, model_xyz, iters=20, tolerance=0.001, reject_dist=None, min_points=5):
    """Point-to-point ICP from the poses RT f32[B,3,4] (pvn3d_eval_utils_kpls.py:126-212, run scene -> model: the selected scene
    points (mask u8/bool [B,N]) are mapped into the model frame, matched to their nearest model vertex by the exact kNN (K = 1, one
    model cloud f32[M,3] shared by every crop) and the absolute pose is refit from those pairs; pairs farther than reject_dist (m)
    are dropped when it is given).  Exactly `iters` iterations are enqueued (the step captures in a hipGraph); a crop stops on the
    device by the reference's rule (|prev_error - mean| < tolerance, prev_error starting at 0), or when it is invalid or has fewer
    than min_points pairs.  -> RT f32[B,3,4] (a new tensor), iterations run i32[B], final mean residual f32[B] (the mean pair
    distance of the last iteration run; 0 for a crop that ran none)."""
    scene, model_xyz, mask, RT, active, nn, d2, search = _icp_setup(RT, valid, cld_rgb_nrm, mask, model_xyz)
    B, N = mask.shape
    n_iter = torch.zeros((B,), dtype=torch.int32, device=mask.device)
    err = torch.zeros((B,), dtype=torch.float64, device=mask.device)
    reject = -1.0 if reject_dist is None else float(reject_dist)
    for _ in range(int(iters)):
        search()
        call("gdm_icp_update_hip", *scene, model_xyz, nn, d2, mask, B, N, model_xyz.shape[0], reject, float(tolerance), int(min_points), RT,
             active, n_iter, err)
    return RT, n_iter, err.float()


ICP_STATUS = {0: "running or never run", 1: "converged", 2: "starved", 3: "degenerate"}


def refine_icp_plane(RT, valid, cld_rgb_nrm, mask, model_xyz, model_nrm, iters=10, tolerance=1e-4, reject_dist=None, normal_gate=None,
                     huber=None, min_points=6, pivot_min=1e-6):
    """Point-to-plane ICP from the poses RT f32[B,3,4] (include/gdm.h gdm_icp_plane_update_hip): refine_icp's transform
    and exact K = 1 search, then one Gauss-Newton step per crop on n . (x - q) with the model's unit normals model_nrm f32[M,3].
    reject_dist (m) drops far pairs, normal_gate (a cosine) drops pairs whose scene normal (rows 6..8 of cld_rgb_nrm, turned into the
    model frame) and model normal agree less than that, huber (m) down-weights residuals above it; None turns each off.  Exactly
    `iters` iterations are enqueued, with no host synchronisation (the step captures in a hipGraph).  A crop stops on the device when
    it converges (|prev_mean - mean| < tolerance, status 1), has fewer than max(min_points, 6) pairs (2) or is degenerate (3: a
    plane, a sphere, a body of revolution; the unit-free pivot test of DESIGN.md 6b) -- in the last two cases with its pose unchanged.
    -> RT f32[B,3,4] (a new tensor), iterations run i32[B], final mean |n . (x - q)| f32[B], status i32[B]."""
    scene, model_xyz, mask, RT, active, nn, d2, search = _icp_setup(RT, valid, cld_rgb_nrm, mask, model_xyz)
    cld, _, _, cs = scene
    B, N = mask.shape
    M = model_xyz.shape[0]
    model_nrm = ops._dev(model_nrm, torch.float32, "model_nrm")
    if tuple(model_nrm.shape) != (M, 3):
        raise ValueError("refine_icp_plane: model_nrm is %s, expected %s" % (tuple(model_nrm.shape), (M, 3)))
    if normal_gate is not None and cld.shape[1] < 9:
        raise ValueError("refine_icp_plane: normal_gate needs the scene normals in rows 6..8 of cld_rgb_nrm")
    n_iter = torch.zeros((B,), dtype=torch.int32, device=mask.device)
    status = torch.zeros((B,), dtype=torch.int32, device=mask.device)
    err = torch.zeros((B,), dtype=torch.float64, device=mask.device)
    reject = -1.0 if reject_dist is None else float(reject_dist)
    snrm = None if normal_gate is None else cld.data_ptr() + 6 * cs * cld.element_size()
    gate = 0.0 if normal_gate is None else float(normal_gate)
    delta = 0.0 if huber is None else float(huber)
    for _ in range(int(iters)):
        query = search()
        call("gdm_icp_plane_update_hip", snrm, *scene[1:], query, model_xyz, model_nrm, nn, d2, mask, B, N, M, reject, gate, delta,
             float(tolerance), int(min_points), float(pivot_min), RT, active, n_iter, err, status, None)
    return RT, n_iter, err.float(), status


def _nearest_two(query, model, chunk=512):
    """The two nearest model vertices of every query row by brute force, in chunks: the four best candidates by the expanded form
    |q|^2 - 2 q.m + |m|^2 (one matrix product), then their distances as sqrt(sum (q - m)^2) in fp64, which decide.
    -> nn i64[n], d1 f64[n], d2nd f64[n] (distances; inf without a second vertex)."""
    n, M = len(query), len(model)
    k = min(4, M)
    nn = np.zeros(n, np.int64)
    d1, d2nd = np.zeros(n), np.full(n, np.inf)
    m2 = (model * model).sum(1)
    for s in range(0, n, chunk):
        q = query[s:s + chunk]
        approx = (q * q).sum(1)[:, None] - 2.0 * (q @ model.T) + m2[None, :]
        cand = np.argpartition(approx, k - 1, axis=1)[:, :k] if k < M else np.tile(np.arange(M), (len(q), 1))
        cand.sort(axis=1)                                            # ties go to the lowest index
        dd = np.sqrt(((q[:, None, :] - model[cand]) ** 2).sum(2))
        order = np.argsort(dd, axis=1, kind="stable")
        r = np.arange(len(q))
        nn[s:s + chunk], d1[s:s + chunk] = cand[r, order[:, 0]], dd[r, order[:, 0]]
        if k > 1:
            d2nd[s:s + chunk] = dd[r, order[:, 1]]
    return nn, d1, d2nd


def icp_plane_solve_numpy(A, g, S, L2, R, t, pivot_min=1e-6):
    """fp64 restatement of csrc/gdm_icp_plane_solve.inc: A [6,6], g [6], S = sum w, L2 = sum w |x|^2, pose (R [3,3], t [3]) ->
    dict degenerate, min_pivot (smallest Cholesky pivot L_kk^2 of D A D / S reached), xi [6], R, t (new; the old ones when degenerate)."""
    A, g = np.asarray(A, np.float64), np.asarray(g, np.float64)
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    out = dict(degenerate=True, min_pivot=np.inf, xi=np.zeros(6), R=R.copy(), t=t.copy())
    l2 = L2 / S if S != 0 else np.nan
    if not l2 > 0.0:
        return out
    D = np.array([1.0 / np.sqrt(l2)] * 3 + [1.0] * 3)
    Ah = A * D[:, None] * D[None, :] / S
    L = np.zeros((6, 6))
    for k in range(6):
        p = Ah[k, k] - (L[k, :k] ** 2).sum()
        out["min_pivot"] = min(out["min_pivot"], p)
        if not p >= pivot_min:
            return out
        L[k, k] = np.sqrt(p)
        for i in range(k + 1, 6):
            L[i, k] = (Ah[i, k] - (L[i, :k] * L[k, :k]).sum()) / L[k, k]
    y = np.linalg.solve(L.T, np.linalg.solve(L, -g * D / S))
    xi = y * D
    w, v = xi[:3], xi[3:]
    th = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    Ri = np.eye(3) + K if th < 1e-8 else np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / (th * th) * (K @ K)
    Rn = R @ Ri.T
    out.update(degenerate=False, xi=xi, R=Rn, t=t - Rn @ v)
    return out


def icp_plane_step_numpy(scene, scene_nrm, model_xyz, model_nrm, RT, mask=None, reject_dist=None, normal_gate=None, huber=None,
                         min_points=6, pivot_min=1e-6, nn=None, d2=None, margin=1e-6):
    """One point-to-plane iteration (include/gdm.h gdm_icp_plane_update_hip) restated in fp64 numpy.  scene [N,3] and scene_nrm [N,3]
    (None without a gate) in the camera frame, model_xyz / model_nrm [M,3], RT [3,4] (model -> camera), mask [N].  The pairs come from a
    brute-force nearest-vertex search of x = R^T (s - t), or from nn [N] / d2 [N] (squared distances, compared in fp32 as the kernel
    does) when given -- the device's search, so that a near tie between two vertices cannot part the two computations.
    -> dict RT [3,4] (new; unchanged when status != 0), status (0, 2 starved, 3 degenerate), n (pairs kept), mean (mean |r|), xi,
    min_pivot, keep bool[N], rows (sqrt(w) J [n,6]) and rhs (sqrt(w) r [n]) of the kept pairs, w, r, nn_ref / dist_ref (the brute-force
    search), ties (masked queries whose two nearest vertices are within `margin`), near_reject / near_gate (masked pairs within
    `margin` of the reject distance / gate cosine)."""
    scene, model_xyz, model_nrm = (np.asarray(a, np.float64) for a in (scene, model_xyz, model_nrm))
    RT = np.asarray(RT, np.float64)
    R, t = RT[:, :3], RT[:, 3]
    N, M = len(scene), len(model_xyz)
    sel = np.ones(N, bool) if mask is None else np.asarray(mask) != 0
    x = (scene - t) @ R
    nn_ref, dist_ref, dist_2nd = _nearest_two(x, model_xyz)
    ties = int((sel & (dist_2nd - dist_ref < margin)).sum())
    if nn is None:
        j, dist = nn_ref, dist_ref
        far = np.zeros(N, bool) if reject_dist is None else dist * dist > float(reject_dist) ** 2
    else:
        j = np.clip(np.asarray(nn, np.int64).reshape(N), 0, M - 1)
        dd = np.maximum(np.asarray(d2, np.float32).reshape(N), np.float32(0))
        dist = np.sqrt(dd.astype(np.float64))
        far = np.zeros(N, bool) if reject_dist is None else ~(dd <= np.float32(reject_dist) * np.float32(reject_dist))
    near_reject = 0 if reject_dist is None else int((sel & (np.abs(dist - float(reject_dist)) < margin)).sum())
    q, n = model_xyz[j], model_nrm[j]
    keep = sel & ~far
    near_gate = 0
    if normal_gate is not None:
        cosang = ((np.asarray(scene_nrm, np.float64) @ R) * n).sum(1)
        near_gate = int((keep & (np.abs(cosang - float(normal_gate)) < margin)).sum())
        keep &= cosang >= float(normal_gate)
    x, q, n = x[keep], q[keep], n[keep]
    r = (n * (x - q)).sum(1)
    ar = np.abs(r)
    w = np.ones_like(r)
    if huber is not None and huber > 0:
        big = ar > huber
        w[big] = huber / ar[big]
    J = np.concatenate([np.cross(x, n), n], axis=1)
    out = dict(RT=RT.copy(), status=0, n=int(keep.sum()), mean=float(ar.mean()) if len(r) else 0.0, xi=np.zeros(6), min_pivot=np.inf,
               keep=keep, rows=np.sqrt(w)[:, None] * J, rhs=np.sqrt(w) * r, w=w, r=r, nn_ref=nn_ref, dist_ref=dist_ref, ties=ties,
               near_reject=near_reject, near_gate=near_gate)
    if out["n"] < max(int(min_points), 6):
        out["status"] = 2
        return out
    sol = icp_plane_solve_numpy((w[:, None] * J).T @ J, (w[:, None] * J).T @ r, w.sum(), (w * (x * x).sum(1)).sum(), R, t, pivot_min)
    out["min_pivot"] = sol["min_pivot"]
    if sol["degenerate"]:
        out["status"] = 3
        return out
    out["xi"] = sol["xi"]
    out["RT"] = np.concatenate([sol["R"], sol["t"][:, None]], axis=1)
    return out


def icp_plane_numpy(scene, scene_nrm, model_xyz, model_nrm, RT0, mask=None, iters=10, tolerance=1e-4, reject_dist=None,
                    normal_gate=None, huber=None, min_points=6, pivot_min=1e-6, fp32_pose=True):
    """refine_icp_plane for one crop, free-running, in fp64 numpy: icp_plane_step_numpy with its own search, the pose rounded to fp32
    after every update as the kernel stores it (fp32_pose), and the stop rule.  -> dict RT, iters, status (0 ran out of iterations,
    1 converged, 2 starved, 3 degenerate), resid (mean |r| of the last iteration run), and per iteration run: n, mean, min_pivot, ties,
    near_reject, near_gate, stop_margin (| |prev - mean| - tolerance |), RTs."""
    RT = np.asarray(RT0, np.float64).copy()
    out = dict(status=0, iters=0, resid=0.0, n=[], mean=[], min_pivot=[], ties=[], near_reject=[], near_gate=[], stop_margin=[], RTs=[])
    prev = 0.0
    for _ in range(int(iters)):
        s = icp_plane_step_numpy(scene, scene_nrm, model_xyz, model_nrm, RT, mask, reject_dist, normal_gate, huber, min_points, pivot_min)
        if s["status"] != 0:
            out["status"] = s["status"]
            break
        RT = s["RT"].astype(np.float32).astype(np.float64) if fp32_pose else s["RT"]
        out["iters"] += 1
        out["resid"] = s["mean"]
        for k in ("n", "mean", "min_pivot", "ties", "near_reject", "near_gate"):
            out[k].append(s[k])
        out["stop_margin"].append(abs(abs(prev - s["mean"]) - tolerance))
        out["RTs"].append(RT)
        if abs(prev - s["mean"]) < tolerance:
            out["status"] = 1
            break
        prev = s["mean"]
    out["RT"] = RT
    return out


CYCLE_RADIUS = 0.005          # m: the default of the cycle filter's definition, not a tuned value


def cycle_filter(res, cld_rgb_nrm, radius=CYCLE_RADIUS):
    """The cycle-consistency pair filter (include/gdm.h THE CYCLE RULE) on a two-way match res (matching.match_frames(twoway=True):
    mask, best_idx, col_idx): a masked point stays iff the point its matched vertex picks back lies within `radius` of it.
    -> (pair_mask u8[B,N], pair_count i32[B], cycle_d2 f32[B,N]).  One launch, no host synchronisation."""
    if "col_idx" not in res:
        raise ValueError("cycle_filter: res has no col_idx (match with twoway=True, or with soft and dual=True)")
    return ops.match_cycle(cld_rgb_nrm, res["best_idx"], res["col_idx"], res["mask"], radius)


def cycle_filter_numpy(xyz, best_idx, col_idx, mask, radius=CYCLE_RADIUS):
    """THE CYCLE RULE restated in fp32, operation for operation, for one crop: xyz f32[N,3], best_idx [N], col_idx [M], mask [N].
    -> (pair_mask u8[N], pair_count int, cycle_d2 f32[N])."""
    f = np.float32
    p = np.asarray(xyz, dtype=f)
    bi, ci, mk = np.asarray(best_idx), np.asarray(col_idx), np.asarray(mask)
    N, M = p.shape[0], ci.shape[0]
    r = f(radius)
    if not (np.isfinite(r) and r >= 0):
        raise ValueError("cycle_filter_numpy: radius=%r must be finite and >= 0" % (radius,))
    with np.errstate(over="ignore", invalid="ignore"):
        r2 = r * r
        pair = np.zeros(N, dtype=np.uint8)
        d2 = np.full(N, np.inf, dtype=f)
        for i in range(N):
            if not mk[i]:
                continue
            j = int(bi[i])
            k = int(ci[j]) if 0 <= j < M else -1
            if not 0 <= k < N:
                continue
            dx, dy, dz = f(p[i, 0] - p[k, 0]), f(p[i, 1] - p[k, 1]), f(p[i, 2] - p[k, 2])
            d2[i] = f(f(f(dx * dx) + f(dy * dy)) + f(dz * dz))
            pair[i] = 1 if d2[i] <= r2 else 0
    return pair, int(pair.sum()), d2


def _pair_filter(o, res, cld_rgb_nrm, who):
    """pose_opts' pair_filter / cycle_radius -> (the res the fit sees, the outputs the filter adds)."""
    kind = o.get("pair_filter", "none")
    if kind not in ("none", "cycle"):
        raise ValueError("%s: pair_filter must be 'none' or 'cycle', got %r" % (who, kind))
    if kind == "none":
        if "cycle_radius" in o:
            raise ValueError("%s: cycle_radius is for pair_filter='cycle'" % who)
        return res, {}
    radius = float(o.get("cycle_radius", CYCLE_RADIUS))
    if not (np.isfinite(radius) and radius >= 0):
        raise ValueError("%s: cycle_radius=%r must be finite and >= 0" % (who, radius))
    if "col_idx" not in res:
        raise ValueError("%s: pair_filter='cycle' needs col_idx in res (match with twoway=True, or with soft and dual=True)" % who)
    pair_mask, pair_count, _ = cycle_filter(res, cld_rgb_nrm, radius)
    return dict(res, mask=pair_mask), dict(pair_mask=pair_mask, pair_count=pair_count)


def estimate_poses(res, cld_rgb_nrm, model_xyz, pose_fit="kabsch", icp_iters=0, pose_opts=None, model_nrm=None):
    """The pose stage of the pipeline: solve_poses with `pose_fit` ("kabsch" | "ransac" | "consensus"), then `icp_iters` ICP iterations
    when > 0.  pose_opts (optional dict): ransac_iters, ransac_inlier_dist, ransac_fix_percent, seed, consensus_tau, consensus_seeds,
    consensus_inlier_dist (pose_fit="consensus": consensus_poses' tau, seeds and inlier_dist), icp_tolerance, icp_reject_dist,
    min_points, and for pose_fit="kabsch" weights ("none" | "conf" | "dual") and targets ("vertex" | "soft") (solve_poses; RANSAC and ICP
    keep the hard pairs); icp_metric ("point" | "plane"): "plane" refines with refine_icp_plane instead of refine_icp, needs the
    model's unit normals model_nrm f32[M,3], takes icp_huber and icp_normal_gate as well (icp_tolerance then defaults to 1e-4) and adds
    icp_status; pair_filter ("none" | "cycle"): "cycle" needs a two-way match (col_idx in res), passes the pairs through cycle_filter
    at cycle_radius (default CYCLE_RADIUS) and gives the fit -- any pose_fit, weighted or not -- dict(res, mask=pair_mask), while ICP
    keeps the segmentation mask; the result gains pair_mask and pair_count.
    -> dict(RT, valid[, pair_mask, pair_count][, icp_iters, icp_resid[, icp_status]])."""
    o = dict(pose_opts or {})
    unknown = set(o) - {"ransac_iters", "ransac_inlier_dist", "ransac_fix_percent", "seed", "icp_tolerance", "icp_reject_dist",
                        "min_points", "weights", "targets", "icp_metric", "icp_huber", "icp_normal_gate", "consensus_tau", "consensus_seeds",
                        "consensus_inlier_dist", "pair_filter", "cycle_radius"}
    if unknown:
        raise ValueError("estimate_poses: unknown pose_opts %s" % sorted(unknown))
    min_points = o.get("min_points", 5)
    metric = o.get("icp_metric", "point")
    if metric not in ("point", "plane"):
        raise ValueError("estimate_poses: icp_metric must be 'point' or 'plane', got %r" % (metric,))
    if metric == "plane" and model_nrm is None:
        raise ValueError("estimate_poses: icp_metric='plane' needs model_nrm (the model's unit normals)")
    if metric == "point" and (o.get("icp_huber") is not None or o.get("icp_normal_gate") is not None):
        raise ValueError("estimate_poses: icp_huber / icp_normal_gate are for icp_metric='plane'")
    seg_res = res
    res, extra = _pair_filter(o, res, cld_rgb_nrm, "estimate_poses")
    if pose_fit == "kabsch":
        RT, valid = solve_poses(res, cld_rgb_nrm, model_xyz, min_points, weights=o.get("weights", "none"),
                                targets=o.get("targets", "vertex"))
    elif pose_fit == "consensus":
        RT, valid = solve_poses(res, cld_rgb_nrm, model_xyz, min_points, method=pose_fit, inlier_dist=o.get("consensus_inlier_dist", 0.015),
                                weights=o.get("weights", "none"), targets=o.get("targets", "vertex"),
                                consensus_tau=o.get("consensus_tau", 0.005), consensus_seeds=o.get("consensus_seeds", 8))
    else:
        RT, valid = solve_poses(res, cld_rgb_nrm, model_xyz, min_points, method=pose_fit, ransac_iters=o.get("ransac_iters", 20),
                                inlier_dist=o.get("ransac_inlier_dist", 0.015), fix_percent=o.get("ransac_fix_percent", 0.7),
                                seed=o.get("seed", 0), weights=o.get("weights", "none"), targets=o.get("targets", "vertex"))
    return _icp_stage(dict(RT=RT, valid=valid, **extra), seg_res, cld_rgb_nrm, model_xyz, icp_iters, o, model_nrm)


def _icp_stage(out, res, cld_rgb_nrm, model_xyz, icp_iters, o, model_nrm):
    """The ICP of estimate_poses on the fit out = dict(RT, valid) under the (checked) options o; `out` comes back, refined."""
    RT, valid = out["RT"], out["valid"]
    min_points, metric = o.get("min_points", 5), o.get("icp_metric", "point")
    if icp_iters > 0 and metric == "plane":
        out["RT"], out["icp_iters"], out["icp_resid"], out["icp_status"] = refine_icp_plane(
            RT, valid, cld_rgb_nrm, res["mask"], model_xyz, model_nrm, icp_iters, o.get("icp_tolerance", 1e-4), o.get("icp_reject_dist"),
            o.get("icp_normal_gate"), o.get("icp_huber"), min_points)
    elif icp_iters > 0:
        out["RT"], out["icp_iters"], out["icp_resid"] = refine_icp(RT, valid, cld_rgb_nrm, res["mask"], model_xyz, icp_iters,
                                                                   o.get("icp_tolerance", 0.001), o.get("icp_reject_dist"), min_points)
    return out


def transform(pts, RT):
    """pts f32[M,3], RT f32[B,3,4] -> f32[B,M,3]."""
    return pts[None] @ RT[:, :, :3].transpose(1, 2) + RT[:, None, :, 3]


def add_metric(RT_est, RT_gt, model_xyz):
    """pose_error.py:297-312 for a batch: mean vertex distance, f32[B]."""
    return (transform(model_xyz, RT_est) - transform(model_xyz, RT_gt)).norm(dim=2).mean(dim=1)


def adi_metric(RT_est, RT_gt, model_xyz):
    """pose_error.py:315-337: for every GT-posed vertex the nearest estimated-pose vertex (exact 1-NN, HIP)."""
    pe, pg = transform(model_xyz, RT_est).contiguous(), transform(model_xyz, RT_gt).contiguous()
    _, d2 = ops.knn_batch(pe, pg, 1, return_d2=True)
    return d2[:, :, 0].clamp(min=0).sqrt().mean(dim=1)


# ---- verification against the observed depth (csrc/gdm_verify.hip; include/gdm.h THE VERIFICATION RULE) ---------------
VERIFY_TILE = 64               # kTile of csrc/gdm_verify.hip: the side of the LDS tile a window is cut into
VERIFY_Q = 256                 # quantisation steps of |z_o - z_r| / delta over an agreeing pixel
VERIFY_Q_DEN = 512.0           # score = (n_agree - q_agree / 512) / ...: a pixel at the tolerance edge counts 0.5
VERIFY_COUNTS = ("n_model", "n_agree", "n_front", "n_behind", "n_nodepth", "q_agree")
VERIFY_CANDIDATES = ("kabsch", "ransac", "kabsch+icp", "ransac+icp")


def _host(a):
    """A tensor or an array as a numpy array on the host."""
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _verify_like_args(who, verts, faces, RT, depth, K, window, cand_valid):
    """The argument handling verify_poses and refine_poses_depth share: everything on RT's device in the dtype the entries take."""
    if not torch.is_tensor(RT) or RT.dim() != 4 or tuple(RT.shape[2:]) != (3, 4) or RT.shape[0] < 1 or RT.shape[1] < 1:
        raise ValueError("%s: RT must be a tensor [n,C,3,4], got %s" % (who, tuple(RT.shape) if torch.is_tensor(RT) else type(RT)))
    dev = RT.device
    n, C = RT.shape[:2]
    RT = ops._dev(RT.to(torch.float64), torch.float64, "RT")
    verts = torch.as_tensor(verts).to(dev)
    if verts.dtype not in (torch.float32, torch.float64):
        verts = verts.double()
    verts = ops._dev(verts, verts.dtype, "verts")
    faces = ops._dev(torch.as_tensor(faces).to(device=dev, dtype=torch.int32), torch.int32, "faces")
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] < 1:
        raise ValueError("%s: verts must be [V,3], got %s" % (who, tuple(verts.shape)))
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError("%s: faces must be [F,3], got %s" % (who, tuple(faces.shape)))
    depth = ops._dev(torch.as_tensor(depth).to(device=dev, dtype=torch.float32), torch.float32, "depth")
    if depth.dim() == 2:
        opi = 0
    elif depth.dim() == 3 and depth.shape[0] == n:
        opi = 1
    else:
        raise ValueError("%s: depth must be [H,W] or [n=%d,H,W], got %s" % (who, n, tuple(depth.shape)))
    K, kpi = ops._k64(torch.as_tensor(K).to(device=dev, dtype=torch.float64), n, "K")
    if window is not None:
        window = ops._dev(torch.as_tensor(window).to(device=dev, dtype=torch.int32), torch.int32, "window")
        if tuple(window.shape) != (n, 4):
            raise ValueError("%s: window must be [n=%d,4], got %s" % (who, n, tuple(window.shape)))
    if cand_valid is not None:
        cand_valid = ops._dev(torch.as_tensor(cand_valid).to(device=dev, dtype=torch.uint8), torch.uint8, "cand_valid")
        if tuple(cand_valid.shape) != (n, C):
            raise ValueError("%s: cand_valid must be [n=%d,C=%d], got %s" % (who, n, C, tuple(cand_valid.shape)))
    return verts, faces, RT, depth, opi, K, kpi, window, cand_valid


def verify_poses(verts, faces, RT, depth, K, window=None, delta=0.01, near=0.0, front_weight=0.25, min_px=16, cand_valid=None):
    """C candidate poses of one mesh for each of n instances against the observed depth, in one fused launch (gdm_pose_verify_hip):
    every candidate is rasterised by the pixel rule of include/gdm.h into LDS tiles of the instance's window and compared there with
    the depth frame; no [n C, H, W] image exists.  verts f32|f64[V,3] (passed on in that dtype, as evaluation.render_depth does) and
    faces i32[F,3] (device tensors or arrays); RT [n,C,3,4], a device tensor of any float dtype; depth f32[H,W] or [n,H,W]; K [3,3]
    or [n,3,3]; window i32[n,4] = (x0, y0, x1, y1) inclusive in frame pixels (boxes_to_windows), None = the whole frame; cand_valid
    bool[n,C] or None.  delta: the agreement tolerance in the unit of depth.  front_weight and min_px are the defaults of a
    definition, not tuned values.  -> dict(counts i32[n,C,6] = VERIFY_COUNTS, score f64[n,C], best i32[n]: the eligible candidate
    with the largest score, the lowest index on a tie, -1 when there is none).  No host synchronisation."""
    verts, faces, RT, depth, opi, K, kpi, window, cand_valid = _verify_like_args("verify_poses", verts, faces, RT, depth, K, window,
                                                                                 cand_valid)
    dev = RT.device
    n, C = RT.shape[:2]
    H, W = depth.shape[-2:]
    counts = torch.empty((n, C, 6), dtype=torch.int32, device=dev)
    score = torch.empty((n, C), dtype=torch.float64, device=dev)
    best = torch.empty((n,), dtype=torch.int32, device=dev)
    call("gdm_pose_verify_hip", verts, int(verts.dtype == torch.float64), faces, RT, K, kpi, depth, opi, window, cand_valid, n, C,
         verts.shape[0], faces.shape[0], H, W, float(near), float(delta), float(front_weight), int(min_px), counts, score, best)
    return dict(counts=counts, score=score, best=best)


def verify_select_numpy(counts, front_weight=0.25, min_px=16, cand_valid=None):
    """THE SELECTION of include/gdm.h on counts i[n,C,6] in fp64 -> score f64[n,C], best i32[n]."""
    k = np.asarray(counts).astype(np.float64)
    n, C = k.shape[:2]
    den = (k[..., 1] + k[..., 3]) + np.float64(front_weight) * k[..., 2]
    score = (k[..., 1] - k[..., 5] / VERIFY_Q_DEN) / np.maximum(1.0, den)
    ok = np.asarray(counts)[..., 0] >= int(min_px)
    if cand_valid is not None:
        ok &= np.asarray(cand_valid).reshape(n, C) != 0
    best = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        for c in range(C):
            if ok[i, c] and (best[i] < 0 or score[i, c] > score[i, best[i]]):
                best[i] = c
    return score, best


def verify_poses_numpy(verts, faces, RT, depth, K, window=None, delta=0.01, near=0.0, front_weight=0.25, min_px=16, cand_valid=None):
    """verify_poses on the host, the definition the kernel is tested against: evaluation.render_depth_numpy draws every candidate,
    np.float32 arithmetic restates THE VERIFICATION RULE of include/gdm.h and fp64 the selection.  Same arguments (arrays or
    tensors), same dict, as numpy arrays."""
    from . import evaluation
    RT = _host(RT).astype(np.float64)
    n, C = RT.shape[:2]
    depth = _host(depth).astype(np.float32)
    H, W = depth.shape[-2:]
    depth = np.broadcast_to(depth, (n, H, W))
    K = np.broadcast_to(_host(K).astype(np.float64), (n, 3, 3))
    verts = _host(verts)
    rendered = evaluation.render_depth_numpy(verts, faces, RT.reshape(n * C, 3, 4), np.repeat(K, C, axis=0), H, W, near)
    rendered = rendered.reshape(n, C, H, W)
    D, Q = np.float32(delta), np.float32(256.0 / float(delta))
    counts = np.zeros((n, C, 6), dtype=np.int32)
    for i in range(n):
        x0, y0, x1, y1 = (0, 0, W - 1, H - 1) if window is None else (int(v) for v in _host(window)[i])
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        z_o = depth[i, y0:y1 + 1, x0:x1 + 1]
        for c in range(C):
            z_r = rendered[i, c, y0:y1 + 1, x0:x1 + 1]
            model = z_r > 0                                                 # render_depth_numpy leaves 0 where nothing is drawn
            with np.errstate(invalid="ignore"):
                seen = z_o > 0
                d = (z_o - z_r).astype(np.float32)
                a = np.abs(d)
                agree = model & seen & (a <= D)
                front = model & seen & ~(a <= D) & (d < -D)
                behind = model & seen & ~(a <= D) & ~(d < -D)
                q = np.floor((a * Q).astype(np.float32))[agree].astype(np.int64).sum()
            nodepth = model & ~seen
            counts[i, c] = [model.sum(), agree.sum(), front.sum(), behind.sum(), nodepth.sum(), q]
    score, best = verify_select_numpy(counts, front_weight, min_px, None if cand_valid is None else _host(cand_valid))
    return dict(counts=counts, score=score, best=best)


# ---- refinement against the observed depth (csrc/gdm_refine.hip; include/gdm.h THE DEPTH REFINEMENT RULE) --------------
REFINE_STATUS = {0: "active", 1: "converged", 2: "starved", 3: "degenerate", 4: "invalid on entry"}
REFINE_SUMS = 30               # A upper triangle (21), g (6), S, L2, E: the doubles of a partial row before the pair count


def refine_poses_depth(verts, faces, RT, depth, K, window=None, iters=5, reject=0.01, huber=None, min_cos=0.0, near=0.0, min_px=16,
                       tolerance=0.0, pivot_min=1e-6, cand_valid=None):
    """C candidate poses of one mesh for each of n instances moved towards the observed depth by render-and-compare
    (gdm_pose_refine_depth_hip; include/gdm.h THE DEPTH REFINEMENT RULE): per iteration every active candidate is rasterised into LDS
    tiles of its window, every drawn pixel whose observed depth lies within `reject` of the rendered one pairs with the face drawn
    there, and one point-to-plane Gauss-Newton step is solved from the fp64 sums; the pose stays fp64 throughout.  Arguments as for
    verify_poses; huber None or 0 = no robust weights, min_cos 0 = no grazing gate.  reject, huber and min_cos are the defaults of a
    definition, not tuned values.  -> dict(RT f64[n,C,3,4], status i32[n,C] (REFINE_STATUS), iters i32[n,C], err f64[n,C] = mean |r|
    of the last applied iteration, pairs i32[n,C]).  A candidate with status 2, 3 or 4 keeps the pose it had.  Reproducible bit for
    bit; no host synchronisation; the only temporary is the planner's workspace."""
    verts, faces, RT, depth, opi, K, kpi, window, cand_valid = _verify_like_args("refine_poses_depth", verts, faces, RT, depth, K, window,
                                                                                 cand_valid)
    dev = RT.device
    n, C = RT.shape[:2]
    H, W = depth.shape[-2:]
    nbytes = call("gdm_pose_refine_depth_workspace_bytes", n, C, H, W)
    if nbytes == 0:
        raise ValueError("refine_poses_depth: n=%d C=%d H=%d W=%d is beyond the entry's limits (include/gdm.h)" % (n, C, H, W))
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    out = torch.empty((n, C, 3, 4), dtype=torch.float64, device=dev)
    status = torch.empty((n, C), dtype=torch.int32, device=dev)
    its = torch.empty((n, C), dtype=torch.int32, device=dev)
    err = torch.empty((n, C), dtype=torch.float64, device=dev)
    pairs = torch.empty((n, C), dtype=torch.int32, device=dev)
    call("gdm_pose_refine_depth_hip", verts, int(verts.dtype == torch.float64), faces, RT, K, kpi, depth, opi, window, cand_valid, n, C,
         verts.shape[0], faces.shape[0], H, W, float(near), int(iters), float(reject), float(huber or 0.0), float(min_cos), int(min_px),
         float(tolerance), float(pivot_min), ws, nbytes, out, status, its, err, pairs)
    return dict(RT=out, status=status, iters=its, err=err, pairs=pairs)


def raster_depth_face_numpy(verts, faces, rt, K, H, W, near):
    """One pose by the pixel rule of include/gdm.h (pixel_rule.covered, as evaluation.render_depth_numpy), keeping the face too: depth
    f32[H,W] (+inf where nothing is drawn) and face i64[H,W] (-1 there) -- per pixel the unsigned minimum of depth bits << 32 | face,
    as the kernel's tile keeps it: the minimum depth, the lowest face index among equal depths."""
    verts, rt, K = np.asarray(verts, dtype=np.float64), np.asarray(rt, dtype=np.float64), np.asarray(K, dtype=np.float64)
    faces = np.asarray(faces).astype(np.int64)
    keys = np.full((H, W), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    for f, (px0, py0, px1, py1), inside, d in pixel_rule.covered(faces, *pixel_rule.project(verts, rt, K, near), H, W):
        tile = keys[py0:py1 + 1, px0:px1 + 1]
        tile[inside] = np.minimum(tile[inside], pixel_rule.depth_keys(d, f)[inside])
    bits = (keys >> np.uint64(32)).astype(np.uint32)
    drawn = bits < pixel_rule.INF_BITS
    zbuf = np.where(drawn, bits, np.uint32(pixel_rule.INF_BITS)).view(np.float32)
    fbuf = np.where(drawn, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    return zbuf, fbuf


def refine_depth_sums_numpy(verts, faces, rt, depth, K, window=None, reject=0.01, huber=None, min_cos=0.0, near=0.0, terms=False):
    """The pairs and sums of ONE iteration of THE DEPTH REFINEMENT RULE for one pose rt f64[3,4] against depth f32[H,W]: the same fp64
    single operations as the kernel, the sums in numpy's order.  -> dict(sums f64[30] = A upper triangle (21), g (6), S, L2, E;
    pairs; with terms=True also J f64[P,6], r, w f64[P], the pixel coordinates uv i64[P,2] and the margins |r| - huber and
    |cos| - min_cos of every pair that reached the gate in question)."""
    verts_in = np.asarray(verts)
    verts64 = verts_in.astype(np.float64)                                  # fp32 vertices widen exactly
    faces = np.asarray(faces).astype(np.int64)
    rt = np.asarray(rt, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64)
    depth = np.asarray(depth, dtype=np.float32)
    H, W = depth.shape
    x0, y0, x1, y1 = (0, 0, W - 1, H - 1) if window is None else (int(v) for v in np.asarray(window))
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
    out = dict(sums=np.zeros(REFINE_SUMS), pairs=0)
    huber = float(huber or 0.0)
    empty = np.zeros(0)
    if terms:
        out.update(J=np.zeros((0, 6)), r=empty, w=empty, uv=np.zeros((0, 2), dtype=np.int64), huber_margin=empty, cos_margin=empty)
    if x0 > x1 or y0 > y1:
        return out
    zbuf, fbuf = raster_depth_face_numpy(verts64, faces, rt, K, H, W, near)
    inside = np.zeros((H, W), dtype=bool)
    inside[y0:y1 + 1, x0:x1 + 1] = True
    with np.errstate(invalid="ignore"):
        pair = inside & (fbuf >= 0) & np.isfinite(zbuf) & (depth > 0)
        pair &= np.abs((depth - zbuf).astype(np.float32)) <= np.float32(reject)
    v, u = np.nonzero(pair)                                                # row-major pixel order
    if len(u) == 0:
        return out
    f = faces[fbuf[v, u]]
    a, b, c = verts64[f[:, 0]], verts64[f[:, 1]], verts64[f[:, 2]]
    e1, e2 = b - a, c - a
    mx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    my = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    mz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    mm = (mx * mx + my * my) + mz * mz
    keep = mm > 0.0
    with np.errstate(all="ignore"):
        ln = np.sqrt(mm)
        nx, ny, nz = mx / ln, my / ln, mz / ln
    zo = depth[v, u].astype(np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    ox, oy, oz = (zo * (u.astype(np.float64) - cx)) / fx, (zo * (v.astype(np.float64) - cy)) / fy, zo
    R, t = rt[:, :3], rt[:, 3]
    cos_margin = empty
    if min_cos > 0.0:
        qx = (R[0, 0] * nx + R[0, 1] * ny) + R[0, 2] * nz
        qy = (R[1, 0] * nx + R[1, 1] * ny) + R[1, 2] * nz
        qz = (R[2, 0] * nx + R[2, 1] * ny) + R[2, 2] * nz
        dot = np.abs((qx * ox + qy * oy) + qz * oz)
        lim = np.float64(min_cos) * np.sqrt((ox * ox + oy * oy) + oz * oz)
        cos_margin = (dot - lim)[keep]
        with np.errstate(invalid="ignore"):
            keep = keep & ~(dot < lim)
    dx, dy, dz = ox - t[0], oy - t[1], oz - t[2]
    X = (R[0, 0] * dx + R[1, 0] * dy) + R[2, 0] * dz
    Y = (R[0, 1] * dx + R[1, 1] * dy) + R[2, 1] * dz
    Z = (R[0, 2] * dx + R[1, 2] * dy) + R[2, 2] * dz
    r = (nx * (X - a[:, 0]) + ny * (Y - a[:, 1])) + nz * (Z - a[:, 2])
    sel = np.nonzero(keep)[0]
    X, Y, Z, nx, ny, nz, r, u, v = (q[sel] for q in (X, Y, Z, nx, ny, nz, r, u, v))
    ar = np.abs(r)
    w = np.ones(len(r))
    if huber > 0.0:
        with np.errstate(all="ignore"):
            w = np.where(ar <= huber, 1.0, huber / ar)
    J = np.stack([Y * nz - Z * ny, Z * nx - X * nz, X * ny - Y * nx, nx, ny, nz], axis=1)
    sums = np.zeros(REFINE_SUMS)
    e = 0
    for p in range(6):
        wj = w * J[:, p]
        for q in range(p, 6):
            sums[e] = (wj * J[:, q]).sum()
            e += 1
        sums[21 + p] = (wj * r).sum()
    sums[27] = w.sum()
    sums[28] = (w * ((X * X + Y * Y) + Z * Z)).sum()
    sums[29] = ar.sum()
    out.update(sums=sums, pairs=len(r))
    if terms:
        out.update(J=J, r=r, w=w, uv=np.stack([u, v], axis=1), huber_margin=ar - huber, cos_margin=cos_margin)
    return out


def refine_poses_depth_numpy(verts, faces, RT, depth, K, window=None, iters=5, reject=0.01, huber=None, min_cos=0.0, near=0.0, min_px=16,
                             tolerance=0.0, pivot_min=1e-6, cand_valid=None, trace=False):
    """refine_poses_depth on the host, the definition the kernels are tested against: raster_depth_face_numpy draws every active
    candidate, refine_depth_sums_numpy forms the pairs and sums, icp_plane_solve_numpy (the restatement of gdm_icp_plane_solve.inc)
    solves and composes, and the stop rule follows the header statement for statement.  Same arguments (arrays or tensors), the same
    dict as numpy arrays.  trace=True adds `trace`: per (instance, candidate) a list with one dict per iteration evaluated --
    sums f64[30], pairs, min_pivot (None when starved), mean, stop_margin = | |err - mean| - tolerance |, RT (the pose after it)."""
    RT = _host(RT).astype(np.float64).copy()
    n, C = RT.shape[:2]
    depth = _host(depth).astype(np.float32)
    H, W = depth.shape[-2:]
    depth = np.broadcast_to(depth, (n, H, W))
    K = np.broadcast_to(_host(K).astype(np.float64), (n, 3, 3))
    verts, faces = _host(verts), _host(faces)
    status = np.zeros((n, C), dtype=np.int32)
    if cand_valid is not None:
        status[_host(cand_valid).reshape(n, C) == 0] = 4
    its = np.zeros((n, C), dtype=np.int32)
    err = np.zeros((n, C), dtype=np.float64)
    pairs = np.zeros((n, C), dtype=np.int32)
    log = [[[] for _ in range(C)] for _ in range(n)]
    for _ in range(int(iters)):
        for i in range(n):
            win = None if window is None else _host(window)[i]
            for c in range(C):
                if status[i, c] != 0:
                    continue
                s = refine_depth_sums_numpy(verts, faces, RT[i, c], depth[i], K[i], win, reject, huber, min_cos, near)
                pairs[i, c] = s["pairs"]
                rec = dict(sums=s["sums"], pairs=s["pairs"], min_pivot=None, mean=None, stop_margin=None, RT=RT[i, c].copy())
                log[i][c].append(rec)
                if s["pairs"] < max(int(min_px), 6):
                    status[i, c] = 2
                    continue
                A = np.zeros((6, 6))
                A[np.triu_indices(6)] = s["sums"][:21]
                A = A + np.triu(A, 1).T
                with np.errstate(all="ignore"):
                    sol = icp_plane_solve_numpy(A, s["sums"][21:27], s["sums"][27], s["sums"][28], RT[i, c, :, :3], RT[i, c, :, 3], pivot_min)
                rec["min_pivot"] = sol["min_pivot"]
                if sol["degenerate"]:
                    status[i, c] = 3
                    continue
                RT[i, c, :, :3], RT[i, c, :, 3] = sol["R"], sol["t"]
                its[i, c] += 1
                mean = s["sums"][29] / np.float64(s["pairs"])
                rec.update(mean=mean, stop_margin=abs(abs(err[i, c] - mean) - tolerance), RT=RT[i, c].copy())
                if abs(err[i, c] - mean) < tolerance:
                    status[i, c] = 1
                err[i, c] = mean
    out = dict(RT=RT, status=status, iters=its, err=err, pairs=pairs)
    if trace:
        out["trace"] = log
    return out


def boxes_to_windows(bbox_xyxy, H, W, pad=1.25):
    """Detection boxes f[n,4] = (x0, y0, x1, y1) -> the windows verify_poses takes, i32[n,4] on the boxes' device: the box scaled
    about its centre by `pad`, floor / ceil to whole pixels, cut to the frame.  A box that misses the frame gives an empty window
    (x0 > x1 or y0 > y1: all-zero counts, never eligible)."""
    b = torch.as_tensor(bbox_xyxy).to(torch.float64)
    if b.dim() != 2 or b.shape[1] != 4:
        raise ValueError("boxes_to_windows: boxes must be [n,4], got %s" % (tuple(b.shape),))
    cx, cy = (b[:, 0] + b[:, 2]) * 0.5, (b[:, 1] + b[:, 3]) * 0.5
    hx, hy = (b[:, 2] - b[:, 0]) * 0.5 * float(pad), (b[:, 3] - b[:, 1]) * 0.5 * float(pad)
    lo = torch.stack([torch.floor(cx - hx).nan_to_num(nan=float(W)).clamp(0, W), torch.floor(cy - hy).nan_to_num(nan=float(H)).clamp(0, H)], 1)
    hi = torch.stack([torch.ceil(cx + hx).nan_to_num(nan=-1.0).clamp(-1, W - 1), torch.ceil(cy + hy).nan_to_num(nan=-1.0).clamp(-1, H - 1)], 1)
    return torch.cat([lo, hi], dim=1).to(torch.int32)


_VERIFY_KEYS = {"verts", "faces", "depth", "K", "window", "delta", "near", "front_weight", "min_px"}


def select_verified(candidates, verify):
    """candidates: an ordered dict name -> (RT f32[n,3,4], valid bool[n]); verify: dict(verts, faces, depth, K[, window, delta, near,
    front_weight, min_px]) -- verify_poses' arguments.  The candidates are stacked in the dict's order, verified with their valid
    flags as cand_valid, and the winner is gathered on the device (no host synchronisation).  -> dict(RT f32[n,3,4], valid bool[n] =
    best >= 0 -- an invalid item keeps candidate 0's RT and score --, which i32[n] = best, score f64[n], scores f64[n,C], counts
    i32[n,C,6], names, cand_RT f32[n,C,3,4], cand_valid bool[n,C])."""
    if not candidates:
        raise ValueError("select_verified: no candidates")
    unknown = set(verify) - _VERIFY_KEYS
    missing = {"verts", "faces", "depth", "K"} - set(verify)
    if unknown or missing:
        raise ValueError("select_verified: verify has unknown keys %s / lacks %s" % (sorted(unknown), sorted(missing)))
    names = tuple(candidates)
    cand_RT = torch.stack([candidates[k][0] for k in names], dim=1).contiguous()
    cand_valid = torch.stack([candidates[k][1].bool() for k in names], dim=1)
    v = verify_poses(verify["verts"], verify["faces"], cand_RT, verify["depth"], verify["K"], cand_valid=cand_valid,
                     **{k: verify[k] for k in ("window", "delta", "near", "front_weight", "min_px") if k in verify})
    pick = v["best"].clamp_min(0).long()
    RT = torch.gather(cand_RT, 1, pick[:, None, None, None].expand(-1, 1, 3, 4))[:, 0]
    score = torch.gather(v["score"], 1, pick[:, None])[:, 0]
    return dict(RT=RT, valid=v["best"] >= 0, which=v["best"], score=score, scores=v["score"], counts=v["counts"], names=names,
                cand_RT=cand_RT, cand_valid=cand_valid)


_DEPTH_OPTS = {"reject", "huber", "min_cos", "min_px", "tolerance", "pivot_min"}


def estimate_poses_verified(res, cld_rgb_nrm, model_xyz, verify, candidates=VERIFY_CANDIDATES, icp_iters=10, pose_opts=None,
                            model_nrm=None, depth_iters=5, depth_opts=None):
    """Several pose estimates of every crop, judged against the depth frame the crop came from: each name of `candidates` -- "kabsch",
    "ransac" or "consensus", with "+icp" for `icp_iters` ICP iterations on it, and after that "+depth" for `depth_iters` iterations of
    refine_poses_depth on its parent (the name without "+depth") against the verify dict's verts, faces, depth, K, window and near with
    depth_opts (reject, huber, min_cos, min_px, tolerance, pivot_min) -- goes through estimate_poses' stages with pose_opts, every
    parent made once and shared; then select_verified(verify) keeps, per crop, the one the observed depth agrees with best.  A
    "+depth" candidate is its refined pose rounded to f32, valid when the parent was and the refinement's status is 0 or 1.
    -> select_verified's dict; with a "+depth" name also depth_status i32[n,C]: the refinement's status, -1 for the other candidates;
    with pose_opts' pair_filter="cycle" (every fit then sees the filtered pairs, estimate_poses) also pair_mask and pair_count."""
    names = tuple(candidates)
    bad = [k for k in names if k.split("+")[0] not in ("kabsch", "ransac", "consensus")
           or k.split("+")[1:] not in ([], ["icp"], ["depth"], ["icp", "depth"])]
    if bad or not names or len(set(names)) != len(names):
        raise ValueError("estimate_poses_verified: candidates must be distinct names out of kabsch, ransac, consensus, kabsch+icp, "
                         "ransac+icp, consensus+icp, each optionally followed by +depth; got %r" % (names,))
    o = dict(pose_opts or {})
    dopts = dict(depth_opts or {})
    if set(dopts) - _DEPTH_OPTS:
        raise ValueError("estimate_poses_verified: unknown depth_opts %s" % sorted(set(dopts) - _DEPTH_OPTS))
    # pose_opts' pair_filter runs once: every fit sees the same filtered pairs, ICP (below) the segmentation mask
    fit_res, pair_out = _pair_filter(o, res, cld_rgb_nrm, "estimate_poses_verified")
    fit_opts = {k: v for k, v in o.items() if k not in ("pair_filter", "cycle_radius")}
    made = {}

    def stage(k):
        if k not in made:
            fit = k.split("+")[0]
            if k == fit:
                made[k] = estimate_poses(fit_res, cld_rgb_nrm, model_xyz, fit, 0, fit_opts, model_nrm)
            else:
                made[k] = _icp_stage(dict(stage(fit)), res, cld_rgb_nrm, model_xyz, int(icp_iters), o, model_nrm)
        return made[k]

    fits, depth_status = {}, {}
    for k in names:
        parent = stage(k[:-len("+depth")] if k.endswith("+depth") else k)
        if k.endswith("+depth"):
            missing = {"verts", "faces", "depth", "K"} - set(verify)
            if missing:
                raise ValueError("estimate_poses_verified: verify lacks %s" % sorted(missing))
            r = refine_poses_depth(verify["verts"], verify["faces"], parent["RT"][:, None], verify["depth"], verify["K"],
                                   window=verify.get("window"), iters=int(depth_iters), near=verify.get("near", 0.0),
                                   cand_valid=parent["valid"][:, None], **dopts)
            depth_status[k] = r["status"][:, 0]
            fits[k] = (r["RT"][:, 0].to(torch.float32), parent["valid"].bool() & (r["status"][:, 0] <= 1))
        else:
            fits[k] = (parent["RT"], parent["valid"])
    sel = select_verified(fits, verify)
    sel.update(pair_out)
    if depth_status:
        none = torch.full_like(next(iter(depth_status.values())), -1)
        sel["depth_status"] = torch.stack([depth_status.get(k, none) for k in names], dim=1)
    return sel


def verify_counts_composed(verts, faces, RT, depth, K, window=None, delta=0.01, near=0.0):
    """The counts of verify_poses composed from what the package offered before the fused kernel: evaluation.render_depth into an
    [n C, H, W] z-buffer, then torch comparisons.  The yardstick of tools/pose_verify_profile.py and of the test that ties the LDS
    path to raster_kernel; it reads and writes n C H W floats several times over and is not meant for use.  -> counts i32[n,C,6]."""
    from . import evaluation
    n, C = RT.shape[:2]
    dev = RT.device
    depth = torch.as_tensor(depth).to(device=dev, dtype=torch.float32)
    H, W = depth.shape[-2:]
    K = torch.as_tensor(K).to(device=dev, dtype=torch.float64)
    z_r = evaluation.render_depth(verts, faces, RT.reshape(n * C, 3, 4), K if K.dim() == 2 else K.repeat_interleave(C, dim=0), H, W, near,
                                  keep_inf=True).view(n, C, H, W)
    model = torch.isfinite(z_r)
    if window is not None:
        w = torch.as_tensor(window).to(dev).long()
        xs, ys = torch.arange(W, device=dev), torch.arange(H, device=dev)
        inside = ((ys[None, :, None] >= w[:, 1, None, None]) & (ys[None, :, None] <= w[:, 3, None, None])
                  & (xs[None, None, :] >= w[:, 0, None, None]) & (xs[None, None, :] <= w[:, 2, None, None]))
        model = model & inside[:, None]
    z_o = depth.view(-1, 1, H, W).expand(n, C, H, W)
    D = torch.tensor(np.float32(delta), device=dev)
    Q = torch.tensor(np.float32(256.0 / float(delta)), device=dev)
    seen = z_o > 0
    d = z_o - z_r
    a = d.abs()
    agree = model & seen & (a <= D)
    front = model & seen & ~(a <= D) & (d < -D)
    behind = model & seen & ~(a <= D) & ~(d < -D)
    nodepth = model & ~seen
    q = torch.where(agree, torch.floor(a * Q), torch.zeros_like(a)).to(torch.int64)
    return torch.stack([m.sum(dim=(2, 3)) for m in (model, agree, front, behind, nodepth, q)], dim=-1).to(torch.int32)


def refine_sums_composed(verts, faces, RT, depth, K, window=None, reject=0.01, huber=None, min_cos=0.0, near=0.0):
    """The pairs and sums of one iteration of refine_poses_depth composed from what the package offered before the fused kernel:
    render.render_frames' kernel into [n C, H, W] depth and face images, then torch gathers and fp64 sums over whole images.  The
    yardstick of tools/pose_depth_refine_profile.py and of the test that ties the 64-bit LDS path to raster_kernel; not meant for use.
    -> dict(pairs i32[n,C], sums f64[n,C,30] in the kernel's layout, torch's summation order)."""
    n, C = RT.shape[:2]
    dev = RT.device
    verts = torch.as_tensor(verts).to(dev)
    verts = verts if verts.dtype in (torch.float32, torch.float64) else verts.double()
    faces = torch.as_tensor(faces).to(device=dev, dtype=torch.int32).contiguous()
    depth = torch.as_tensor(depth).to(device=dev, dtype=torch.float32)
    H, W = depth.shape[-2:]
    K = torch.as_tensor(K).to(device=dev, dtype=torch.float64)
    Kc = K.expand(n, 3, 3).repeat_interleave(C, dim=0).contiguous()
    V, F = verts.shape[0], faces.shape[0]
    RTc = RT.to(torch.float64).reshape(n * C, 1, 3, 4).contiguous()
    light = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64, device=dev).expand(n * C, 3).contiguous()
    _, z_r, _, face, _ = ops.render_frames(verts.contiguous(), torch.zeros((V, 3), dtype=torch.uint8, device=dev),
                                           torch.zeros((V, 3), dtype=torch.float32, device=dev), faces, [0, F],
                                           torch.zeros((n * C, 1), dtype=torch.int32, device=dev), RTc, Kc, light, H, W, 0.5, near)
    z_r, face = z_r.view(n, C, H, W), face.view(n, C, H, W).long()
    pair = face >= 0
    xs, ys = torch.arange(W, device=dev), torch.arange(H, device=dev)
    if window is not None:
        w = torch.as_tensor(window).to(dev).long()
        inside = ((ys[None, :, None] >= w[:, 1, None, None]) & (ys[None, :, None] <= w[:, 3, None, None])
                  & (xs[None, None, :] >= w[:, 0, None, None]) & (xs[None, None, :] <= w[:, 2, None, None]))
        pair = pair & inside[:, None]
    z_o = depth.view(-1, 1, H, W).expand(n, C, H, W)
    pair = pair & (z_o > 0) & ((z_o - z_r).abs() <= torch.tensor(np.float32(reject), device=dev))
    vd = verts.double()
    tri = vd[faces.long()[face.clamp_min(0)]]                              # [n,C,H,W,3,3]
    a, e1, e2 = tri[..., 0, :], tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 0, :]
    m = torch.cross(e1, e2, dim=-1)
    mm = (m * m).sum(-1)
    pair = pair & (mm > 0)
    nrm = m / mm.clamp_min(1e-300).sqrt()[..., None]
    zo = torch.where(pair, z_o, torch.zeros_like(z_o)).double()
    Kn = K.expand(n, 3, 3)
    fx, fy, cx, cy = (Kn[:, i, j].view(n, 1, 1, 1) for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))
    o = torch.stack([zo * (xs.double().view(1, 1, 1, W) - cx) / fx, zo * (ys.double().view(1, 1, H, 1) - cy) / fy, zo], dim=-1)
    R, t = RT[..., :3].double(), RT[..., 3].double()
    if min_cos > 0.0:
        q = torch.einsum("ncij,nchwj->nchwi", R, nrm)
        pair = pair & ~((q * o).sum(-1).abs() < float(min_cos) * (o * o).sum(-1).sqrt())
    x = torch.einsum("ncji,nchwj->nchwi", R, o - t[:, :, None, None, :])
    r = (nrm * (x - a)).sum(-1)
    ar = r.abs()
    h = float(huber or 0.0)
    wt = torch.where(ar <= h, torch.ones_like(ar), h / ar.clamp_min(1e-300)) if h > 0.0 else torch.ones_like(ar)
    wt = torch.where(pair, wt, torch.zeros_like(wt))
    J = torch.cat([torch.cross(x, nrm, dim=-1), nrm], dim=-1)
    sums = []
    for p in range(6):
        sums += [(wt * J[..., p] * J[..., q]).sum(dim=(2, 3)) for q in range(p, 6)]
    sums += [(wt * J[..., p] * r).sum(dim=(2, 3)) for p in range(6)]
    sums += [wt.sum(dim=(2, 3)), (wt * (x * x).sum(-1)).sum(dim=(2, 3)), torch.where(pair, ar, torch.zeros_like(ar)).sum(dim=(2, 3))]
    return dict(pairs=pair.sum(dim=(2, 3)).to(torch.int32), sums=torch.stack(sums, dim=-1))
