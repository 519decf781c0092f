"""Training losses of the geoMatch path, same names / semantics as /root/reference/models/loss.py:
CircleLoss :433-494, FocalLoss :15-46, AutomaticWeightedLoss :496-516.
Plain torch on the device the inputs live on (the reference hard-codes `.cuda()`, :509)."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class FocalLoss(nn.Module):
    def __init__(self, gamma=0, alpha=None, size_average=True):
        super().__init__()
        self.gamma = gamma
        self.alpha = alpha
        if isinstance(alpha, (float, int)):
            self.alpha = torch.tensor([alpha, 1 - alpha])
        if isinstance(alpha, list):
            self.alpha = torch.tensor(alpha)
        self.size_average = size_average

    def forward(self, input, target):
        input = input.transpose(1, 2)                       # [B,C,N] -> [B,N,C]
        input = input.contiguous().view(-1, input.size(2))
        target = target.view(-1, 1)
        logpt = F.log_softmax(input, dim=-1).gather(1, target).view(-1)
        pt = logpt.detach().exp()
        if self.alpha is not None:
            at = self.alpha.to(input).gather(0, target.view(-1))
            logpt = logpt * at
        loss = -1 * (1 - pt) ** self.gamma * logpt
        return loss.mean() if self.size_average else loss.sum()


class CircleLoss(nn.Module):
    def __init__(self, gamma):
        super().__init__()
        self.gamma = gamma
        self.soft_plus = nn.Softplus()

    @staticmethod
    def log_sum_exp(inputs, mask):
        """loss.py:441-459: masked LSE; `mask` is 1.0 where the entry takes part."""
        inv = 1.0 - mask
        s, _ = torch.max(inputs + (-1e7 * inv), dim=-1, keepdim=True)
        off = (inputs - s).masked_fill(inv.to(torch.bool), -float("inf"))
        return (s + off.exp().sum(dim=-1, keepdim=True).log()).squeeze(-1)

    def rows(self, sim, mask, m):
        """Per-row loss f32[rows] (forward() is its mean)."""
        ap = torch.clamp_min(-sim.detach() + 1 + m, min=0.0).masked_fill(~mask, 0)
        an = torch.clamp_min(sim.detach() + m, min=0.0).masked_fill(mask, 0)
        delta_p, delta_n = 1 - m, m
        logit_p = -ap * (sim - delta_p) * self.gamma
        logit_n = an * (sim - delta_n) * self.gamma
        lse_p = self.log_sum_exp(logit_p, mask.to(torch.float))
        lse_n = self.log_sum_exp(logit_n, (~mask).to(torch.float))
        return self.soft_plus(lse_p + lse_n)

    def forward(self, sim, mask, m):
        return self.rows(sim, mask, m).mean()


class AutomaticWeightedLoss(nn.Module):
    def __init__(self, num=2):
        super().__init__()
        self.params = nn.Parameter(torch.ones(num))

    def forward(self, *x):
        loss_sum = 0
        for i, loss in enumerate(x):
            loss_sum = loss_sum + 0.5 / (self.params[i] ** 2) * loss + torch.log(1 + self.params[i] ** 2)
        return loss_sum


def soft_coord_reference(x, y, xyz, gamma):
    """The soft assignment of ops.soft_coord_match in plain torch, any dtype and device, WITH the [R, M] similarity materialised:
    x [R,D] and y [M,D] unit rows, xyz [M,3] -> lse [R] = logsumexp_c(gamma <x_r, y_c>), soft [R,3] = softmax_c(gamma <x_r, y_c>) @ xyz.
    What the fused operator is held to (tests) and the materialised leg of tools/soft_coord_profile.py."""
    logits = float(gamma) * (x @ y.t())
    lse = torch.logsumexp(logits, dim=1)
    soft = torch.exp(logits - lse.unsqueeze(1)) @ xyz.to(logits.dtype)
    return lse, soft


class SoftAssignLoss(nn.Module):
    """Two training losses on the differentiable soft assignment, per selected scene row r with ground-truth vertex g_r:
      coordinate  sum_k smooth_l1(soft_rk - t_rk, beta)     metres; t_r = the row's model coordinate (given by the caller)
      likelihood  lse_r - gamma s_{r,g_r}                    = -log softmax_c(gamma s_rc)[g_r]; symmetric objects (c2 given):
                  lse_r - logaddexp(gamma s_{r,c1}, gamma s_{r,c2})
    averaged as the circle loss is: the mean over the items with at least 3 selected rows of the mean over their selected rows.  A
    row without a ground-truth vertex (g == M; symmetric: either column == M) has weight 0 in both terms and still counts in its
    item's denominator.  The coordinate term is refused for symmetric objects: the expectation over two valid vertices is neither.
    match = "kernel": ops.soft_coord_match (HIP, no [R, M] tensor, float32 on the GPU only); "reference": soft_coord_reference
    (materialised; any dtype and device) -- an explicit choice, never a fall-back."""

    def __init__(self, gamma=16.0, beta=0.005, match="kernel"):
        super().__init__()
        if match not in ("kernel", "reference"):
            raise ValueError("SoftAssignLoss: match must be 'kernel' or 'reference', got %r" % (match,))
        self.gamma, self.beta, self.match = float(gamma), float(beta), match

    def assignment(self, rows, mesh_rows, xyz):
        if self.match == "kernel":
            from . import ops
            return ops.soft_coord_match(rows, mesh_rows, xyz, self.gamma)
        return soft_coord_reference(rows, mesh_rows, xyz, self.gamma)

    def forward(self, rows, mesh_rows, xyz, g, item, counts, target=None, c2=None, row_weight=None, terms=("xyz", "nll"),
                static_shape=None, pose=None):
        """rows [R,D] / mesh_rows [M,D] unit rows, xyz [M,3], g int[R] (M = none), item int[R] in [0, B), counts int[B] = selected
        rows per item, target [R,3] (default xyz[g]), c2 int[R] (symmetric objects), row_weight [R] (1 = selected, 0 = not: the
        static all-rows form; default all selected), static_shape = (B, N) when the rows are all B*N points in order (the per-item
        sums are then plain row sums, no index_add).  -> (coordinate loss, likelihood loss); a term not in `terms` is None.
        "pose" in terms adds the pose-fit loss of the same assignment (one soft_coord_match for all three) as a third value:
        pose = dict(fn=PoseFitLoss, scene=cld_rgb_nrm [B,C,N] or [B,N,3], RT=[B,3,4], point=int[R] the point index of every row,
        shape=(B, N)); the soft vertices are the targets, scattered into [B,N] (the static form is a view)."""
        M = mesh_rows.shape[0]
        symmetric = c2 is not None
        if symmetric and "pose" in terms:
            raise ValueError("SoftAssignLoss: the pose-fit term is not defined for symmetric objects (the expected vertex of two valid "
                             "vertices is neither of them); pose.kabsch_pose_loss takes symmetry transforms for hard targets")
        if symmetric and "xyz" in terms:
            raise ValueError("SoftAssignLoss: the coordinate term is not defined for symmetric objects (the expected vertex of two "
                             "valid vertices is neither of them); use the likelihood term alone")
        g = g.long()
        has = g < M
        if symmetric:
            c2 = c2.long()
            has = has & (c2 < M) & (c2 >= 0)
        w = has.to(rows.dtype)
        if row_weight is not None:
            w = w * row_weight.to(rows.dtype)
        lse, soft = self.assignment(rows, mesh_rows, xyz)
        gc = g.clamp(0, M - 1)
        B = counts.shape[0]
        ok = (counts >= 3).to(rows.dtype)
        denom = counts.clamp(min=1).to(rows.dtype)

        def averaged(per_row):
            per_row = per_row * w
            if static_shape is not None:
                per_item = per_row.view(static_shape).sum(dim=1)
            else:
                per_item = torch.zeros(B, dtype=rows.dtype, device=rows.device).index_add_(0, item.long(), per_row)
            return (per_item / denom * ok).sum() / ok.sum().clamp(min=1.0)

        out_xyz = out_nll = None
        if "xyz" in terms:
            t = xyz[gc].to(rows.dtype) if target is None else target.to(rows.dtype)
            out_xyz = averaged(F.smooth_l1_loss(soft, t, beta=self.beta, reduction="none").sum(dim=1))
        if "nll" in terms:
            s1 = self.gamma * (rows * mesh_rows[gc]).sum(dim=1)
            if symmetric:
                s2 = self.gamma * (rows * mesh_rows[c2.clamp(0, M - 1)]).sum(dim=1)
                s1 = torch.logaddexp(s1, s2)
            out_nll = averaged(lse - s1)
        if "pose" not in terms:
            return out_xyz, out_nll
        fn = pose["fn"]
        wrow = fn.row_weight(w, self.gamma * (rows * mesh_rows[gc]).sum(dim=1) if fn.weights == "prob" else None, lse)
        B, N = pose["shape"]
        if static_shape is not None:
            tgt, wgt = soft.view(B, N, 3), wrow.view(B, N)
        else:
            at = (item.long(), pose["point"].long())
            tgt = torch.zeros((B, N, 3), dtype=soft.dtype, device=soft.device).index_put(at, soft)
            wgt = torch.zeros((B, N), dtype=soft.dtype, device=soft.device).index_put(at, wrow)
        return out_xyz, out_nll, fn(pose["scene"], tgt, wgt, pose["RT"], xyz)


class PoseFitLoss(nn.Module):
    """The pose-fit training loss (include/gdm.h THE POSE LOSS RULE): the mean, over the crops whose fit is well
    conditioned (state 0; clamp(min=1) on their number, as SoftAssignLoss averages), of the mean distance of the first `points` model
    points between the weighted Kabsch fit of the targets and the ground-truth pose -- what the evaluator's ADD measures, with a
    gradient for the targets and the weights.  weights: what the caller's rows weigh (row_weight): "uniform" the 0/1 row selection,
    "prob" the soft assignment's probability of the ground-truth vertex, exp(gamma s_{r,g_r} - lse_r), 0 for a row without one.
    match = "kernel": pose.kabsch_pose_loss (HIP, float32 on the GPU only); "reference": pose.kabsch_pose_loss_reference (plain torch,
    torch.linalg.svd and autograd; any dtype and device) -- an explicit choice, never a fall-back.  cond_min = 1e-3 is the default of a
    definition, not a tuned value."""

    def __init__(self, points=256, weights="uniform", cond_min=1e-3, match="kernel"):
        super().__init__()
        if weights not in ("uniform", "prob"):
            raise ValueError("PoseFitLoss: weights must be 'uniform' or 'prob', got %r" % (weights,))
        if match not in ("kernel", "reference"):
            raise ValueError("PoseFitLoss: match must be 'kernel' or 'reference', got %r" % (match,))
        if int(points) < 1:
            raise ValueError("PoseFitLoss: points=%r must be >= 1" % (points,))
        self.points, self.weights, self.cond_min, self.match = int(points), weights, float(cond_min), match

    def row_weight(self, selected, logit_g=None, lse=None):
        """The fit weight of every row: selected (0/1, 0 for a row without a ground-truth vertex), times exp(logit_g - lse) for "prob"."""
        if self.weights == "uniform":
            return selected
        return torch.exp(logit_g - lse) * selected

    def per_crop(self, scene, target, weight, RT_gt, model_xyz, sym=None, mask=None, min_points=5):
        """-> (loss [B], RT f32[B,3,4], state u8[B], sym_idx i32[B]) of the first `points` rows of model_xyz [M,3]."""
        from . import pose
        pts = model_xyz[:self.points].detach().contiguous()
        if self.match == "kernel":
            return pose.kabsch_pose_loss(scene, target, weight, RT_gt.detach(), pts, sym, mask, min_points, self.cond_min)
        return pose.kabsch_pose_loss_reference(scene, target, weight, RT_gt.detach(), pts, sym, mask, min_points, self.cond_min)

    def forward(self, scene, target, weight, RT_gt, model_xyz, sym=None, mask=None, min_points=5):
        loss_b, _, state, _ = self.per_crop(scene, target, weight, RT_gt, model_xyz, sym, mask, min_points)
        ok = (state == 0).to(loss_b.dtype)
        return (loss_b * ok).sum() / ok.sum().clamp(min=1.0)


def soft_assign_terms(model, rows, mesh_rows, xyz, c1, c2, bi, pi, counts, x, static_shape=None, row_weight=None):
    """The shared wiring of SoftAssignLoss into both variants' pointwise_feature_matching: (soft_xyz_loss, soft_nll_loss) for the
    selected rows (bi, pi) of the batch x, controlled by the model attributes soft_gamma / soft_xyz_weight / soft_nll_weight; a term
    whose weight is 0 is not computed and comes back as a zero scalar.  Coordinate target: R_b^T (p_r - t_b), the scene point in
    model coordinates, when the batch carries RT; else the ground-truth vertex xyz[match_idx_r].  A model attribute soft_match =
    "reference" selects the materialised plain-torch assignment (tests on the CPU / in fp64); the default is the HIP operator.
    With the model attribute pose_loss_weight != 0 the pose-fit loss (PoseFitLoss on pose_loss_points model points with pose_loss_weights
    row weights; targets = the soft vertices at soft_gamma, from the same single soft_coord_match) is a third value: it needs the
    batch's RT and a model that is not symmetric, and raises ValueError otherwise.  soft_match selects its reference as well."""
    terms = tuple(t for t, wt in (("xyz", model.soft_xyz_weight), ("nll", model.soft_nll_weight)) if wt != 0)
    pose = None
    if getattr(model, "pose_loss_weight", 0.0) != 0:
        if "RT" not in x:
            raise ValueError("pose_loss_weight != 0 needs the ground-truth pose x['RT'] in the batch")
        if c2 is not None:
            raise ValueError("pose_loss_weight != 0: the pose-fit loss is not defined for symmetric objects (an expectation over two "
                             "valid vertices is neither); pose.kabsch_pose_loss takes symmetry transforms for hard targets")
        terms += ("pose",)
        fit = PoseFitLoss(getattr(model, "pose_loss_points", 256), getattr(model, "pose_loss_weights", "uniform"),
                          match=getattr(model, "soft_match", "kernel"))
        cld = x["cld_rgb_nrm"]
        pose = dict(fn=fit, scene=cld.detach() if cld.dtype == rows.dtype else cld[:, :3, :].detach().to(rows.dtype), RT=x["RT"][:, :3, :].to(rows.dtype),
                    point=pi, shape=static_shape if static_shape is not None else (counts.shape[0], cld.shape[2]))
    target = None
    if "xyz" in terms and "RT" in x:
        RT = x["RT"].to(rows.dtype)
        p = x["cld_rgb_nrm"][:, :3, :].transpose(1, 2)[bi, pi].to(rows.dtype)              # [R,3] scene points (m)
        target = torch.einsum("rj,rjk->rk", p - RT[bi, :, 3], RT[bi, :, :3])               # R^T (p - t) as a row vector
    fn = SoftAssignLoss(model.soft_gamma, model.soft_beta, match=getattr(model, "soft_match", "kernel"))
    zero = torch.zeros((), dtype=rows.dtype, device=rows.device)
    if pose is not None:
        lx, ln, lp = fn(rows, mesh_rows, xyz, c1, bi, counts, target=target, c2=c2, row_weight=row_weight, terms=terms,
                        static_shape=static_shape, pose=pose)
        return (zero if lx is None else lx), (zero if ln is None else ln), lp
    lx, ln = fn(rows, mesh_rows, xyz, c1, bi, counts, target=target, c2=c2, row_weight=row_weight, terms=terms, static_shape=static_shape)
    return (zero if lx is None else lx), (zero if ln is None else ln)
