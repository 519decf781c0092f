"""GeoMatch, DGCNN variant: drop-in for /root/reference/models/geoMatch_DGCNN.py:12-183 (same constructor,
forward, end_points and parameter names).  Differences from the FFB6D/SplineCNN GeoMatch: both embeddings are
DGCNN edge-conv stacks over `cld_rgb_nrm` / the model buffer, `mesh` is returned as [1,D,M] straight from
the mesh trunk, and the positive radius of the matching loss scales with depth (:66-67)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, settings
from .dgcnn import DgcnnMeshEmb, DgcnnPcdEmb
from .layers import PtSeq, pt_conv1d
from .loss import AutomaticWeightedLoss, CircleLoss, FocalLoss


class GeoMatch(nn.Module):
    needs_pyramid = False            # dynamic graphs are built inside the trunks; no neighbour pyramid in the inputs
    train_path = "modules"           # "modules" | "fused": how both trunks run in TRAINING mode (dgcnn._DgcnnTrunk._embed /
                                     # ._embed_train_fused); not part of the state dict, read only when self.training

    soft_gamma = 16.0                # the soft-assignment training losses (loss.SoftAssignLoss, geoMatch.GeoMatch): opt-in,
    soft_beta = 0.005                # plain attributes; with both weights 0 nothing of them runs
    soft_xyz_weight = 0.0
    soft_nll_weight = 0.0
    pose_loss_weight = 0.0           # the pose-fit loss (loss.PoseFitLoss), as in geoMatch.GeoMatch: opt-in, off at 0
    pose_loss_points = 256
    pose_loss_weights = "uniform"

    def __init__(self, cfg, cls_id, model_points=None):
        super().__init__()
        self.awl = AutomaticWeightedLoss(2)
        self.feat_dim = cfg["feat_dim"]
        self.positive_r = 3
        self.model_emb = DgcnnMeshEmb(cfg, cls_id, model_points=model_points)
        self.pcd_emb = DgcnnPcdEmb(cfg)
        self.circle_loss = CircleLoss(16)
        self.seg_loss_func = FocalLoss(gamma=2)
        self.seg_layer = (PtSeq(self.feat_dim).conv1d(128, bn=True).conv1d(128, bn=True).conv1d(128, bn=True)
                          .conv1d(2, activation=None))
        self.feature_encoding_layer = (PtSeq(self.feat_dim).conv1d(128, bn=True).conv1d(128, bn=True).conv1d(128, bn=True)
                                       .conv1d(self.feat_dim, activation=None, bias=False))
        self.normalize_feature_layer = pt_conv1d(self.feat_dim, self.feat_dim, bn=True)

    def pointwise_feature_matching(self, rgbd_feature, mesh_feature, x, parts=False):
        """The training matching loss of geoMatch_DGCNN.py:52-135 for the whole batch at once, WITHOUT the [B, N, M+1] similarity:
        value and gradients of the reference's per-item loop (mean over the items with >= 3 rows of `origin_labels == 1` of the
        mean circle loss of their rows).  What differs from the FFB6D variant (geoMatch.GeoMatch.pointwise_feature_matching):
          * the padding column is the unit vector e0 (:96-99): its similarity with a row is the row's first component;
          * a vertex v is a positive of a row with ground-truth vertex g when it is visible in the row's item and
            pdist(g, v) < positive_r / 1000 * z_i(v), z_i(v) = depth of v posed by the item's RT (:62-67): the radius depends on the
            item AND the vertex, so the positive tables are built per item (ops.circle_nbr_items, one launch for the batch) and the
            fused kernels index them by (item, g) -- ops.circle_match(..., pad="e0").
        soft_xyz_weight / soft_nll_weight / pose_loss_weight / parts: as in geoMatch.GeoMatch.pointwise_feature_matching."""
        from .loss import soft_assign_terms
        pose_on = self.pose_loss_weight != 0
        soft_on = self.soft_xyz_weight != 0 or self.soft_nll_weight != 0 or pose_on

        def result(match_loss, lx=None, ln=None, lp=None):
            if not soft_on:
                return (match_loss, None, None) if parts else match_loss
            if pose_on:                  # the pose-fit loss rides as a fourth part
                return (match_loss, lx, ln, lp) if parts else (match_loss + self.soft_xyz_weight * lx + self.soft_nll_weight * ln
                                                               + self.pose_loss_weight * lp)
            return (match_loss, lx, ln) if parts else match_loss + self.soft_xyz_weight * lx + self.soft_nll_weight * ln
        if not rgbd_feature.is_cuda:
            raise RuntimeError("GeoMatch (DGCNN) training matching loss runs on the GPU (HIP kernels); there is no CPU fallback")
        B, D, N = rgbd_feature.shape
        mesh = mesh_feature[0]
        M = mesh.shape[1]
        sel = x["origin_labels"] == 1
        counts = sel.sum(dim=1)
        item_ok = counts >= 3                                      # :112-113
        sel = sel & item_ok.unsqueeze(1)
        bi, pi = torch.nonzero(sel, as_tuple=True)                 # row-major: item, then point order
        if bi.numel() == 0:
            zero = torch.zeros((), device=mesh.device)
            return result(zero, zero, zero, zero)
        rows = F.normalize(rgbd_feature.transpose(1, 2)[bi, pi], p=2, dim=1)          # [R,128] (normalising a row commutes with selecting it)
        mesh_rows = F.normalize(mesh, p=2, dim=0).t().contiguous()                   # [M,128]; the padding column stays e0 under the normalisation
        g = x["match_idx"].long()[bi, pi]
        mesh_xyz = self.model_emb.mesh[0][:3, :].transpose(0, 1).contiguous()         # [M,3]
        RT = x["RT"].to(mesh_xyz.dtype)
        z = torch.matmul(mesh_xyz, RT[:, 2, :3].unsqueeze(2)).squeeze(2) + RT[:, 2, 3:4]     # [B,M]: third row of RT . v (:65)
        rad = (self.positive_r / 1000.0 * z).contiguous()
        lrow = ops.circle_match(rows, mesh_rows, g, bi, nbr=ops.circle_nbr_items(mesh_xyz, rad),
                                visb=ops.circle_visbits(x["visible_flag"]), gamma=16.0, m=0.2, pad="e0")
        per_item = torch.zeros(B, dtype=torch.float32, device=mesh.device).index_add_(0, bi, lrow)
        per_item = per_item[item_ok] / counts[item_ok].to(torch.float32)
        if not soft_on:
            return result(per_item.mean())
        lx, ln, *lp = soft_assign_terms(self, rows, mesh_rows, mesh_xyz, g, None, bi, pi, counts, x)
        return result(per_item.mean(), lx, ln, *lp)

    def forward(self, inputs, end_points=None, fused=False, defer_seg=False):
        """fused: both trunks on the fused inference path (dgcnn._DgcnnTrunk._embed_fused; eval only; raises in training mode).  In
        training mode `self.train_path == "fused"` sends both trunks through dgcnn._DgcnnTrunk._embed_train_fused.  defer_seg is accepted and
        ignored, as in geoMatch.GeoMatch: infer.pipeline_step passes it to every model."""
        if not end_points:
            end_points = {}
        x = inputs["cld_rgb_nrm"]
        if fused and settings.USE_SIDE_STREAMS and "mesh" in settings.SIDE_PARTS and (not self.training) and x.is_cuda and not torch.is_grad_enabled():
            # the mesh trunk depends on nothing in `inputs`: it runs on a side stream beside the cloud trunk
            with ops.fork(x.device, 1) as f:                 # reads module buffers / parameters only (never freed mid-step)
                mesh_features = self.model_emb(fused=True)
            rgbd_emb = self.pcd_emb(x, fused=True)
            f.join(mesh_features)
        else:
            if self.train_path not in ("modules", "fused"):
                raise ValueError("train_path must be 'modules' or 'fused', got %r" % (self.train_path,))
            train_fused = self.training and not fused and self.train_path == "fused"
            rgbd_emb = self.pcd_emb(x, fused=fused, train_fused=train_fused)          # cloud first, then mesh: the dropout masks of a
            mesh_features = self.model_emb(fused=fused, train_fused=train_fused)      # seed do not depend on the path
        rgbd_features = self.feature_encoding_layer(rgbd_emb)
        rgbd_normalized = self.normalize_feature_layer(rgbd_features)
        rgbd_emb = rgbd_emb + rgbd_normalized
        seg_features = self.seg_layer(rgbd_emb)
        if self.training:
            pose_on = self.pose_loss_weight != 0
            soft_on = self.soft_xyz_weight != 0 or self.soft_nll_weight != 0 or pose_on
            if soft_on:
                match_loss, soft_xyz_loss, soft_nll_loss, *pose_loss = self.pointwise_feature_matching(rgbd_features, mesh_features, inputs,
                                                                                                     parts=True)
            else:
                match_loss = self.pointwise_feature_matching(rgbd_features, mesh_features, inputs)
            seg_loss = self.seg_loss_func(seg_features, inputs["labels"].long())
            end_points["loss"] = self.awl(seg_loss, match_loss)
            end_points["seg_loss"] = seg_loss
            end_points["match_loss"] = match_loss
            if self.soft_xyz_weight != 0 or self.soft_nll_weight != 0:
                end_points["loss"] = end_points["loss"] + self.soft_xyz_weight * soft_xyz_loss + self.soft_nll_weight * soft_nll_loss
                end_points["soft_xyz_loss"] = soft_xyz_loss
                end_points["soft_nll_loss"] = soft_nll_loss
            if pose_on:
                end_points["loss"] = end_points["loss"] + self.pose_loss_weight * pose_loss[0]
                end_points["pose_loss"] = pose_loss[0]
        end_points["seg"] = seg_features
        end_points["mesh"] = mesh_features
        end_points["rgbd"] = rgbd_features
        return end_points
