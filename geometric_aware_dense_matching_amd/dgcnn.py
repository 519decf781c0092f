"""DGCNN embeddings for the geoMatch_DGCNN variant (BASELINE config 4).

Mirrors /root/reference/models/dgcnn.py: `DgcnnPcdEmb` :58-136 (cloud, k=16) and `DgcnnMeshEmb` :138-237
(object model, k=20).  Parameter names are identical (`bn1..bn8` AND their aliases `conv1.1 ...` inside the
Sequentials, `conv9`, buffer `mesh`).  The dynamic graph (dgcnn.py:21-56) is rebuilt three times per
forward: dense negative squared distances by one GEMM (same formula as the reference), row-wise top-k by a
HIP kernel, edge features cat(x_j - x_i, x_i) by a HIP kernel; the reference's hard-coded
`torch.device('cuda')` (:39) is gone.

Inference has a second, fused path (`forward(..., fused=True)`, `_DgcnnTrunk._embed_fused`): graphs by `knn_fused` (ops.feature_knn:
Gram tile and selection in one kernel, no [B,n,n] matrix), every edge stage by one per-point layer + ops.edge_block (no [B,2C,n,k]
tensor), conv6 .. conv9 by ops.pointwise over segments.  It folds the running statistics, so it raises in training mode.

Training has its own fused path (`forward(..., train_fused=True)`, `_DgcnnTrunk._embed_train_fused`; selected by
`geoMatch_DGCNN.GeoMatch.train_path = "fused"`): the same graphs and the same split of each stage's first convolution, with
ops.edge_block_train (train-mode BatchNorm over all edges, full backward, every pass recomputing its edges) in place of the edge
tensors, and a tail that never repeats the global feature.  Same parameters and state-dict names as the module path.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .derived import derived
from .layers import folded_bn, fused_eval
from .synthetic import COLOR_MEAN, COLOR_STD_MESH


def knn(x, k):
    """dgcnn.py:21-27: x f32[B,C,n] -> idx i32[B,n,k], nearest first (largest negative squared distance)."""
    gram = torch.matmul(x.transpose(2, 1), x)
    xx = torch.sum(x ** 2, dim=1)
    # pairwise_distance = -xx - (-2 * gram) - xx^T is formed inside the top-k kernel (same operations, same order)
    return ops.topk_negdist(gram, xx, k)


def knn_fused(feat, k):
    """The graph of the fused inference path: feat f32[B,C,n] -> idx i32[B,n,k], the same ranking as `knn` with the Gram tile and the
    selection in one kernel (ops.feature_knn): no [B,n,n] matrix.  The one seam the fused trunk builds its graphs through."""
    return ops.feature_knn(feat, k)


def get_graph_feature(x, k=20, idx=None, dim9=False):
    """dgcnn.py:30-56 -> f32[B,2C,n,k]."""
    x = x.contiguous()
    if idx is None:
        idx = knn(x[:, :3].contiguous(), k) if dim9 else knn(x, k)
    return ops.edge_feature(x, idx)


def _lrelu():
    return nn.LeakyReLU(negative_slope=0.2)


class _DgcnnTrunk(nn.Module):
    def _build(self, embed_dim, feat_dim, dropout):
        self.bn1 = nn.BatchNorm2d(64)
        self.bn2 = nn.BatchNorm2d(64)
        self.bn3 = nn.BatchNorm2d(64)
        self.bn4 = nn.BatchNorm2d(64)
        self.bn5 = nn.BatchNorm2d(64)
        self.bn6 = nn.BatchNorm1d(embed_dim)
        self.bn7 = nn.BatchNorm1d(512)
        self.bn8 = nn.BatchNorm1d(256)
        self.conv1 = nn.Sequential(nn.Conv2d(18, 64, kernel_size=1, bias=False), self.bn1, _lrelu())
        self.conv2 = nn.Sequential(nn.Conv2d(64, 64, kernel_size=1, bias=False), self.bn2, _lrelu())
        self.conv3 = nn.Sequential(nn.Conv2d(64 * 2, 64, kernel_size=1, bias=False), self.bn3, _lrelu())
        self.conv4 = nn.Sequential(nn.Conv2d(64, 64, kernel_size=1, bias=False), self.bn4, _lrelu())
        self.conv5 = nn.Sequential(nn.Conv2d(64 * 2, 64, kernel_size=1, bias=False), self.bn5, _lrelu())
        self.conv6 = nn.Sequential(nn.Conv1d(192, embed_dim, kernel_size=1, bias=False), self.bn6, _lrelu())
        self.conv7 = nn.Sequential(nn.Conv1d(embed_dim + 192, 512, kernel_size=1, bias=False), self.bn7, _lrelu())
        self.conv8 = nn.Sequential(nn.Conv1d(512, 256, kernel_size=1, bias=False), self.bn8, _lrelu())
        self.dp1 = nn.Dropout(dropout)
        self.conv9 = nn.Conv1d(256, feat_dim, kernel_size=1, bias=False)

    def _cba(self, seq, x, maxk=False):
        """conv + BatchNorm + LeakyReLU (+ max over the neighbour dimension): eval mode folds BN + activation (+ max) into one pass."""
        if fused_eval(x, self) and (not maxk or (x.dim() == 4 and x.shape[-1] % 4 == 0 and x.shape[0] * seq[0].out_channels <= 65535)):
            y = seq[0](x)
            scale, shift = folded_bn(seq[1])
            slope = float(seq[2].negative_slope)
            if maxk:
                return ops.affine_act_maxk(y, scale, shift, ops.ACT_LEAKY, slope)
            if y.numel() // (y.shape[0] * y.shape[1]) % 4 == 0 and y.shape[0] * y.shape[1] <= 65535:
                return ops.affine_act(y, scale, shift, ops.ACT_LEAKY, slope)
            return seq[2](seq[1](y))
        y = seq(x)
        return y.max(dim=-1, keepdim=False)[0] if maxk else y

    def _embed(self, x):
        num_points = x.size(2)
        x = get_graph_feature(x, k=self.k, dim9=True)
        x1 = self._cba(self.conv2, self._cba(self.conv1, x), maxk=True)
        x = get_graph_feature(x1, k=self.k)
        x2 = self._cba(self.conv4, self._cba(self.conv3, x), maxk=True)
        x = get_graph_feature(x2, k=self.k)
        x3 = self._cba(self.conv5, x, maxk=True)
        x = self._cba(self.conv6, torch.cat((x1, x2, x3), dim=1))
        x = x.max(dim=-1, keepdim=True)[0].repeat(1, 1, num_points)
        x = torch.cat((x, x1, x2, x3), dim=1)
        x = self._cba(self.conv8, self._cba(self.conv7, x))
        return self.conv9(self.dp1(x))

    # -- fused inference path: HIP operators only, neither [B,n,n] distances nor [B,2C,n,k] edge tensors --------------------------
    @staticmethod
    def _wt(conv):
        """The weight of a 1x1 convolution transposed to [Cin,Cout], as ops.pointwise reads it."""
        return derived(conv, "wt", (conv.weight,), lambda: conv.weight.reshape(conv.weight.shape[0], -1).t().contiguous())

    @staticmethod
    def _edge_wt(conv):
        """The first convolution of an edge stage, W = [W_a | W_b] over cat(x_j - x_i, x_i), split per point:
        W cat(x_j - x_i, x_i) = W_a x_j + (W_b - W_a) x_i  ->  the stacked weight [W_a ; W_b - W_a] transposed to [C,128]."""
        def make():
            w = conv.weight.reshape(conv.weight.shape[0], -1)
            c = w.shape[1] // 2
            return torch.cat((w[:, :c], w[:, c:] - w[:, :c]), dim=0).t().contiguous()
        return derived(conv, "edge_wt", (conv.weight,), make)

    def _edge_stage(self, x, idx, seq1, seq2, out):
        """conv (+ conv) of one edge stage and the max over the neighbours -> out f32[B,64,n]; x f32[B,C,n], idx i32[B,n,k]."""
        pq = ops.pointwise([x], self._edge_wt(seq1[0]), point_major=True)          # [B,n,128]: both halves of the split, one launch
        s1, t1 = folded_bn(seq1[1])
        w2 = s2 = t2 = None
        if seq2 is not None:
            w2 = seq2[0].weight
            s2, t2 = folded_bn(seq2[1])
        return ops.edge_block(pq, idx, s1, t1, w2, s2, t2, float(seq1[2].negative_slope), out=out)

    def _pw(self, seq, segs):
        scale, shift = folded_bn(seq[1])
        return ops.pointwise(segs, self._wt(seq[0]), scale, shift, ops.ACT_LEAKY, float(seq[2].negative_slope))

    def _embed_fused(self, x):
        """`_embed` in eval mode on HIP operators alone (the max over the points excepted): graphs by `knn_fused`, every edge stage by
        one per-point layer + ops.edge_block, conv6 .. conv9 by ops.pointwise over segments (no cat, no repeat).  No backward: training
        has `_embed_train_fused`."""
        if self.training:
            raise RuntimeError("the fused DGCNN path is inference only (it has no backward): call .eval() or pass fused=False")
        if not x.is_cuda:
            raise RuntimeError("the fused DGCNN path runs on the GPU (HIP kernels); there is no CPU fallback")
        x = x.contiguous()
        B, _, n = x.shape
        # x1, x2, x3: three contiguous [B,64,n] slices of one allocation, read as segments by conv6 / conv7 (cat(x1, x2, x3) is never formed)
        x1, x2, x3 = torch.empty((3, B, 64, n), dtype=torch.float32, device=x.device).unbind(0)
        self._edge_stage(x, knn_fused(x[:, :3], self.k), self.conv1, self.conv2, x1)       # the graph from xyz, the features from all 9 channels
        self._edge_stage(x1, knn_fused(x1, self.k), self.conv3, self.conv4, x2)
        self._edge_stage(x2, knn_fused(x2, self.k), self.conv5, None, x3)
        g = self._pw(self.conv6, [x1, x2, x3]).max(dim=-1, keepdim=True)[0]                 # [B,embed,1]
        # the global feature is read by every point through an all-zero index: a constant of the shape, made once per trunk
        everywhere = derived(self, "zero_idx", (), lambda: torch.zeros((B, n), dtype=torch.int32, device=x.device), extra=(B, n, str(x.device)))
        y = self._pw(self.conv8, [self._pw(self.conv7, [(g, everywhere), x1, x2, x3])])
        return ops.pointwise([y], self._wt(self.conv9))                                     # dropout is the identity in eval

    # -- fused TRAINING path: the same structure under autograd ---------------------------------------------------------------------
    def _edge_stage_train(self, x, idx, seq1, seq2):
        """One edge stage in training mode -> f32[B,64,n].  The split weight [W_a ; W_b - W_a] is built with torch operations, so autograd
        reaches conv.weight; the per-point layer's two gradient products are small batched GEMMs (ops.pointwise_pm_train)."""
        w = seq1[0].weight.reshape(seq1[0].weight.shape[0], -1)
        c = w.shape[1] // 2
        pq = ops.pointwise_pm_train(x, torch.cat((w[:, :c], w[:, c:] - w[:, :c]), dim=0))   # [B,n,128]
        if seq2 is None:
            return ops.edge_block_train(pq, idx, seq1[1], slope=float(seq1[2].negative_slope))
        return ops.edge_block_train(pq, idx, seq1[1], seq2[0].weight, seq2[1], slope=float(seq1[2].negative_slope))

    @staticmethod
    def _bn_act_train(seq, y):
        if ops.bn_train_supported(y, seq[1]):
            return ops.batch_norm_act_train(y, seq[1], ops.ACT_LEAKY, float(seq[2].negative_slope))
        return seq[2](seq[1](y))

    def _embed_train_fused(self, x):
        """`_embed` in training mode without [B,n,n] distances, [B,2C,n,k] edge tensors or the repeated global feature.  Graphs by
        `knn_fused` (no gradient flows through indices, as in `_embed`); stages by `_edge_stage_train`; conv6 .. conv9 by the
        differentiable per-point operators; conv7(cat(g_rep, x123)) = W7[:, :embed] g + W7[:, embed:] x123 with the first term
        [B,512,1] broadcast.  Dropout is self.dp1, called once per trunk as in `_embed`."""
        if not self.training:
            raise RuntimeError("the fused DGCNN training path needs training mode (batch statistics): call .train(), or use fused=True for inference")
        if not x.is_cuda:
            raise RuntimeError("the fused DGCNN path runs on the GPU (HIP kernels); there is no CPU fallback")
        x = x.contiguous()
        with torch.no_grad():
            idx = knn_fused(x[:, :3], self.k)
        x1 = self._edge_stage_train(x, idx, self.conv1, self.conv2)
        with torch.no_grad():
            idx = knn_fused(x1.detach(), self.k)
        x2 = self._edge_stage_train(x1, idx, self.conv3, self.conv4)
        with torch.no_grad():
            idx = knn_fused(x2.detach(), self.k)
        x3 = self._edge_stage_train(x2, idx, self.conv5, None)
        x123 = torch.cat((x1, x2, x3), dim=1)                                                # [B,192,n]
        g = self._bn_act_train(self.conv6, ops.conv1x1_train(self.conv6[0], x123)).max(dim=-1, keepdim=True)[0]      # [B,embed,1]
        w7 = self.conv7[0].weight.reshape(self.conv7[0].weight.shape[0], -1)
        e = g.shape[1]
        y = ops.conv1x1_train_w(x123, w7[:, e:].contiguous()) + torch.matmul(w7[:, :e], g)   # the global term is one column per item
        y = self._bn_act_train(self.conv7, y)
        y = self._bn_act_train(self.conv8, ops.conv1x1_train(self.conv8[0], y))
        return ops.conv1x1_train(self.conv9, self.dp1(y))


class DgcnnPcdEmb(_DgcnnTrunk):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.k = args.get("k", 16)
        self.embed_dim = args.get("embed_dim", 1024)
        self.feat_dim = args.get("feat_dim", 128)
        self.dropout = args.get("dropout", 0.1)
        self._build(self.embed_dim, self.feat_dim, self.dropout)

    def forward(self, x, fused=False, train_fused=False):
        if fused:
            return self._embed_fused(x)
        return self._embed_train_fused(x) if train_fused else self._embed(x)


class DgcnnMeshEmb(_DgcnnTrunk):
    def __init__(self, args, cls_id, model_points=None):
        super().__init__()
        self.args = args
        self.k = args.get("k", 20)
        self.feat_dim = args.get("feat_dim", 128)
        self.embed_dim = args.get("embed_dim", 1024)
        self.dropout = args.get("dropout", 0.1)
        self.model_pth = args.get("model_pth", "datasets/ycb/ycbv/bop_ycb_kps")
        self.model_id = cls_id
        self.n_mesh_node = args.get("n_mesh_node", 2048)
        self.load_mesh(model_points)
        self._build(self.embed_dim, self.feat_dim, self.dropout)
        self.sys_corr_idx = None

    def load_mesh(self, model_points=None):
        """dgcnn.py:188-202: rows xyz (m), rgb normalised (std .229,.224,.225), normal -> buffer mesh [1,9,M]."""
        if model_points is None:
            model_points = np.load(os.path.join(self.model_pth, "obj_%06d_fps.npy" % self.model_id))
        data = np.asarray(model_points)[: self.n_mesh_node, :9].astype(np.float64)
        data[:, :3] = data[:, :3].astype(np.float32) / 1000.0
        x = data[:, 3:6] / 255.0
        x -= COLOR_MEAN.astype(np.float64)
        x /= COLOR_STD_MESH.astype(np.float64)
        data[:, 3:6] = x
        self.register_buffer("mesh", torch.from_numpy(data.T[np.newaxis, :, :]).float())

    @property
    def xyz(self):
        return self.mesh[0, :3].t()

    def forward(self, fused=False, train_fused=False):
        if fused or train_fused:
            # the buffer is a transposed view of the loaded rows: its channel-major copy is made once, not per step
            mesh = derived(self, "mesh_cm", (self.mesh,), lambda: self.mesh.contiguous())
            return self._embed_fused(mesh) if fused else self._embed_train_fused(mesh)
        return self._embed(self.mesh)
