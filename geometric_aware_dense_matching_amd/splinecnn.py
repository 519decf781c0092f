"""Object-model (mesh) embedding: kNN graph (k=4) + Cartesian pseudo-coordinates + 3 SplineConv
layers + concat + Linear(393,128).  Mirrors /root/reference/models/SplineCNN.py:101-251.

torch_geometric / torch_spline_conv / torch_cluster are third-party, un-vendored and absent here
(reference README.md:24-25), so the graph transform and SplineConv are re-stated from their
published definitions (see csrc/gdm_spline.hip and DESIGN.md: parity unpinned for this op):
  KNNGraph(k=4)  : for every vertex its 4 nearest other vertices; edges neighbour -> centre
  Cartesian()    : attr = (pos_j - pos_i) / (2 max|.|) + 0.5 over all edges
  SplineConv     : dim 3, kernel 5^3, degree 1, open, aggr mean, root weight, bias

MI355X formulation: the dense part of SplineConv is one GEMM X @ [W_0|...|W_124]
(hipBLASLt through torch.matmul), the sparse part (basis, 8-row gather, mean, root, bias, ReLU) is
one HIP kernel over CSR edges (ops below).  The graph's kNN runs on the HIP kNN kernel.
Inference runs the edge-grouped form instead (only the (source, kernel index) pairs some edge needs are multiplied, no table), and so
does training with `SplineCNN_Mesh.train_path = "grouped"`, whose backward gathers through the inverse maps of build_spline_pairs.

The embedding is input independent (`forward()` takes no arguments, SplineCNN.py:234); the
reference nevertheless recomputes it on every GeoMatch.forward (geoMatch.py:179).  `forward`
recomputes too (training needs it); `GeoMatch(cache_mesh_in_eval=True)` may reuse it in eval.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import ops, settings
from ._lib import call
from .derived import derived
from .layers import cached_gemm_weight
from .synthetic import COLOR_MEAN, COLOR_STD_MESH

KERNEL_SIZE = 5


class _SplineAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xw, root, bias, rowptr, src, attr, relu):
        M, nk, C = xw.shape
        out = torch.empty((M, C), dtype=torch.float32, device=xw.device)
        call("gdm_spline_aggregate_hip", xw, rowptr, src, attr, root, bias, M, C, KERNEL_SIZE, int(relu), out)
        ctx.save_for_backward(rowptr, src, attr, out)
        ctx.relu = relu
        ctx.nk = nk
        return out

    @staticmethod
    def backward(ctx, go):
        rowptr, src, attr, out = ctx.saved_tensors
        go = go.contiguous()
        if ctx.relu:
            go = go * (out > 0).to(go.dtype)
        M, C = go.shape
        gxw = torch.zeros((M, ctx.nk, C), dtype=torch.float32, device=go.device)
        call("gdm_spline_aggregate_bwd_hip", go, rowptr, src, attr, M, C, KERNEL_SIZE, gxw)
        return gxw, go, go.sum(dim=0), None, None, None, None


def _pairs_grad(go, out, pairs, relu, want_packed):
    """gY f32[R,C] of the pair rows (gdm_spline_pairs_grad_hip: gather form, ReLU mask inside), and its packed operand if wanted."""
    M, C = go.shape
    R = pairs["rowidx"].shape[0]
    gy = torch.empty((R, C), dtype=torch.float32, device=go.device)
    pk = ops.spline_packed_buffer(C, R, go.device) if want_packed else None
    call("gdm_spline_pairs_grad_hip", go, out if relu else None, pairs["pair_ptr"], pairs["pair_ec"], pairs["basis"],
         pairs["tgt"], pairs["inv_deg"], R, C, gy, pk)
    return gy, pk


def _spline_wgrad(x, gy, pairs, cin, cout):
    """dW f32[125,cin,cout] = per kernel index X[rowidx]^T gY over its block of pair rows (gdm_spline_wgrad_hip, exact-fp32 MFMA:
    per-tile partial products, then their sum in ascending tile order)."""
    nk = KERNEL_SIZE ** 3
    R = pairs["rowidx"].shape[0]
    dw = torch.empty((nk, cin, cout), dtype=torch.float32, device=x.device)
    part = torch.empty((R // 256, cin, cout), dtype=torch.float32, device=x.device)          # per-tile partial products
    call("gdm_spline_wgrad_hip", x, pairs["rowidx"], gy, pairs["tile_co0"], pairs["blk_start"], pairs["blk_rows"], nk, R, cin, cout, part,
         dw)
    return dw


def _train_gemm_weight(conv, tag, w, make):
    """Packed split-bf16 GEMM weight made from the tensor `w` the Function was given (or saved), cached on `conv` under `tag` until
    `w` changes.  While a hipGraph is being captured the pack runs (and is captured) every time: a cache hit there would leave the
    pack out of the graph, and replays after an optimizer step would multiply by stale weights."""
    if torch.cuda.is_current_stream_capturing():
        with torch.no_grad():
            return ops.gemm_pack_weight(make(w).contiguous())
    return cached_gemm_weight(conv, tag, lambda: make(w), (w,))[0]


def _train_root_t(conv, lin_weight):
    """lin_weight^T (the slot SplineConv._root_t fills) from the tensor the Function was given; recomputed (and captured) while a
    hipGraph is being captured, as _train_gemm_weight."""
    if torch.cuda.is_current_stream_capturing():
        with torch.no_grad():
            return lin_weight.t().contiguous()
    return derived(conv, "root_t", (lin_weight,), lambda: lin_weight.t().contiguous())


class _SplineDirectTrain(torch.autograd.Function):
    """First layer (cin <= 16, input without gradient) in training: the forward is gdm_spline_direct3_hip as in inference; the backward
    gathers the pair gradient gY and forms dW on the grouped weight-gradient kernel.  Saved: x, out and the static maps -- no table."""

    @staticmethod
    def forward(ctx, x, weight, lin_weight, bias, conv, rowptr, src, attr, pairs, relu):
        M = x.shape[0]
        out = torch.empty((M, conv.cout), dtype=torch.float32, device=x.device)
        root_t = _train_root_t(conv, lin_weight)
        call("gdm_spline_direct3_hip", x, weight, rowptr, src, attr, root_t, bias, M, conv.cin, conv.cout, KERNEL_SIZE, int(relu), out,
             None, None, int(settings.SPLINE_LDS_WEIGHTS))
        ctx.save_for_backward(x, out)
        ctx.pairs, ctx.relu, ctx.dims = pairs, relu, (conv.cin, conv.cout)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        x, out = ctx.saved_tensors
        go = go.contiguous()
        cin, cout = ctx.dims
        gy, _ = _pairs_grad(go, out, ctx.pairs, ctx.relu, False)
        dw = _spline_wgrad(x, gy, ctx.pairs, cin, cout)
        g = go * (out > 0).to(go.dtype) if ctx.relu else go
        return None, dw, g.t() @ x, g.sum(dim=0), None, None, None, None, None, None


class _SplineGroupedTrain(torch.autograd.Function):
    """128 -> 128 layer in training on the edge-grouped form.  Forward: the launches of the inference path (pack, gdm_gemm_grouped_hip,
    root product, gdm_spline_pairs_aggregate3_hip).  Backward: gY by gather over the pair -> (edge, corner) lists; dX = segment sum
    over the source -> pair-row lists of Z = gY . W[k]^T (the same grouped GEMM, identity gather) + g . W_root; dW on the grouped
    weight-gradient kernel.  Saved: x, out and the static maps; Y is not kept."""

    @staticmethod
    def forward(ctx, x, weight, lin_weight, bias, conv, rowptr, pairs, relu):
        M = x.shape[0]
        nk = KERNEL_SIZE ** 3
        wpk = _train_gemm_weight(conv, "dense", weight, lambda w: w.permute(0, 2, 1).reshape(nk * conv.cout, conv.cin))
        xt = x.t().contiguous().unsqueeze(0)
        Y = ops.gemm_grouped(xt, wpk, pairs["rowidx"], pairs["tile_co0"], nk * conv.cout)
        if settings.USE_POINTWISE:
            root = ops.pointwise([xt], _train_root_t(conv, lin_weight), point_major=True).view(M, conv.cout)
        else:
            root = x @ lin_weight.t()
        out = torch.empty((M, conv.cout), dtype=torch.float32, device=x.device)
        call("gdm_spline_pairs_aggregate3_hip", Y, rowptr, pairs["pos"], pairs["basis"], root, bias, M, conv.cout, int(relu), out, None,
             None)
        ctx.save_for_backward(x, out, weight, lin_weight)
        ctx.conv, ctx.pairs, ctx.relu = conv, pairs, relu
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        x, out, weight, lin_weight = ctx.saved_tensors          # the saved weights: an in-place update since the forward raises here
        conv, pairs = ctx.conv, ctx.pairs
        go = go.contiguous()
        M = x.shape[0]
        nk = KERNEL_SIZE ** 3
        R = pairs["rowidx"].shape[0]
        gy, pk = _pairs_grad(go, out, pairs, ctx.relu, ctx.needs_input_grad[0])
        g = go * (out > 0).to(go.dtype) if ctx.relu else go
        dx = None
        if ctx.needs_input_grad[0]:
            # Z[r, :] = gY[r, :] . W[k(r)]^T: rows of weight.reshape(125*cin, cout) are (k, ci); cin == cout, so tile_co0 = k*cin as it stands
            wpk = _train_gemm_weight(conv, "dgrad", weight, lambda w: w.reshape(nk * conv.cin, conv.cout))
            Z = torch.empty((R, conv.cin), dtype=torch.float32, device=x.device)
            call("gdm_gemm_grouped_hip", pk, wpk, pairs["rowid"], pairs["tile_co0"], R, R, conv.cout, nk * conv.cin, Z)
            add = g @ lin_weight
            dx = torch.empty((M, conv.cin), dtype=torch.float32, device=x.device)
            call("gdm_spline_segment_sum_hip", Z, pairs["src_ptr"], pairs["src_rows"], add, M, conv.cin, dx)
        dw = _spline_wgrad(x, gy, pairs, conv.cin, conv.cout)
        return dx, dw, g.t() @ x, g.sum(dim=0), None, None, None, None


class SplineConv(nn.Module):
    """torch_geometric.nn.SplineConv(in, out, dim=3, kernel_size=5) parameter layout:
    weight [125, in, out], lin.weight [out, in] (root), bias [out]."""

    def __init__(self, cin, cout):
        super().__init__()
        self.cin, self.cout = cin, cout
        self.weight = nn.Parameter(torch.empty(KERNEL_SIZE ** 3, cin, cout))
        self.lin = nn.Linear(cin, cout, bias=False)
        self.bias = nn.Parameter(torch.zeros(cout))
        bound = 1.0 / np.sqrt(cin * KERNEL_SIZE ** 3)
        nn.init.uniform_(self.weight, -bound, bound)
        nn.init.uniform_(self.lin.weight, -bound, bound)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        old = prefix + "root"                                  # torch_geometric 1.x name: root [in, out]
        if old in state_dict and prefix + "lin.weight" not in state_dict:
            state_dict[prefix + "lin.weight"] = state_dict.pop(old).t().contiguous()
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _root_t(self):
        return derived(self, "root_t", (self.lin.weight,), lambda: self.lin.weight.t().contiguous())

    def forward_direct_cm(self, x, rowptr, src, attr, relu):
        """First layer (cin <= 16), result CHANNEL-major f32[1, cout, M]: what the next layer's grouped GEMM / root product and the
        final linear read in place (no transposing copy)."""
        return self.forward_direct_cm_packed(x, rowptr, src, attr, relu, False)[0]

    def forward_direct_cm_packed(self, x, rowptr, src, attr, relu, want_packed):
        """... and, want_packed, ALSO as the packed split-bf16 operand of the next layer's grouped GEMM (the kernel writes it itself: no
        pack launch between the layers).  Returns (out_t, packed buffer or None)."""
        M = x.shape[0]
        out_t = torch.empty((1, self.cout, M), dtype=torch.float32, device=x.device)
        pk = ops.spline_packed_buffer(self.cout, M, x.device) if want_packed and ops.spline_packed_supported(self.cout) else None
        xc = x.contiguous()
        call("gdm_spline_direct3_hip", xc, self.weight, rowptr, src, attr, self._root_t(), self.bias, M, self.cin, self.cout, KERNEL_SIZE,
             int(relu), None, out_t, pk, int(settings.SPLINE_LDS_WEIGHTS))
        return out_t, pk

    def forward_grouped_cm(self, xt, rowptr, pairs, relu, xpk=None, want_packed=False):
        """128 -> 128 layer on the edge-grouped GEMM, channel-major in (xt f32[1, cin, M]) and out (f32[1, cout, M]).  xpk: xt's packed
        operand when the previous layer wrote it; want_packed: this layer's result also as the next layer's -> (out_t, packed or None)."""
        M = xt.shape[2]
        nk = KERNEL_SIZE ** 3
        wpk, _ = cached_gemm_weight(self, "dense", lambda: self.weight.permute(0, 2, 1).reshape(nk * self.cout, self.cin), (self.weight,))
        Y = ops.gemm_grouped(xt, wpk, pairs["rowidx"], pairs["tile_co0"], nk * self.cout, xpk=xpk)
        root = ops.pointwise([xt], self._root_t(), point_major=True)                       # [1, M, cout] = x @ W_root^T
        out_t = torch.empty((1, self.cout, M), dtype=torch.float32, device=xt.device)
        pk = ops.spline_packed_buffer(self.cout, M, xt.device, avoid=xpk) if want_packed and ops.spline_packed_supported(self.cout) else None
        call("gdm_spline_pairs_aggregate3_hip", Y, rowptr, pairs["pos"], pairs["basis"], root, self.bias, M, self.cout, int(relu), None,
             out_t, pk)
        return out_t, pk

    def train_grouped_ok(self, x, pairs):
        """Whether forward_train_grouped serves this layer: a first layer (cin <= 16, input without gradient) or a 128 -> 128 layer,
        on the GPU, with the pairs' inverse maps."""
        if not (x.is_cuda and pairs is not None and "inv_deg" in pairs and self.cout == 128 and self.lin.bias is None):
            return False
        if self.cin <= 16:
            return not x.requires_grad
        return self.cin == 128 and settings.USE_MFMA_GEMM and settings.USE_GROUPED_SPLINE

    def forward_train_grouped(self, x, rowptr, src, attr, relu, pairs):
        """Differentiable layer without the [M, 125*cout] table (SplineCNN_Mesh.train_path = "grouped"): same launches as inference
        forward, gather-form backward (_SplineDirectTrain / _SplineGroupedTrain)."""
        x = x.contiguous()
        if self.cin <= 16:
            return _SplineDirectTrain.apply(x, self.weight, self.lin.weight, self.bias, self, rowptr, src, attr, pairs, relu)
        return _SplineGroupedTrain.apply(x, self.weight, self.lin.weight, self.bias, self, rowptr, pairs, relu)

    def forward(self, x, rowptr, src, attr, relu=False, pairs=None):
        M = x.shape[0]
        nk = KERNEL_SIZE ** 3
        if self.cin <= 16 and x.is_cuda and not torch.is_grad_enabled():
            # few input channels (first layer, 9 -> 128): messages formed directly, no [M, 125*out] table (524 MB at M = 8192)
            out = torch.empty((M, self.cout), dtype=torch.float32, device=x.device)
            xc = x.contiguous()
            call("gdm_spline_direct3_hip", xc, self.weight, rowptr, src, attr, self._root_t(), self.bias, M, self.cin, self.cout,
                 KERNEL_SIZE, int(relu), out, None, None, int(settings.SPLINE_LDS_WEIGHTS))
            return out
        if (settings.USE_MFMA_GEMM and settings.USE_GROUPED_SPLINE and pairs is not None and not torch.is_grad_enabled() and x.is_cuda
                and self.cin % 128 == 0 and self.cout == 128):
            # edge-grouped form: only the (source, kernel index) pairs some edge needs are multiplied (about a quarter of the dense
            # [M, 125*out] table, which is then never written), on the same split-bf16 MFMA kernel with gathered rows
            wpk, _ = cached_gemm_weight(self, "dense", lambda: self.weight.permute(0, 2, 1).reshape(nk * self.cout, self.cin),
                                        (self.weight,))
            xt = x.t().contiguous().unsqueeze(0)                     # [1, cin, M] channel-major: the GEMM's and the root layer's operand
            Y = ops.gemm_grouped(xt, wpk, pairs["rowidx"], pairs["tile_co0"], nk * self.cout)
            if settings.USE_POINTWISE and self.lin.bias is None:
                root = ops.pointwise([xt], self._root_t(), point_major=True).view(M, self.cout)      # x @ W_root^T on the own kernel
            else:
                root = self.lin(x)
            out = torch.empty((M, self.cout), dtype=torch.float32, device=x.device)
            call("gdm_spline_pairs_aggregate3_hip", Y, rowptr, pairs["pos"], pairs["basis"], root, self.bias, M, self.cout, int(relu), out,
                 None, None)
            return out
        if (settings.USE_MFMA_GEMM and not torch.is_grad_enabled() and x.is_cuda
                and ops.gemm_supported(self.cin, nk * self.cout, M, 1)):
            # dense part on the split-bf16 MFMA GEMM, written node-major ([M, 125*out]) as the aggregation kernel reads it
            wpk, _ = cached_gemm_weight(self, "dense", lambda: self.weight.permute(0, 2, 1).reshape(nk * self.cout, self.cin),
                                        (self.weight,))
            xw = ops.gemm_bf16x3(x.t().contiguous().unsqueeze(0), wpk, nk * self.cout, pixel_major=True).view(M, nk, self.cout)
            root = self.lin(x)
            return _SplineAggregate.apply(xw, root, self.bias, rowptr, src, attr, relu)
        w = self.weight.permute(1, 0, 2).reshape(self.cin, -1)            # [in, 125*out]
        xw = torch.matmul(x, w).view(M, KERNEL_SIZE ** 3, self.cout)      # dense GEMM
        root = self.lin(x)
        return _SplineAggregate.apply(xw, root, self.bias, rowptr, src, attr, relu)


def mesh_node_features(model_pts):
    """utils/ply.py:519-535 read_ply_to_data: x = [rgb normalised (std .229,.224,.225), xyz (m), normal]."""
    rgb = model_pts[:, 3:6].astype(np.uint8).astype(np.float64) / 255.0
    rgb = (rgb - COLOR_MEAN.astype(np.float64)) / COLOR_STD_MESH.astype(np.float64)
    xyz = model_pts[:, :3].astype(np.float32) / 1000.0
    x = np.concatenate([rgb, xyz, model_pts[:, 6:9].astype(np.float32)], axis=-1)
    return torch.tensor(x, dtype=torch.float32), torch.tensor(xyz, dtype=torch.float32)


def build_mesh_graph(pos, k=4):
    """KNNGraph(k) + Cartesian() on the GPU. pos f32[M,3] (cuda) -> edge_index i64[2,E] (row 0 = neighbour j,
    row 1 = centre i, grouped by centre, ascending distance), edge_attr f32[E,3]."""
    M = pos.shape[0]
    idx = ops.knn_batch(pos[None], pos[None], k + 1)[0].long()           # [M,k+1], self first (d=0)
    centre = torch.arange(M, device=pos.device).unsqueeze(1).expand(M, k + 1)
    keep = idx != centre                                                 # knn_graph(loop=False): drop self loops
    # exactly one self hit per row unless duplicate vertices tie at distance 0; keep the first k others
    order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)[:, :k]
    nbr = torch.gather(idx, 1, order)
    row = nbr.reshape(-1)
    col = centre[:, :k].reshape(-1)
    cart = pos[row] - pos[col]
    cart = cart / (2 * cart.abs().max()) + 0.5
    return torch.stack([row, col], dim=0), cart


def build_spline_pairs(src, attr, M, cout=128, rowptr=None):
    """Static bookkeeping of the edge-grouped SplineConv: the unique (source vertex, kernel index) pairs the edges need, sorted by
    kernel index and padded per kernel index to whole 256-row tiles.  src i32[E] / attr f32[E,3] in CSR (target-sorted) order.
    -> dict(rowidx i32[R], tile_co0 i32[R/256], pos i32[E,8], basis f32[E,8]).  Same fp32 arithmetic as spline_aggregate_kernel.

    Given rowptr i32[M+1] (the CSR the edges are sorted by), also the inverse maps the training path (SplineCNN_Mesh.train_path =
    "grouped") reads, built with torch ops that run on CPU tensors too (SplineCNN_Mesh builds them the first time that path is taken):
      pair_ptr i32[R+1], pair_ec i32[8E]   pair row -> its (edge, corner) uses e*8+s, ascending; padding rows have empty lists
      src_ptr i32[M+1], src_rows i32[U]    source vertex -> its pair rows, ascending; the U real pairs only, never a padding row
      blk_start, blk_rows i32[125]         first row and row count of every kernel index' block, padding excluded
      rowid i32[R]                         0..R-1: the identity gather of the input-gradient GEMM
      tgt i32[E], inv_deg f32[M]           target vertex of every edge; 1 / in-degree (0 for a vertex without incoming edges)"""
    ks = KERNEL_SIZE
    v = attr * float(ks - 1)
    f = torch.floor(v)
    fl = f.to(torch.int64)
    fr = v - f
    E = src.shape[0]
    wi = torch.zeros((E, 8), dtype=torch.int64, device=src.device)
    basis = torch.ones((E, 8), dtype=torch.float32, device=src.device)
    for s_ in range(8):
        off = 1
        for d in range(3):
            kd = (s_ >> d) & 1
            wi[:, s_] += ((fl[:, d] + kd) % ks) * off
            off *= ks
            basis[:, s_] = basis[:, s_] * (fr[:, d] if kd else 1.0 - fr[:, d])
    key = wi * M + src.to(torch.int64)[:, None]                       # sorts by kernel index, then source
    uniq, inv = torch.unique(key.reshape(-1), sorted=True, return_inverse=True)
    pw = uniq // M                                                     # kernel index of every unique pair
    counts = torch.bincount(pw, minlength=ks ** 3)
    padded = (counts + 255) // 256 * 256
    start = torch.cumsum(padded, 0) - padded                          # first row of each kernel index' block
    first = torch.cumsum(counts, 0) - counts                          # first unique-pair id of each kernel index
    row = start[pw] + (torch.arange(uniq.shape[0], device=src.device) - first[pw])
    R = max(int(padded.sum().item()), 256)
    rowidx = torch.zeros(R, dtype=torch.int32, device=src.device)
    rowidx[row] = (uniq % M).to(torch.int32)
    tile_k = torch.repeat_interleave(torch.arange(ks ** 3, device=src.device), padded // 256)
    tile_co0 = torch.zeros(R // 256, dtype=torch.int32, device=src.device)
    tile_co0[: tile_k.shape[0]] = (tile_k * cout).to(torch.int32)
    pairs = dict(rowidx=rowidx.contiguous(), tile_co0=tile_co0.contiguous(), pos=row[inv].view(E, 8).to(torch.int32).contiguous(),
                 basis=basis.contiguous())
    if rowptr is None:
        return pairs
    i32 = lambda t: t.to(torch.int32).contiguous()
    ptr = lambda counts_: torch.cat((counts_.new_zeros(1), torch.cumsum(counts_, 0)))
    pos_flat = row[inv]                                                # pair row of every (edge, corner), flat index e*8+s
    pairs["pair_ptr"] = i32(ptr(torch.bincount(pos_flat, minlength=R)))
    pairs["pair_ec"] = i32(torch.argsort(pos_flat, stable=True))       # stable: ascending (edge, corner) inside a row
    pair_src = uniq % M                                                # `row` ascends with the unique-pair id
    pairs["src_ptr"] = i32(ptr(torch.bincount(pair_src, minlength=M)))
    pairs["src_rows"] = i32(row[torch.argsort(pair_src, stable=True)])
    pairs["blk_start"] = i32(start)
    pairs["blk_rows"] = i32(counts)
    pairs["rowid"] = torch.arange(R, dtype=torch.int32, device=src.device)
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.int64)
    pairs["tgt"] = i32(torch.repeat_interleave(torch.arange(M, device=src.device), deg))
    pairs["inv_deg"] = torch.where(deg > 0, 1.0 / deg.clamp(min=1).to(torch.float32), torch.zeros((), device=src.device)).contiguous()
    return pairs


class SplineCNN_Mesh(nn.Module):
    """The mesh branch.  `train_path` selects how the SplineConv layers run when autograd records them:
      "dense"    (default) X @ [W_0|...|W_124] into an [M, 125*C] table on the library GEMM, kept for the backward, whose gradient
                 table is filled with atomics (SplineConv.forward's last branch);
      "grouped"  the edge-grouped launches of inference with a gather-form backward (SplineConv.forward_train_grouped): no table, no
                 atomics, the same gradient bits every run.
    "grouped" is taken when ALL of these hold, and the dense path silently otherwise (as the eval predicates do): the module is in
    training mode with grad enabled, on the GPU, `self._pairs` exists (out_channels == 128), the first layer has cin <= 16 and an input
    that does not require grad, every later layer is 128 -> 128, and settings.USE_MFMA_GEMM / USE_GROUPED_SPLINE are on.  torch.cat,
    F.dropout and mesh_final are torch modules on both paths, so both draw the same dropout mask from the same seed."""
    train_path = "dense"

    def __init__(self, cfg, idx, mesh_in_channels=9, out_channels=128, mesh_coord_dim=3, num_mesh_layers=3,
                 cat=True, lin=True, dropout=0.1, model_points=None):
        """cfg keys as the reference (SplineCNN.py:108-110): model_pth, n_mesh_node, model_name.
        `model_points` f32[>=M,9] may be passed instead of reading obj_%06d_fps.npy."""
        super().__init__()
        self.selected_mesh_num = cfg["n_mesh_node"]
        self.name = cfg.get("model_name", "lmo")
        if model_points is None:
            model_points = np.load(os.path.join(cfg["model_pth"], "obj_%06d_fps.npy" % idx))
        model_points = np.asarray(model_points)[: self.selected_mesh_num]
        M = model_points.shape[0]
        x, pos = mesh_node_features(model_points)
        self.register_buffer("xyz", pos)
        self.register_buffer("mesh_graph_x", x)
        self.register_buffer("mesh_graph_edge_index", torch.zeros((2, 4 * M), dtype=torch.int64))
        self.register_buffer("mesh_graph_edge_attr", torch.zeros((4 * M, 3), dtype=torch.float32))
        self.register_buffer("const_one", torch.tensor(1))
        self.graph_ready = False

        self.out_channels = out_channels
        self.cat = cat
        self.dropout = dropout
        self.mesh_convs = nn.ModuleList()
        cin = mesh_in_channels
        for _ in range(num_mesh_layers):
            self.mesh_convs.append(SplineConv(cin, out_channels))
            cin = out_channels
        fin = mesh_in_channels + num_mesh_layers * out_channels if cat else out_channels
        self.mesh_final = nn.Linear(fin, out_channels) if lin else None
        # symmetric objects (SplineCNN.py:155-161): the reference raises NameError there (`misc` is not
        # imported); symmetry correspondences are a "next" row, none for the LineMOD/YCB objects benched.
        self.sys_corr_idx = None
        self._csr = None
        self._pairs = None

    def set_symmetry(self, sys_idx):
        """Symmetric object: sys_idx int[M] = index of each vertex's counterpart under the object's symmetry (the reference's
        `cal_sys_idx`, SplineCNN.py:163-169, registered as buffer `sys_idx` :161).  Switches the training matching loss to
        matching_loss_sys (geoMatch.py:138-141)."""
        idx = torch.as_tensor(sys_idx).long().reshape(-1)
        if idx.shape[0] != self.xyz.shape[0]:
            raise ValueError("sys_idx must have one entry per model vertex (%d), got %d" % (self.xyz.shape[0], idx.shape[0]))
        if "sys_idx" in self._buffers:
            self.sys_idx = idx.to(self.xyz.device)
        else:
            self.register_buffer("sys_idx", idx.to(self.xyz.device))
        self.sys_corr_idx = self.sys_idx

    def unit_normals(self):
        """The model's vertex normals (columns 6..8 of mesh_graph_x) scaled to unit length, f32[M,3]: what point-to-plane ICP
        (pose.refine_icp_plane) pairs with `xyz`.  Computed once per model (a zero normal stays zero)."""
        x = self.mesh_graph_x

        def make():
            n = x[:, 6:9].float()
            return (n / n.norm(dim=1, keepdim=True).clamp_min(1e-20)).contiguous()
        return derived(self, "unit_nrm", (x,), make)

    def set_symmetry_transform(self, R, t_mm):
        """sys_idx from a symmetry transform of the model frame (SplineCNN.py:163-169: `sym_transforms[1]` of
        misc.get_symmetry_transformations, t in mm): for every vertex the nearest vertex of the transformed model, by the HIP kNN."""
        if not self.xyz.is_cuda:
            raise RuntimeError("set_symmetry_transform runs the HIP kNN: move the module to the GPU first")
        Rm = torch.as_tensor(R, dtype=torch.float32, device=self.xyz.device).reshape(3, 3)
        t = torch.as_tensor(t_mm, dtype=torch.float32, device=self.xyz.device).reshape(1, 3) / 1000.0
        moved = (self.xyz @ Rm.t() + t).contiguous()
        self.set_symmetry(ops.knn_batch(moved[None], self.xyz[None].contiguous(), 1)[0, :, 0])

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        ei = state_dict.get(prefix + "mesh_graph_edge_index")
        if ei is not None and bool(torch.as_tensor(ei).any()):
            self.graph_ready = True                                       # a real graph comes with the checkpoint
            self._csr = None
        elif ei is not None:
            # the all-zero placeholder of a state_dict taken before the first GPU forward: keep building the graph here
            state_dict = dict(state_dict)
            state_dict[prefix + "mesh_graph_edge_index"] = self.mesh_graph_edge_index
            if prefix + "mesh_graph_edge_attr" in state_dict:
                state_dict[prefix + "mesh_graph_edge_attr"] = self.mesh_graph_edge_attr
        if prefix + "sys_idx" in state_dict and "sys_idx" not in self._buffers:
            self.set_symmetry(state_dict[prefix + "sys_idx"])
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _ensure_graph(self):
        if not self.graph_ready:
            if not self.xyz.is_cuda:
                raise RuntimeError("SplineCNN_Mesh: the mesh graph is built by the HIP kNN kernel; move the module "
                                   "to the GPU (or load a checkpoint that carries the graph) before calling forward")
            ei, ea = build_mesh_graph(self.xyz, k=4)
            self.mesh_graph_edge_index = ei
            self.mesh_graph_edge_attr = ea
            self.graph_ready = True
            self._csr = None
        if self._csr is None or self._csr[0].device != self.xyz.device:
            ei, ea = self.mesh_graph_edge_index, self.mesh_graph_edge_attr
            M = self.xyz.shape[0]
            order = torch.argsort(ei[1], stable=True)                     # group edges by target
            tgt = ei[1][order]
            rowptr = torch.zeros(M + 1, dtype=torch.int32, device=ei.device)
            rowptr[1:] = torch.cumsum(torch.bincount(tgt, minlength=M), 0).to(torch.int32)
            self._csr = (rowptr.contiguous(), ei[0][order].to(torch.int32).contiguous(), ea[order].contiguous())
            self._pairs = build_spline_pairs(self._csr[1], self._csr[2], M, self.out_channels) if ei.is_cuda and self.out_channels == 128 else None
        return self._csr

    def _channel_major_ok(self):
        convs = list(self.mesh_convs)
        return (settings.USE_POINTWISE and settings.USE_MFMA_GEMM and settings.USE_GROUPED_SPLINE and self.cat and self.mesh_final is not None
                and (not self.training) and not torch.is_grad_enabled() and self.xyz.is_cuda and self._pairs is not None and len(convs) <= 3
                and convs[0].cin <= 16 and convs[0].cout == 128 and all(c.cin % 128 == 0 and c.cout == 128 for c in convs[1:]))

    def _forward_channel_major(self, rowptr, src, attr):
        """Inference: every layer hands its result on channel-major ([1, C, M]), which is what the next layer's grouped GEMM and root
        product read and what the final linear reads as concat-free segments -- no transposing copies, no torch.cat, no library GEMM;
        the result f32[128, M] is the layout GeoMatch.forward returns."""
        x0 = self.mesh_graph_x
        segs = [derived(self, "x0_t", (x0,), lambda: x0.t().contiguous().unsqueeze(0))]       # [1, 9, M], constant per object
        convs = list(self.mesh_convs)
        # each layer's kernel also writes the packed operand of the NEXT layer's grouped GEMM (settings.USE_PACKED_PRODUCERS)
        packed = settings.USE_PACKED_PRODUCERS
        out_t, pk = convs[0].forward_direct_cm_packed(x0, rowptr, src, attr, True, packed and len(convs) > 1)
        segs.append(out_t)
        for li, conv in enumerate(convs[1:]):
            out_t, pk = conv.forward_grouped_cm(segs[-1], rowptr, self._pairs, True, xpk=pk, want_packed=packed and li + 2 < len(convs))
            segs.append(out_t)
        w = self.mesh_final.weight
        out = ops.pointwise(segs, derived(self.mesh_final, "wt", (w,), lambda: w.t().contiguous()), None, self.mesh_final.bias)     # [1, 128, M]; eval: dropout is the identity
        return out[0]

    def _train_grouped_ok(self):
        convs = list(self.mesh_convs)
        if (self.train_path == "grouped" and self.training and torch.is_grad_enabled() and self._pairs is not None
                and "inv_deg" not in self._pairs):
            # the inverse maps of the backward: built the first time the path is asked for, never for inference or the dense path
            self._pairs = build_spline_pairs(self._csr[1], self._csr[2], self.xyz.shape[0], self.out_channels, rowptr=self._csr[0])
        return (self.train_path == "grouped" and self.training and torch.is_grad_enabled() and self.xyz.is_cuda and self._pairs is not None
                and settings.USE_MFMA_GEMM and settings.USE_GROUPED_SPLINE and len(convs) >= 1
                and convs[0].cin <= 16 and not self.mesh_graph_x.requires_grad and convs[0].train_grouped_ok(self.mesh_graph_x, self._pairs)
                and all(c.cin == 128 and c.cout == 128 and c.lin.bias is None for c in convs[1:]))

    def forward(self):
        if self.train_path not in ("dense", "grouped"):
            raise ValueError("train_path must be 'dense' or 'grouped', got %r" % (self.train_path,))
        rowptr, src, attr = self._ensure_graph()
        if self._channel_major_ok():
            return self._forward_channel_major(rowptr, src, attr)
        grouped = self._train_grouped_ok()
        feats = [self.mesh_graph_x]
        for conv in self.mesh_convs:
            if grouped:
                feats.append(conv.forward_train_grouped(feats[-1], rowptr, src, attr, True, self._pairs))
                continue
            feats.append(conv(feats[-1], rowptr, src, attr, relu=True, pairs=self._pairs))   # F.relu(conv(...)) (SplineCNN.py:238-239)
        out = torch.cat(feats, dim=-1) if self.cat else feats[-1]
        out = F.dropout(out, p=self.dropout, training=self.training)
        if self.mesh_final is not None:
            out = self.mesh_final(out)
        return out.transpose(0, 1)
