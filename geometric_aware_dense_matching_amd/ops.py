"""Torch-facing operators over the C ABI of libgdm_hip.so.

PyTorch is plumbing here: it owns device memory and the current HIP stream; every operator
passes raw device pointers + that stream to the hand-written HIP kernels.  There is no CPU
path: CPU tensors raise.  Index tensors are int32 on the device (the reference widens them to
int64 only because torch.gather demands it: /root/reference/train_lm.py:167-168); int64 is
accepted and narrowed.

Operator <-> reference map (file:line under /root/reference):
  knn_batch / knn_jobs   models/RandLA/utils/nearest_neighbors/knn.pyx:71-109, knn_.cxx:104-135
  group_gather           models/RandLA/RandLANet.py:729-738 (+ permute :704-716); pointops.py:151-176
  gather_max             models/ffb6d.py:128-146 random_sample
  gather_nn              models/ffb6d.py:148-163 nearest_interpolation; pointops.py:61-82
  rel_pos_enc            models/RandLA/RandLANet.py:720-727
  att_pool               models/RandLA/RandLANet.py:749-752
  match / seg_mask       evaluator.py:79-93
  ballquery / furthestsampling   lib/pointops/functions/pointops.py:205-219, 40-50
  surface_sample / furthestsampling_wide / point_diameter   the producer of obj_%06d_fps.npy, which the reference names
                         (ref/ycbv.py:106) and does not ship: model_prep.py, DESIGN.md 6n
  texture_mips / render_frames(textures=...) / surface_sample_tex   no counterpart in the reference: texture maps by the written
                         rule of include/gdm.h (texture.py)
"""
import collections
import ctypes
import functools
import os

import torch

from . import _lib, settings
from ._lib import KnnJob, call, check  # noqa: F401  (tests and tools reach check as ops.check)
from .derived import derived

MATCH_BF16X3 = _lib.GDM_MATCH_BF16X3
MATCH_F32 = _lib.GDM_MATCH_F32


def _stream():
    return torch.cuda.current_stream().cuda_stream


_side_streams = {}


def side_stream(device, which=0):
    """A per-device side stream (HIP streams let independent branches of the step overlap: most of its ~120 kernels are far too
    small to fill 256 CUs).  Callers fork with side.wait_stream(current), join with current.wait_stream(side)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), which)
    st = _side_streams.get(key)
    if st is None:
        st = torch.cuda.Stream(device=device)
        _side_streams[key] = st
    return st


def _stream_lane(device):
    """Which ROLE the current stream plays for the scratch-buffer pools: ("side", k) for side stream k of the device, "main" for any
    other stream.  The pools are keyed by role, not by stream handle: a hipGraph capture runs on a stream of its own (torch's capture
    stream), and a pool keyed by handle missed every buffer the eager warm-up had made -- the capture then allocated and ZERO-FILLED
    them again inside the graph (12 fill kernels, 0.13-0.15 ms of every replay).  A BufferPool serves ONE step at a time."""
    h = torch.cuda.current_stream(device).cuda_stream
    idx = device.index if device.index is not None else torch.cuda.current_device()
    for (d, which), st in _side_streams.items():
        if d == idx and st.cuda_stream == h:
            return ("side", which)
    # The process-wide default pool has no owner that could promise "one step at a time": two eager callers on different user
    # streams must not share a zero-bordered operand buffer or a matching workspace, so there the handle is part of the key.
    if _pool is _default_pool:
        return ("main", h)
    return "main"


class fork:
    """with ops.fork(device, which) as f: ...   -- the body is enqueued on side stream `which`, which first waits for everything
    already on the current stream (and for the `after` events, if given); `f.join(*tensors)` afterwards makes the current stream
    wait for the side stream and hands the tensors made there over to it.  Works eagerly and inside hipGraph capture.

    Lifetime rule (explicit, no argument by allocator behaviour): every tensor that crosses a stream is `record_stream`ed on the
    stream that did not allocate it -- `f.use(t)` for a tensor of the current stream that the body reads, `f.join(t, ...)` for
    the tensors the body made -- so the caching allocator never hands its block out again before both streams are done with it."""

    def __init__(self, device, which=0, after=(), start=None):
        self.side = side_stream(device, which)
        self.cur = torch.cuda.current_stream(device)
        self.after = tuple(after) if isinstance(after, (tuple, list)) else (after,)
        self.start = start          # an event of the current stream: the body waits for IT instead of for everything enqueued so far
        self._ctx = None

    def __enter__(self):
        if self.start is not None:
            self.side.wait_event(self.start)
        else:
            self.side.wait_stream(self.cur)
        for ev in self.after:
            if ev is not None:
                self.side.wait_event(ev)           # waiting for an event of the same stream is free
        self._ctx = torch.cuda.stream(self.side)
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        self._ctx.__exit__(*exc)
        return False

    def use(self, *tensors):
        """Tensors allocated on the current stream that the forked body reads."""
        for t in tensors:
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(self.side)

    def join(self, *tensors):
        """The current stream waits for the side stream; `tensors` (made on the side stream) may be used on it from here on."""
        self.cur.wait_stream(self.side)
        for t in tensors:
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(self.cur)


def _dev(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA (HIP) tensor: the geoMatch ops have no CPU fallback" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _idx32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA (HIP) tensor: the geoMatch ops have no CPU fallback" % name)
    if t.dtype == torch.int64:
        t = t.to(torch.int32)
    elif t.dtype != torch.int32:
        raise TypeError("%s must be int32 or int64, got %s" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


# --------------------------------------------------------------------------------------
# neighbour search
# --------------------------------------------------------------------------------------
def knn_batch(support, query, K, return_d2=False):
    """support f32[B,S,3], query f32[B,Q,3] -> idx i32[B,Q,K] (ascending d2, ties by index)."""
    support = _dev(support, torch.float32, "support")
    query = _dev(query, torch.float32, "query")
    B, S, _ = support.shape
    Q = query.shape[1]
    assert support.shape[2] == 3 and query.shape[2] == 3 and query.shape[0] == B
    idx = torch.empty((B, Q, K), dtype=torch.int32, device=support.device)
    d2 = torch.empty((B, Q, K), dtype=torch.float32, device=support.device) if return_d2 else None
    call("gdm_knn_batch_hip", support, query, B, S, Q, K, idx, d2)
    return (idx, d2) if return_d2 else idx


def knn_jobs(jobs, B, keep_workspace=None):
    """jobs: list of (support f32 view [B,S,3], query f32 view [B,Q,3], K[, grid_w]).  Views may be prefix
    slices along dim 1 of contiguous [B,N,3] arrays (batch stride kept).  grid_w > 0 declares the support an organised map of
    S / grid_w rows x grid_w columns (row-major pixels of a depth crop): K > 1 searches then scan only the window of pixel
    columns / rows that can hold a neighbour (same results).  One launch per K class.  Returns the idx tensors i32[B,Q,K]."""
    n = len(jobs)
    arr = (KnnJob * n)()
    # ONE allocation for all index arrays (22 per pyramid): the host time of this function sits on the step's critical path (the
    # searches are its first kernels), and 22 allocator calls were a third of it
    sizes = []
    for job in jobs:
        sup, qry, K = job[:3]
        for t, nm in ((sup, "support"), (qry, "query")):
            if not t.is_cuda or t.dtype != torch.float32:
                raise RuntimeError("knn_jobs: %s must be a CUDA float32 tensor" % nm)
            if t.dim() != 3 or t.shape[0] != B or t.shape[2] != 3 or t.stride(2) != 1 or t.stride(1) != 3:
                raise ValueError("knn_jobs: %s must be [B,n,3] with unit point stride, got %s strides %s" %
                                 (nm, tuple(t.shape), t.stride()))
        sizes.append(B * qry.shape[1] * K)
    starts = []
    tot = 0
    for sz in sizes:                                          # every array starts on a 256-byte boundary (its readers use 16-byte loads)
        starts.append(tot)
        tot += (sz + 63) // 64 * 64
    slab = torch.empty(tot, dtype=torch.int32, device=jobs[0][0].device)
    base = slab.data_ptr()
    outs = []
    for i, job in enumerate(jobs):
        off = starts[i]
        sup, qry, K = job[:3]
        grid_w = int(job[3]) if len(job) > 3 else 0
        S, Q = sup.shape[1], qry.shape[1]
        a = arr[i]
        a.support = sup.data_ptr()
        a.query = qry.data_ptr()
        a.idx = base + 4 * off
        a.d2 = None
        a.support_bstride = sup.stride(0) if B > 1 else S * 3
        a.query_bstride = qry.stride(0) if B > 1 else Q * 3
        a.S, a.Q, a.K = S, Q, K
        a.grid_w = grid_w if (grid_w > 0 and S % grid_w == 0) else 0
        outs.append(slab[off:off + sizes[i]].view(B, Q, K))
    ws = _knn_launch(arr, n, B, jobs[0][0].device)
    if keep_workspace is not None:
        keep_workspace.append(ws)        # the caller keeps it alive as long as the results (explicit lifetime across streams)
    return outs


def copy_views(views):
    """Dense copies of a list of strided views in ONE launch (include/gdm.h gdm_copy_jobs_hip): every view is a 3-D or 4-D tensor
    of 4-byte elements whose last dimension is contiguous.  Returns the dense tensors (same shapes)."""
    n = len(views)
    arr = (_lib.CopyJob * n)()
    outs = []
    for i, v in enumerate(views):
        if not v.is_cuda or v.element_size() != 4 or v.dim() not in (3, 4) or v.stride(-1) != 1:
            raise ValueError("copy_views: view %d must be a 3-D / 4-D CUDA tensor of 4-byte elements with a contiguous last dimension" % i)
        out = torch.empty(v.shape, dtype=v.dtype, device=v.device)
        v4 = v if v.dim() == 4 else v.unsqueeze(1)
        arr[i] = _lib.CopyJob(out.data_ptr(), v.data_ptr(), v4.stride(0), v4.stride(1), v4.stride(2),
                              v4.shape[0], v4.shape[1], v4.shape[2], v4.shape[3])
        outs.append(out)
    call("gdm_copy_jobs_hip", arr, n)
    return outs


def _knn_launch(arr, n, B, device):
    """gdm_knn_jobs_ws_hip with a workspace from torch's caching allocator (graph-capture safe): every distinct support set of the
    K > 1 jobs is re-laid out once per launch -- ratio ranges for an organised map, a cell list from 1024 points, hashed float4 tiles
    otherwise (include/gdm.h, gdm_knn_jobs_workspace_bytes)."""
    L = _lib.lib()
    nbytes = int(L.gdm_knn_jobs_workspace_bytes(arr, n, B))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    call("gdm_knn_jobs_ws_hip", arr, n, B, ws, nbytes)
    return ws


def ballquery(radius, nsample, xyz, new_xyz):
    """pointops.BallQuery.forward argument order (pointops.py:205): -> i32[B,m,nsample]."""
    xyz = _dev(xyz, torch.float32, "xyz")
    new_xyz = _dev(new_xyz, torch.float32, "new_xyz")
    B, n, _ = xyz.shape
    m = new_xyz.shape[1]
    idx = torch.zeros((B, m, nsample), dtype=torch.int32, device=xyz.device)
    call("gdm_ballquery_hip", B, n, m, float(radius), nsample, new_xyz, xyz, idx)
    return idx


def furthestsampling(xyz, m):
    """pointops.FurthestSampling.forward (pointops.py:40-50): xyz f32[B,n,3] -> i32[B,m]."""
    xyz = _dev(xyz, torch.float32, "xyz")
    B, n, _ = xyz.shape
    idx = torch.empty((B, m), dtype=torch.int32, device=xyz.device)
    temp = torch.empty((B, n), dtype=torch.float32, device=xyz.device)
    call("gdm_furthestsampling_hip", B, n, m, xyz, temp, idx)
    return idx


def furthestsampling_wide(xyz, m, groups=0):
    """furthestsampling for many candidates: the same idx i32[B,m], bit for bit, from m small launches that spread the candidates
    over the whole device (include/gdm.h gdm_fps_wide_hip).  groups: workgroups per cloud, 1..1024, or 0 = the launcher's choice."""
    xyz = _dev(xyz, torch.float32, "xyz")
    B, n, _ = xyz.shape
    g = int(groups) or int(call("gdm_fps_wide_groups", n))
    idx = torch.empty((B, m), dtype=torch.int32, device=xyz.device)
    dist = torch.empty((B, n), dtype=torch.float32, device=xyz.device)
    partial = torch.empty((B, 2, max(g, 1)), dtype=torch.int64, device=xyz.device)
    call("gdm_fps_wide_hip", B, n, m, int(groups), xyz, dist, partial, idx)
    return idx


def surface_sample(verts, faces, vnrm, vrgb, cdf, S, seed=0):
    """S points on a triangle mesh by the sample rule of include/gdm.h (gdm_surface_sample_hip): verts, vnrm f32[V,3], vrgb u8 or
    f32[V,3] (integer levels), faces i32[F,3], cdf i64[F] = inclusive cumulative integer face weights -> f32[S,9] = xyz, rgb, normal.
    What the device cannot see is refused here: a face index outside [0, V) and a cdf that ends in 0 or decreases."""
    return _surface_sample(verts, faces, vnrm, vrgb, cdf, S, seed, None)


def _surface_sample(verts, faces, vnrm, vrgb, cdf, S, seed, textured):
    """surface_sample and surface_sample_tex: the checks they share, then the entry; `textured` is None or the textured entry's extra
    arguments in its order."""
    verts = _dev(verts, torch.float32, "verts")
    vnrm = _dev(vnrm, torch.float32, "vnrm")
    if isinstance(vrgb, torch.Tensor) and vrgb.dtype == torch.uint8:
        vrgb = vrgb.float()
    vrgb = _dev(vrgb, torch.float32, "vrgb")
    faces = _dev(faces, torch.int32, "faces")
    cdf = _dev(cdf, torch.int64, "cdf")
    V, F, S = verts.shape[0], faces.shape[0], int(S)
    if verts.shape != (V, 3) or vnrm.shape != (V, 3) or vrgb.shape != (V, 3) or faces.shape != (F, 3) or cdf.shape != (F,):
        raise ValueError("surface_sample: verts / vnrm / vrgb must be [V,3], faces [F,3] and cdf [F]")
    if V >= 1 and F >= 1:
        lo, hi, last, step = (int(v) for v in torch.stack([faces.min().long(), faces.max().long(), cdf[-1],
                                                           (cdf - torch.cat([cdf.new_zeros(1), cdf[:-1]])).min()]).tolist())
        if lo < 0 or hi >= V:
            raise ValueError("surface_sample: face indices %d..%d outside the %d vertices" % (lo, hi, V))
        if last <= 0 or step < 0:
            raise ValueError("surface_sample: cdf must be a cumulative sum of non-negative weights that ends above 0 (cdf[F-1]=%d)" % last)
    if not 1 <= S < 1 << 31:
        raise ValueError("surface_sample: S=%d not in [1, 2^31)" % S)
    out = torch.empty((S, 9), dtype=torch.float32, device=verts.device)
    if textured is None:
        call("gdm_surface_sample_hip", verts, faces, vnrm, vrgb, cdf, V, F, S, int(seed) & 0xffffffff, out)
    else:
        call("gdm_surface_sample_tex_hip", verts, faces, vnrm, vrgb, cdf, *textured, V, F, S, int(seed) & 0xffffffff, out)
    return out


def surface_sample_tex(verts, faces, vnrm, vrgb, cdf, fuv, tex, row, S, seed=0, flip_v=True):
    """surface_sample for a textured mesh (gdm_surface_sample_tex_hip): fuv f32[F,3,2], tex u8[T,4] on the device, row = the object's
    (offset, W0, H0, L) as host integers.  The same draws, xyz and normals; rgb is the texture's level 0 at the interpolated (u, v)."""
    fuv = _dev(fuv, torch.float32, "fuv")
    tex = _dev(tex, torch.uint8, "tex")
    F = faces.shape[0]
    if tuple(fuv.shape) != (F, 3, 2):
        raise ValueError("surface_sample_tex: fuv must be [F=%d,3,2], got %s" % (F, tuple(fuv.shape)))
    if tex.dim() != 2 or tex.shape[1] != 4 or not 1 <= tex.shape[0] < 1 << 31:
        raise ValueError("surface_sample_tex: tex must be u8[T,4] with 1 <= T < 2^31, got %s" % (tuple(tex.shape),))
    off, W0, H0, L = (int(v) for v in row)
    return _surface_sample(verts, faces, vnrm, vrgb, cdf, S, seed, (fuv, tex, off, W0, H0, L, tex.shape[0], int(bool(flip_v))))


def point_diameter(xyz):
    """The exact farthest pair of xyz f32[V,3] (include/gdm.h gdm_point_diameter_hip): (pair i32[2] with i < j, d2 f32[1]), the
    lowest i and then the lowest j among equal fp32 squared distances."""
    xyz = _dev(xyz, torch.float32, "xyz")
    V = xyz.shape[0]
    nbytes = int(call("gdm_point_diameter_workspace_bytes", V))
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=xyz.device)
    pair = torch.empty(2, dtype=torch.int32, device=xyz.device)
    d2 = torch.empty(1, dtype=torch.float32, device=xyz.device)
    call("gdm_point_diameter_hip", xyz, V, ws, nbytes, pair, d2)
    return pair, d2


# --------------------------------------------------------------------------------------
# gather / pool, with backward
# --------------------------------------------------------------------------------------
def _feat3(feat):
    if feat.dim() == 4:
        assert feat.shape[3] == 1
        feat = feat.squeeze(3)
    return feat


class _GroupGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, idx):
        feat = _dev(feat, torch.float32, "feat")
        B, C, n = feat.shape
        m, K = idx.shape[1], idx.shape[2]
        out = torch.empty((B, C, m, K), dtype=torch.float32, device=feat.device)
        call("gdm_group_gather_hip", feat, idx, B, C, n, m, K, out)
        ctx.save_for_backward(idx)
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, go):
        (idx,) = ctx.saved_tensors
        B, C, m, K = go.shape
        # a channel slice of a concatenation's gradient (dense rows, a larger batch stride) is read where it lies
        if not (go.dtype == torch.float32 and go.stride(3) == 1 and go.stride(2) == K and go.stride(1) == m * K and go.stride(0) >= C * m * K):
            go = go.contiguous()
        g = torch.zeros((B, C, ctx.n), dtype=torch.float32, device=go.device)
        call("gdm_group_gather_bwd2_hip", go, go.stride(0), idx, B, C, ctx.n, m, K, g)
        return g, None


def group_gather(feat, idx):
    """feat f32[B,C,n(,1)], idx int[B,m,K] -> f32[B,C,m,K]."""
    idx = _idx32(idx, "idx")
    assert idx.dim() == 3
    return _GroupGather.apply(_feat3(feat), idx)


def gather_nn(feat, idx):
    """feat f32[B,C,n(,1)], idx int[B,m] or [B,m,1] -> f32[B,C,m]."""
    idx = _idx32(idx, "idx")
    if idx.dim() == 2:
        idx = idx.unsqueeze(2)
    assert idx.shape[2] == 1
    return _GroupGather.apply(_feat3(feat), idx).squeeze(3)


class _GatherMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, idx):
        feat = _dev(feat, torch.float32, "feat")
        B, C, n = feat.shape
        m, K = idx.shape[1], idx.shape[2]
        out = torch.empty((B, C, m), dtype=torch.float32, device=feat.device)
        need_arg = ctx.needs_input_grad[0]               # (not feat.requires_grad: _dev may have made a contiguous copy under no_grad)
        arg = torch.empty((B, C, m), dtype=torch.int32, device=feat.device) if need_arg else None
        call("gdm_gather_max_hip", feat, idx, B, C, n, m, K, out, arg)
        if need_arg:
            ctx.save_for_backward(arg)
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, go):
        (arg,) = ctx.saved_tensors
        go = go.contiguous()
        B, C, m = go.shape
        g = torch.zeros((B, C, ctx.n), dtype=torch.float32, device=go.device)
        call("gdm_gather_max_bwd_hip", go, arg, B, C, ctx.n, m, g)
        return g, None


def gather_max(feat, idx):
    """feat f32[B,C,n(,1)], idx int[B,m,K] -> f32[B,C,m] = max over the K gathered neighbours."""
    idx = _idx32(idx, "idx")
    assert idx.dim() == 3
    return _GatherMax.apply(_feat3(feat), idx)


def rel_pos_enc(xyz, idx):
    """xyz f32[B,n,3], idx int[B,n,K] -> f32[B,10,n,K] (inputs are data: no gradient)."""
    xyz = _dev(xyz, torch.float32, "xyz")
    idx = _idx32(idx, "idx")
    B, n, _ = xyz.shape
    K = idx.shape[2]
    assert idx.shape[0] == B and idx.shape[1] == n
    out = torch.empty((B, 10, n, K), dtype=torch.float32, device=xyz.device)
    call("gdm_rel_pos_enc_hip", xyz, idx, B, n, K, out)
    return out


class _AttPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, att, feat):
        att = _dev(att, torch.float32, "att")
        feat = _dev(feat, torch.float32, "feat")
        B, C, n, K = att.shape
        assert feat.shape == att.shape
        out = torch.empty((B, C, n), dtype=torch.float32, device=att.device)
        call("gdm_att_pool_hip", att, feat, B, C, n, K, out)
        ctx.save_for_backward(att, feat)
        return out

    @staticmethod
    def backward(ctx, go):
        att, feat = ctx.saved_tensors
        go = go.contiguous()
        B, C, n, K = att.shape
        ga = torch.empty_like(att)
        gf = torch.empty_like(feat)
        call("gdm_att_pool_bwd_hip", att, feat, go, B, C, n, K, ga, gf)
        return ga, gf


def att_pool(att, feat):
    """att, feat f32[B,C,n,K] -> f32[B,C,n]: sum_k softmax_k(att) * feat."""
    return _AttPool.apply(att, feat)


def topk_rows(score, k, return_values=False):
    """score f32[..., n] -> idx i32[..., k] of the k largest per row (ties: lower column first)
    (dgcnn.py:26 `pairwise_distance.topk(k=k, dim=-1)[1]`)."""
    score = _dev(score, torch.float32, "score")
    n = score.shape[-1]
    rows = score.numel() // n
    idx = torch.empty(score.shape[:-1] + (k,), dtype=torch.int32, device=score.device)
    val = torch.empty(score.shape[:-1] + (k,), dtype=torch.float32, device=score.device) if return_values else None
    call("gdm_topk_rows_hip", score, rows, n, k, idx, val)
    return (idx, val) if return_values else idx


def topk_negdist(gram, xx, k):
    """Indices of dgcnn.py:22-26 (`pairwise_distance.topk(k)`), from gram f32[B,n,n] = x^T x and xx f32[B,n] = sum_c x^2, without
    materialising pairwise_distance (same fp32 operations in the same order: identical indices)."""
    gram = _dev(gram, torch.float32, "gram")
    xx = _dev(xx, torch.float32, "xx")
    B, n, _ = gram.shape
    idx = torch.empty((B, n, k), dtype=torch.int32, device=gram.device)
    call("gdm_topk_negdist_hip", gram, xx, B, n, k, idx)
    return idx


def feature_knn(x, k, return_values=False, splits=0):
    """x f32[B,C,n] channel-major -> idx i32[B,n,k] (and val f32[B,n,k]) of the k largest dgcnn.py:22-25 scores per row, Gram tile and
    selection in one kernel (include/gdm.h gdm_feature_knn_hip): no [B,n,n] matrix, the only workspace is O(B n).  Score
    descending, ties by ascending column, short rows filled with index 0.  A channel slice `t[:, :c]` of a contiguous tensor is read
    in place (its batch stride is passed on).  splits (1, 2, 4; 0 = chosen from the shape): how many waves share a row group's columns --
    a launch parameter only, the result does not depend on it.  No gradient flows through indices (both the inference and the training
    path of the variant build their graphs here)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("x must be a CUDA (HIP) tensor: the geoMatch ops have no CPU fallback")
    if x.dtype != torch.float32 or x.dim() != 3:
        raise TypeError("x must be f32[B,C,n], got %s %s" % (x.dtype, tuple(x.shape)))
    B, C, n = x.shape
    if not 1 <= k <= 32:
        raise ValueError("feature_knn: k=%d not in [1, 32]" % k)
    if x.stride(2) != 1 or x.stride(1) != n or (B > 1 and x.stride(0) < C * n):
        x = x.contiguous()
    bstride = x.stride(0) if B > 1 else C * n
    nbytes = _lib.lib().gdm_feature_knn_workspace_bytes(B, n)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)          # xx f32[B,n] + one flag per 32 rows
    idx = torch.empty((B, n, k), dtype=torch.int32, device=x.device)
    val = torch.empty((B, n, k), dtype=torch.float32, device=x.device) if return_values else None
    call("gdm_feature_knn_hip", x, bstride, B, C, n, k, int(splits), ws, nbytes, idx, val)
    return (idx, val) if return_values else idx


def edge_block(pq, idx, scale1, shift1, w2=None, scale2=None, shift2=None, slope=0.2, out=None, out_c0=0):
    """One edge-convolution stage without the edge tensor (include/gdm.h gdm_edge_block_hip), on folded (eval) BatchNorm: no autograd.
    Training goes through `edge_block_train`, which runs this kernel on the batch statistics and has a backward.
    pq f32[B,n,128] point-major: the stage's first convolution applied per point, [W_a ; W_b - W_a] x; idx int[B,n,K], K <= 32;
    scale1 / shift1 f32[64]: the first folded BatchNorm; w2 f32[64,64(,1,1)], scale2 / shift2: the second convolution and its
    BatchNorm, or None for a single-convolution stage.  Returns f32[B,64,n] = max over the neighbours of the last activation, or
    writes channels [out_c0, out_c0 + 64) of `out` f32[B,outC,n] and returns it."""
    pq = _dev(pq, torch.float32, "pq")
    idx = _idx32(idx, "idx")
    B, n, c2 = pq.shape
    if c2 != 128 or idx.dim() != 3 or tuple(idx.shape[:2]) != (B, n):
        raise ValueError("edge_block: pq must be [B,n,128] and idx [B,n,K], got %s and %s" % (tuple(pq.shape), tuple(idx.shape)))
    K = idx.shape[2]
    scale1, shift1 = _dev(scale1, torch.float32, "scale1"), _dev(shift1, torch.float32, "shift1")
    if (w2 is None) != (scale2 is None) or (w2 is None) != (shift2 is None):
        raise ValueError("edge_block: w2, scale2 and shift2 go together")
    if w2 is not None:
        w2, scale2, shift2 = _dev(w2, torch.float32, "w2"), _dev(scale2, torch.float32, "scale2"), _dev(shift2, torch.float32, "shift2")
        if w2.numel() != 64 * 64 or scale2.numel() != 64 or shift2.numel() != 64:
            raise ValueError("edge_block: the second convolution is 64 -> 64")
    if scale1.numel() != 64 or shift1.numel() != 64:
        raise ValueError("edge_block: scale1 / shift1 must hold 64 channels")
    if out is None:
        out = torch.empty((B, 64, n), dtype=torch.float32, device=pq.device)
    elif (not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 3 or out.shape[0] != B
          or out.shape[2] != n):
        raise ValueError("edge_block: out must be a contiguous f32 [B,outC,%d] tensor" % n)
    call("gdm_edge_block_hip", pq, idx, scale1, shift1, w2, scale2, shift2, float(slope), B, n, K, out, out.shape[1], int(out_c0))
    return out


def _edge_sums_buffer(B, n, K, device):
    """f64[groups * 128 + 2] in the layout `_fold_and_all_reduce` reads: one (sum, sum) pair per workgroup and channel, then the local
    edge count and the number of workgroups."""
    groups = _lib.lib().gdm_edge_train_groups(B, n)
    buf = torch.empty(groups * 128 + 2, dtype=torch.float64, device=device)
    buf[-2:] = float(B * n * K)                               # only the count is read
    return buf


def _edge_fold(buf, group):
    """-> (local sums f64[64,2], sums over the ranks of `group` f64[64,2], edge count over the ranks: a number, or a 0-dim tensor when
    it came through the all-reduce -- no host synchronisation either way).  Workgroup partials are added in fp64 in a fixed order."""
    local = buf[:-2].view(-1, 128).sum(0).view(64, 2)
    if group is None:
        return local, local, None
    compact = _fold_and_all_reduce(buf, 64, group)
    return local, compact[:128].view(64, 2), compact[128]


def _edge_bn_fold(sums, E, bn_w, bn_b, eps, momentum, running_mean, running_var):
    """Batch moments from (sum y, sum y^2) over E edges in fp64 -> st f32[4,64] = (gamma rstd | beta - mean gamma rstd | mean | rstd);
    updates the running statistics as the module does (unbiased variance)."""
    mean = sums[:, 0] / E
    var = (sums[:, 1] / E - mean * mean).clamp_min(0.0)
    rstd = torch.rsqrt(var + eps)
    sc = bn_w.detach().double() * rstd
    st = torch.stack((sc, bn_b.detach().double() - mean * sc, mean, rstd)).float()
    if running_mean is not None:
        running_mean.copy_((1.0 - momentum) * running_mean.double() + momentum * mean)
        running_var.copy_((1.0 - momentum) * running_var.double() + momentum * (var * (E / (E - 1.0))))
    return st


class _EdgeBlockTrain(torch.autograd.Function):
    """ops.edge_block_train: forward = two statistics passes + the inference kernel on the folded batch statistics; backward = arg-max /
    last sums, (dW2 and the first layer's sums,) scatter -- every pass recomputes its edges (include/gdm.h gdm_edge_stats_hip ...)."""

    @staticmethod
    def forward(ctx, pq, idx, w1, b1, w2, g2, b2, slope, bn1_args, bn2_args, group):
        B, n, _ = pq.shape
        K = idx.shape[2]
        two = w2 is not None
        count = float(B * n * K)
        buf = _edge_sums_buffer(B, n, K, pq.device)
        call("gdm_edge_stats_hip", pq, idx, None, None, float(slope), B, n, K, buf)
        _, tot, E = _edge_fold(buf, group)
        E = count if E is None else E
        st1 = _edge_bn_fold(tot, E, w1, b1, *bn1_args)
        st2 = None
        if two:
            ctx.w2_shape = w2.shape
            w2 = _dev(w2.detach().reshape(64, 64), torch.float32, "w2")
            call("gdm_edge_stats_hip", pq, idx, st1, w2, float(slope), B, n, K, buf)
            _, tot, _ = _edge_fold(buf, group)
            st2 = _edge_bn_fold(tot, E, g2, b2, *bn2_args)
        out = edge_block(pq, idx, st1[0], st1[1], w2, st2[0] if two else None, st2[1] if two else None, slope)
        ctx.save_for_backward(pq, idx, st1, w2, st2, E if torch.is_tensor(E) else None)
        ctx.count, ctx.slope, ctx.group = count, float(slope), group
        return out

    @staticmethod
    def backward(ctx, go):
        pq, idx, st1, w2, st2, E = ctx.saved_tensors
        E = ctx.count if E is None else E
        go = _dev(go, torch.float32, "grad")
        B, n, _ = pq.shape
        K = idx.shape[2]
        two = w2 is not None
        slope, group = ctx.slope, ctx.group
        amax = torch.empty((B, n, 64), dtype=torch.uint8, device=pq.device)
        buf = _edge_sums_buffer(B, n, K, pq.device)
        call("gdm_edge_bwd_reduce_hip", pq, idx, st1, w2, st2, slope, B, n, K, go, amax, buf)
        # grad gamma / beta (and dW2) stay LOCAL sums, as in _BatchNormAct: DDP averages parameter gradients over the ranks
        local, tot, _ = _edge_fold(buf, group)
        cf_last = (tot / E).t().contiguous().float()                        # [2,64] = dbeta / E | dgamma / E
        gw2 = gg2 = gb2 = cf2 = None
        if two:
            gb2, gg2, cf2 = local[:, 0].float(), local[:, 1].float(), cf_last
            slabs = torch.empty((buf.numel() - 2) // 128, 64, 64, dtype=torch.float32, device=pq.device)
            call("gdm_edge_bwd_mid_hip", pq, idx, st1, w2, st2, cf2, slope, B, n, K, go, amax, buf, slabs)
            gw2 = slabs.sum(0).reshape(ctx.w2_shape)
            local, tot, _ = _edge_fold(buf, group)
            cf1 = (tot / E).t().contiguous().float()
        else:
            cf1 = cf_last
        gb1, gg1 = local[:, 0].float(), local[:, 1].float()
        gpq = torch.zeros_like(pq)                                          # the P half is accumulated by atomicAdd
        call("gdm_edge_bwd_scatter_hip", pq, idx, st1, cf1, w2, st2, cf2, slope, B, n, K, go, amax, gpq)
        return gpq, None, gg1, gb1, gw2, gg2, gb2, None, None, None, None


def _edge_bn_check(bn, name):
    if not (bn.training and bn.affine and bn.momentum is not None and bn.weight.numel() == 64):
        raise ValueError("edge_block_train: %s must be an affine 64-channel BatchNorm in training mode with a numeric momentum" % name)
    return (float(bn.eps), float(bn.momentum), bn.running_mean if bn.track_running_stats else None,
            bn.running_var if bn.track_running_stats else None)


def edge_block_train(pq, idx, bn1, w2=None, bn2=None, slope=0.2):
    """`edge_block` in training mode, differentiable: one edge-convolution stage with train-mode BatchNorm over all B n K edges (over all
    ranks for a SyncBatchNorm that spans several) and no [B,C,n,K] tensor, forward or backward.
    pq f32[B,n,128] point-major (the stage's first convolution per point, as for edge_block); idx int[B,n,K], clamped to [0, n);
    bn1: the first BatchNorm MODULE (weight, bias, eps and momentum are read at call time, running statistics and
    num_batches_tracked are updated as the module does); w2 f32[64,64(,1,1)] and bn2: the second convolution and its BatchNorm, or
    None.  Returns f32[B,64,n].  Gradients reach pq, bn1.weight / bias, w2 and bn2.weight / bias; none flows through idx.
    grad pq's neighbour half is accumulated by float atomics: it is not bitwise reproducible from run to run."""
    pq = _dev(pq, torch.float32, "pq")
    idx = _idx32(idx, "idx")
    if pq.dim() != 3 or pq.shape[2] != 128 or idx.dim() != 3 or tuple(idx.shape[:2]) != tuple(pq.shape[:2]):
        raise ValueError("edge_block_train: pq must be [B,n,128] and idx [B,n,K], got %s and %s" % (tuple(pq.shape), tuple(idx.shape)))
    if not 1 <= idx.shape[2] <= 32:
        raise ValueError("edge_block_train: K=%d not in [1, 32]" % idx.shape[2])
    if (w2 is None) != (bn2 is None):
        raise ValueError("edge_block_train: w2 and bn2 go together")
    if w2 is not None and w2.numel() != 64 * 64:
        raise ValueError("edge_block_train: the second convolution is 64 -> 64")
    a1 = _edge_bn_check(bn1, "bn1")
    a2 = _edge_bn_check(bn2, "bn2") if bn2 is not None else None
    out = _EdgeBlockTrain.apply(pq, idx, bn1.weight, bn1.bias, w2, bn2.weight if bn2 is not None else None,
                                bn2.bias if bn2 is not None else None, float(slope), a1, a2, _sync_group(bn1))
    for bn in (bn1, bn2):
        if bn is not None and bn.num_batches_tracked is not None:
            if _bn_counters is not None:
                _bn_counters.append(bn.num_batches_tracked)
            else:
                bn.num_batches_tracked.add_(1)
    return out


def affine_act_maxk(x, scale, shift, act=0, slope=0.0):
    """max over the last (neighbour) dimension of act(scale[c]*x + shift[c]); x f32[B,C,n,K] -> f32[B,C,n].  Inference only."""
    x = _dev(x, torch.float32, "x")
    B, C, n, K = x.shape
    out = torch.empty((B, C, n), dtype=torch.float32, device=x.device)
    call("gdm_affine_act_maxk_hip", x, scale, shift, B * C, C, n, K, act, float(slope), out)
    return out


class _EdgeFeature(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx):
        x = _dev(x, torch.float32, "x")
        B, C, n = x.shape
        K = idx.shape[2]
        out = torch.empty((B, 2 * C, n, K), dtype=torch.float32, device=x.device)
        call("gdm_edge_feature_hip", x, idx, B, C, n, K, out)
        ctx.save_for_backward(idx)
        return out

    @staticmethod
    def backward(ctx, go):
        (idx,) = ctx.saved_tensors
        go = go.contiguous()
        B, C2, n, K = go.shape
        g = torch.zeros((B, C2 // 2, n), dtype=torch.float32, device=go.device)
        call("gdm_edge_feature_bwd_hip", go, idx, B, C2 // 2, n, K, g)
        return g, None


def edge_feature(x, idx):
    """x f32[B,C,n], idx int[B,n,K] -> f32[B,2C,n,K] = cat(x_j - x_i, x_i) (dgcnn.py:30-56 get_graph_feature)."""
    idx = _idx32(idx, "idx")
    return _EdgeFeature.apply(x, idx)


class _CircleRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sim, match, item, xyz, vis, radius, gamma, m):
        sim = _dev(sim, torch.float32, "sim")
        R, Mp = sim.shape
        lse_p = torch.empty(R, dtype=torch.float32, device=sim.device)
        lse_n = torch.empty_like(lse_p)
        loss = torch.empty_like(lse_p)
        call("gdm_circle_rows_fwd_hip", sim, R, Mp, match, item, xyz, vis, radius, gamma, m, lse_p, lse_n, loss)
        ctx.save_for_backward(sim, match, item, xyz, vis, lse_p, lse_n)
        ctx.consts = (radius, gamma, m)
        return loss

    @staticmethod
    def backward(ctx, g):
        sim, match, item, xyz, vis, lse_p, lse_n = ctx.saved_tensors
        radius, gamma, m = ctx.consts
        g = g.contiguous()
        R, Mp = sim.shape
        dsim = torch.empty_like(sim)
        call("gdm_circle_rows_bwd_hip", sim, R, Mp, match, item, xyz, vis, radius, gamma, m, lse_p, lse_n, g, dsim)
        return dsim, None, None, None, None, None, None, None


def circle_rows(sim, match, item, xyz, vis, radius, gamma=16.0, m=0.2):
    """Per-row circle loss with the on-the-fly positive mask (geoMatch.py:55-83 + loss.py:470-494).
    sim f32[R,M+1], match int[R] (M = none), item int[R], xyz f32[M,3], vis (any dtype, nonzero = visible)[B,M] -> f32[R]."""
    match = _idx32(match, "match")
    item = _idx32(item, "item")
    xyz = _dev(xyz, torch.float32, "xyz")
    if not vis.is_cuda:
        raise RuntimeError("vis must be a CUDA (HIP) tensor: the geoMatch ops have no CPU fallback")
    vis8 = (vis != 0).to(torch.uint8).contiguous()
    return _CircleRows.apply(sim, match, item, xyz, vis8, float(radius), float(gamma), float(m))


# --------------------------------------------------------------------------------------
# training matching loss without the similarity matrix (gdm_circle.hip)
# --------------------------------------------------------------------------------------
def circle_nbr_table(xyz, radius):
    """Bit table u32[M, ceil(M/32)]: vertices within `radius` of each vertex (the reference's pdist arithmetic).  Depends on the
    model only: build once per (xyz, radius) and reuse."""
    xyz = _dev(xyz, torch.float32, "xyz")
    M = xyz.shape[0]
    nbr = torch.empty((M, (M + 31) // 32), dtype=torch.int32, device=xyz.device)
    call("gdm_circle_match_nbr_hip", xyz, M, float(radius), nbr)
    return nbr


def circle_nbr_items(xyz, rad):
    """Per-item positive tables u32[B, M, ceil(M/32)] for a per-item, per-vertex radius rad f32[B,M]: bit c of row (b, g) =
    sqrt(|xyz_g - xyz_c|^2 + 1e-7) < rad[b, c] (the geoMatch_DGCNN variant, geoMatch_DGCNN.py:62-70)."""
    xyz = _dev(xyz, torch.float32, "xyz")
    rad = _dev(rad, torch.float32, "rad")
    B, M = rad.shape
    assert xyz.shape == (M, 3)
    nbr = torch.empty((B, M, (M + 31) // 32), dtype=torch.int32, device=xyz.device)
    call("gdm_circle_match_nbr_items_hip", xyz, M, rad, B, nbr)
    return nbr


def circle_visbits(vis):
    """visible_flag (any dtype, nonzero = visible) [B,M] -> bits i32[B, ceil(M/32)]."""
    if not vis.is_cuda:
        raise RuntimeError("vis must be a CUDA (HIP) tensor: the geoMatch ops have no CPU fallback")
    v8 = (vis != 0).to(torch.uint8).contiguous()
    B, M = v8.shape
    bits = torch.empty((B, (M + 31) // 32), dtype=torch.int32, device=vis.device)
    call("gdm_circle_match_visbits_hip", v8, B, M, bits)
    return bits


def _cm_pack(x):
    L = _lib.lib()
    n = x.shape[0]
    npad = (n + 127) // 128 * 128
    rows = torch.empty(L.gdm_circle_match_rows_bytes(n), dtype=torch.uint8, device=x.device)
    tp = torch.empty(L.gdm_circle_match_tp_bytes(n), dtype=torch.uint8, device=x.device)
    rsum = torch.empty(npad, dtype=torch.float32, device=x.device)
    call("gdm_circle_match_pack_hip", x, n, rows, tp, rsum)
    return rows, tp, rsum


def _pad_rows(t, npad, fill):
    if t.shape[0] == npad:
        return t.contiguous()
    out = torch.full((npad,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
    out[: t.shape[0]] = t
    return out


class _CircleMatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, g, c2, item, nbr, visb, gamma, m, pad_e0=False):
        x = _dev(x, torch.float32, "x")
        y = _dev(y, torch.float32, "y")
        R, M = x.shape[0], y.shape[0]
        assert x.shape[1] == 128 and y.shape[1] == 128, "descriptors must have 128 channels"
        Rp = (R + 127) // 128 * 128
        xr, xt, xs = _cm_pack(x)
        yr, yt, _ = _cm_pack(y)
        per_item = nbr is not None and nbr.dim() == 3            # [B, M, W]: one table per batch item (circle_nbr_items)
        if pad_e0:
            xs = _pad_rows(x[:, 0].contiguous(), Rp, 0.0)          # <x_r, e0>: the similarity with the padding column
        gp = _pad_rows(g, Rp, M)
        ip = _pad_rows(item, Rp, 0)
        c2p = _pad_rows(c2, Rp, -1) if c2 is not None else None
        lp = torch.empty(Rp, dtype=torch.float32, device=x.device)
        ln = torch.empty_like(lp)
        loss = torch.empty_like(lp)
        call("gdm_circle_match_fwd2_hip", xr, xt, xs, yr, yt, R, M, gp, c2p, ip, nbr, int(per_item), visb, int(bool(pad_e0)), gamma, m, lp,
             ln, loss)
        ctx.save_for_backward(xr, xt, xs, yr, yt, gp, ip, lp, ln)
        ctx.extra = (c2p, nbr, visb, gamma, m, R, M, per_item, bool(pad_e0))
        return loss[:R]

    @staticmethod
    def backward(ctx, gout):
        xr, xt, xs, yr, yt, gp, ip, lp, ln = ctx.saved_tensors
        c2p, nbr, visb, gamma, m, R, M, per_item, pad_e0 = ctx.extra
        L = _lib.lib()
        Rp, Mp = lp.shape[0], (M + 127) // 128 * 128
        z = lp[:R] + ln[:R]
        sig = torch.where(z > 20.0, torch.ones_like(z), torch.sigmoid(z))            # d softplus
        coef = torch.where(torch.isfinite(lp[:R]), gout.contiguous().float() * sig, torch.zeros_like(z))   # empty positive set: 0
        coef = _pad_rows(coef, Rp, 0.0)
        P = int(L.gdm_circle_match_bwd_parts(R, M))
        gx = torch.empty((Rp, 128), dtype=torch.float32, device=lp.device)
        gyp = torch.empty((P, Mp, 128), dtype=torch.float32, device=lp.device)
        call("gdm_circle_match_bwd2_hip", xr, xt, xs, yr, yt, R, M, gp, c2p, ip, nbr, int(per_item), visb, int(pad_e0), gamma, m, lp, ln,
             coef, gx, gyp)
        return gx[:R], gyp.sum(dim=0)[:M], None, None, None, None, None, None, None, None


def circle_match(x, y, g, item, nbr=None, visb=None, c2=None, gamma=16.0, m=0.2, pad="ones"):
    """Per-row circle loss of unit scene rows x f32[R,128] against unit vertex rows y f32[M,128] WITHOUT the [R, M+1] similarity
    matrix (geoMatch.py:117-136 + :55-100 + loss.py:441-494, forward and backward).  g int[R]: ground-truth vertex (M = none),
    item int[R]: batch item; positives from `nbr` (circle_nbr_table) & `visb` (circle_visbits), or -- symmetric objects -- the two
    columns g / c2 of each row.  `nbr` may be one table per batch item (circle_nbr_items, [B, M, W]); pad = "ones": the padding column
    is -1/sqrt(128) everywhere (geoMatch.py:117-119), "e0": the unit vector e0 (geoMatch_DGCNN.py:96-99).  Returns f32[R];
    differentiable w.r.t. x and y."""
    if pad not in ("ones", "e0"):
        raise ValueError("circle_match: pad=%r" % (pad,))
    g = _idx32(g, "g")
    item = _idx32(item, "item")
    if c2 is not None:
        c2 = _idx32(c2, "c2")
    elif nbr is None or visb is None:
        raise ValueError("circle_match: pass nbr and visb (radius-test positives) or c2 (symmetric objects)")
    return _CircleMatch.apply(x, y, g, c2, item, nbr, visb, float(gamma), float(m), pad == "e0")


SOFT_COORD_MAX_GAMMA = _lib.GDM_SOFT_COORD_MAX_GAMMA


# The differentiable soft assignment is registered through torch.library (custom_op + register_autograd), not as an autograd.Function
# subclass: two operators, gdm::soft_coord_fwd and gdm::soft_coord_bwd, each a fixed sequence of launches on the current stream with
# no host read and no allocation that depends on data, so a hipGraph capture records them like any other operator.
@torch.library.custom_op("gdm::soft_coord_fwd", mutates_args=(), device_types="cuda")
def _soft_coord_fwd(x: torch.Tensor, y: torch.Tensor, xyz: torch.Tensor,
                    gamma: float) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    R, M = x.shape[0], y.shape[0]
    xr, xt, _ = _cm_pack(x)
    yr, yt, _ = _cm_pack(y)
    lse = torch.empty(R, dtype=torch.float32, device=x.device)
    soft = torch.empty((R, 3), dtype=torch.float32, device=x.device)
    call("gdm_soft_coord_fwd_hip", xr, xt, yr, yt, xyz, R, M, gamma, lse, soft)
    return lse, soft, xr, xt, yr, yt


@_soft_coord_fwd.register_fake
def _(x, y, xyz, gamma):
    def nb(n):
        return (n + 127) // 128 * 128
    R, M = x.shape[0], y.shape[0]
    u8 = dict(dtype=torch.uint8, device=x.device)
    return (x.new_empty(R), x.new_empty((R, 3)), torch.empty(nb(R) * 512, **u8), torch.empty(nb(R) * 512, **u8),
            torch.empty(nb(M) * 512, **u8), torch.empty(nb(M) * 512, **u8))


@torch.library.custom_op("gdm::soft_coord_bwd", mutates_args=(), device_types="cuda")
def _soft_coord_bwd(xr: torch.Tensor, xt: torch.Tensor, yr: torch.Tensor, yt: torch.Tensor, xyz: torch.Tensor, lse: torch.Tensor,
                    kb: torch.Tensor, M: int, gamma: float) -> tuple[torch.Tensor, torch.Tensor]:
    L = _lib.lib()
    R = lse.shape[0]
    P = int(L.gdm_soft_coord_bwd_parts(R, M))
    Mp = (M + 127) // 128 * 128
    gx = torch.empty((R, 128), dtype=torch.float32, device=lse.device)
    gy = torch.empty((M, 128), dtype=torch.float32, device=lse.device)
    part = torch.empty((P, Mp, 128), dtype=torch.float32, device=lse.device)
    call("gdm_soft_coord_bwd_hip", xr, xt, yr, yt, xyz, R, M, gamma, lse, kb, gx, part, gy)
    return gx, gy


@_soft_coord_bwd.register_fake
def _(xr, xt, yr, yt, xyz, lse, kb, M, gamma):
    return lse.new_empty((lse.shape[0], 128)), lse.new_empty((M, 128))


def _soft_coord_setup(ctx, inputs, output):
    x, y, xyz, gamma = inputs
    lse, soft, xr, xt, yr, yt = output
    ctx.save_for_backward(xr, xt, yr, yt, xyz, lse, soft)
    ctx.gamma, ctx.M = gamma, y.shape[0]


def _soft_coord_backward(ctx, g_lse, g_soft, *unused):
    xr, xt, yr, yt, xyz, lse, soft = ctx.saved_tensors
    a = g_lse.to(torch.float32)
    b = g_soft.to(torch.float32)
    k = a - (b * soft).sum(dim=1)                                  # k_r = a_r - b_r . soft_r
    kb = torch.cat([k.unsqueeze(1), b], dim=1).contiguous()        # [R,4]
    gx, gy = _soft_coord_bwd(xr, xt, yr, yt, xyz, lse, kb, ctx.M, ctx.gamma)
    return gx, gy, None, None


_soft_coord_fwd.register_autograd(_soft_coord_backward, setup_context=_soft_coord_setup)


def soft_coord_match(x, y, xyz, gamma=16.0):
    """The differentiable soft assignment of unit scene rows x f32[R,128] over the unit vertex rows y f32[M,128] with coordinates
    xyz f32[M,3], WITHOUT the [R, M] similarity matrix (csrc/gdm_softcoord.hip, forward and backward on the matrix cores):
        lse_r = log sum_c exp(gamma <x_r, y_c>)            f32[R]
        soft_r = sum_c softmax_c(gamma <x_r, y_c>) xyz_c    f32[R,3]   the expected model coordinate
    over exactly the M vertices; 0 < gamma <= 40.  Differentiable w.r.t. x and y (not xyz); normalisation stays with the caller's
    autograd, as for circle_match.  loss.soft_coord_reference states the same in plain torch."""
    gamma = float(gamma)
    if not (0.0 < gamma <= SOFT_COORD_MAX_GAMMA):                  # NaN fails both comparisons; refused before any launch
        raise ValueError("soft_coord_match: gamma=%r outside (0, %g]" % (gamma, SOFT_COORD_MAX_GAMMA))
    x = _dev(x, torch.float32, "x")
    y = _dev(y, torch.float32, "y")
    xyz = _dev(xyz, torch.float32, "xyz")
    if x.dim() != 2 or y.dim() != 2 or x.shape[1] != 128 or y.shape[1] != 128 or x.shape[0] < 1 or y.shape[0] < 1:
        raise ValueError("soft_coord_match: x [R,128] and y [M,128] with R, M >= 1, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    if tuple(xyz.shape) != (y.shape[0], 3):
        raise ValueError("soft_coord_match: xyz must be [M,3] = [%d,3], got %s" % (y.shape[0], tuple(xyz.shape)))
    lse, soft = _soft_coord_fwd(x, y, xyz.detach(), gamma)[:2]
    return lse, soft


ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


def affine_act(x, scale, shift, act=ACT_NONE, slope=0.0, res=None, res_scale=None, res_shift=None, inplace=True):
    """Inference only (no autograd): y = act(x*scale[c] + shift[c] (+ res*res_scale[c] + res_shift[c])) for
    x f32[B,C,...] contiguous.  Folded eval BatchNorm + activation (+ residual) in one launch."""
    x = _dev(x, torch.float32, "x")
    B, C = x.shape[0], x.shape[1]
    inner = x.numel() // (B * C)
    if inner % 4 != 0 or B * C > 65535 or x.data_ptr() % 16 != 0:
        y = x * scale.view(1, C, *([1] * (x.dim() - 2))) + shift.view(1, C, *([1] * (x.dim() - 2)))
        if res is not None:
            y = y + (res * res_scale.view_as(scale.view(1, C, *([1] * (x.dim() - 2)))) + res_shift.view(1, C, *([1] * (x.dim() - 2)))
                     if res_scale is not None else res)
        if act == ACT_RELU:
            y = torch.relu(y)
        elif act == ACT_LEAKY:
            y = torch.where(y > 0, y, y * slope)
        return y
    if res is not None:
        res = _dev(res, torch.float32, "res")
        if res.data_ptr() % 16:
            res = res.clone()                        # the kernel reads it four elements at a time
        assert res.shape == x.shape
    y = x if inplace else torch.empty_like(x)
    call("gdm_affine_act_hip", x, scale, shift, res, res_scale, res_shift, B * C, C, inner, act, float(slope), y)
    return y


def _pw_seg(spec, B, name):
    """(x f32[B,C,n_src(,1)] channel-major[, idx int[B,n(,1)]]) -> (_lib.PwSeg, tensors to keep alive, n or None)."""
    x, idx = (spec, None) if torch.is_tensor(spec) else (spec[0], spec[1])
    x = _dev(x, torch.float32, name)
    if x.dim() == 4 and x.shape[3] == 1:
        x = x.reshape(x.shape[0], x.shape[1], x.shape[2])
    if x.dim() != 3 or x.shape[0] != B:
        raise ValueError("pointwise: %s must be [B,C,n(,1)] with B=%d, got %s" % (name, B, tuple(x.shape)))
    n = None
    if idx is not None:
        idx = _idx32(idx, name + " index").reshape(B, -1)
        n = idx.shape[1]
    seg = _lib.PwSeg(x.data_ptr(), idx.data_ptr() if idx is not None else None, x.shape[1], x.shape[2])
    return seg, (x, idx), n


def pointwise(segs, wt, scale=None, shift=None, act=ACT_NONE, slope=0.0, point_major=False, out=None, out_c0=0, w_rowmajor=False):
    """One per-point (1x1) layer in one launch (include/gdm.h gdm_pointwise2_hip), inference only:
        y[b,:,i] = act(scale * (W . cat(segs)[b,:,i]) + shift)
    segs: a list of one to four (three when the layer has fewer than 32 input channels) of  x f32[B,C,n(,1)]  or  (x f32[B,C,n_src(,1)], idx int[B,n(,1)])  -- the concat along channels
    is never formed, an indexed segment is read through its index (nearest-neighbour interpolation folded into the load).
    wt f32[K,Cout]: the layer's weight TRANSPOSED (K = total input channels); w_rowmajor: wt is f32[Cout,K] instead, the weight as an
    nn.Conv1d / nn.Conv2d holds it (the training path: no transposed copy of a weight that changes every step).
    Returns f32[B,Cout,n], or f32[B,n,Cout] when point_major; with `out` (f32[B,outC,n] / [B,n,outC]) channels
    [out_c0, out_c0+Cout) of it are written instead."""
    if not isinstance(segs, list):
        segs = [segs]
    first = segs[0] if torch.is_tensor(segs[0]) else segs[0][0]
    B = first.shape[0]
    wt = _dev(wt, torch.float32, "wt")
    K, Cout = (wt.shape[1], wt.shape[0]) if w_rowmajor else wt.shape
    if w_rowmajor and K >= 32 and B * first.numel() // max(1, first.shape[0] * first.shape[1]) >= 131072:
        # many points: the kernel's weight fragment loads run along Cout ([K, Cout]: one 64-byte piece per K row; from [Cout, K] sixteen
        # cache lines per load -- 76 vs 52 us at 64 -> 64 channels, 393 k points), so the few-KB transposed copy pays for itself
        wt, w_rowmajor = wt.t().contiguous(), False
    arr = (_lib.PwSeg * len(segs))()
    keep = []
    n = None
    ksum = 0
    for i, sp in enumerate(segs):
        seg, k, ni = _pw_seg(sp, B, "segment %d" % i)
        arr[i] = seg
        keep.append(k)
        ksum += seg.C
        ni = ni if ni is not None else seg.n_src
        if n is not None and ni != n:
            raise ValueError("pointwise: segments disagree on the number of points (%d vs %d)" % (n, ni))
        n = ni
    if ksum != K:
        raise ValueError("pointwise: weight has %d input rows, the segments %d channels" % (K, ksum))
    if out is None:
        out = torch.empty((B, n, Cout) if point_major else (B, Cout, n), dtype=torch.float32, device=wt.device)
        outC = Cout
    else:
        outC = out.shape[2] if point_major else out.shape[1]
        if not out.is_contiguous() or out.dtype != torch.float32 or out.shape[0] != B or (out.shape[1] if point_major else out.shape[2]) != n:
            raise ValueError("pointwise: out must be a contiguous f32 [B,%s] tensor" % ("n,outC" if point_major else "outC,n"))
    call("gdm_pointwise2_hip", arr, len(segs), wt, 1 if w_rowmajor else 0, scale, shift, B, n, Cout, int(act), float(slope), out, outC,
         int(out_c0), 1 if point_major else 0)
    return out


def pointwise_chain2(x, p0, p1):
    """Two chained narrow per-point layers in one launch (include/gdm.h gdm_pointwise_chain2_hip): x f32[B,C0,n]; p0, p1 =
    (wt [K,Cout], scale, shift, act, slope) as `_FusedConvMixin._pointwise_params` gives them -> (y0 [B,C1,n], y1 [B,C2,n])."""
    x = _dev(x, torch.float32, "x")
    B, C0, n = x.shape
    (w0, s0, b0, a0, sl0), (w1, s1, b1, a1, sl1) = p0, p1
    C1, C2 = w0.shape[1], w1.shape[1]
    if w0.shape[0] != C0 or w1.shape[0] != C1:
        raise ValueError("pointwise_chain2: weights %s, %s do not chain from %d channels" % (tuple(w0.shape), tuple(w1.shape), C0))
    y0 = torch.empty((B, C1, n), dtype=torch.float32, device=x.device)
    y1 = torch.empty((B, C2, n), dtype=torch.float32, device=x.device)
    call("gdm_pointwise_chain2_hip", x, w0, s0, b0, int(a0), float(sl0), w1, s1, b1, int(a1), float(sl1), B, n, C0, C1, C2, y0, y1)
    return y0, y1


def pointwise_jobs(xs, wts):
    """Up to four independent plain per-point layers of equal K and Cout in ONE launch (include/gdm.h gdm_pointwise_jobs_hip):
    xs[j] f32[B,K,n_j], wts[j] f32[K,Cout] (the weight transposed) -> [f32[B,Cout,n_j]].  Bit-identical to `pointwise([x], wt)` per
    job (same tile function, same K split); jobs whose K splits would differ alone go in one launch per distinct split."""
    if not (1 <= len(xs) <= 4 and len(xs) == len(wts)):
        raise ValueError("pointwise_jobs: one to four (x, wt) pairs")
    B, K = xs[0].shape[0], xs[0].shape[1]
    Cout = wts[0].shape[1]
    arr = (_lib.PwJob * len(xs))()
    keep, outs = [], []
    for j, (x, wt) in enumerate(zip(xs, wts)):
        x = _dev(x.reshape(x.shape[0], x.shape[1], -1), torch.float32, "xs[%d]" % j)
        wt = _dev(wt, torch.float32, "wts[%d]" % j)
        if x.shape[0] != B or x.shape[1] != K or tuple(wt.shape) != (K, Cout):
            raise ValueError("pointwise_jobs: job %d has x %s / wt %s, job 0 has B=%d K=%d Cout=%d" % (j, tuple(x.shape), tuple(wt.shape), B, K, Cout))
        out = torch.empty((B, Cout, x.shape[2]), dtype=torch.float32, device=x.device)
        arr[j] = _lib.PwJob(x.data_ptr(), wt.data_ptr(), out.data_ptr(), x.shape[2])
        keep += [x, wt]
        outs.append(out)
    call("gdm_pointwise_jobs_hip", arr, len(xs), B, K, Cout)
    return outs


def _fold_and_all_reduce(sums, C, group):
    """Partial pairs [G][C][2] + count + G  ->  double[2C+1] = one pair per channel + count, summed over the ranks of `group`."""
    import torch.distributed as dist
    compact = torch.cat([sums[:-2].view(-1, 2 * C).sum(0), sums[-2:-1]])
    if dist.get_backend(group) == "nccl":
        dist.all_reduce(compact, group=group)
    else:                                                   # gloo rehearsals: through host memory
        host = compact.cpu()
        dist.all_reduce(host, group=group)
        compact = host.to(sums.device)
    return compact


class _BatchNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, eps, momentum, act, slope, group):
        x = _dev(x, torch.float32, "x")
        B, C = x.shape[0], x.shape[1]
        inner = x.numel() // (B * C)
        L = _lib.lib()
        sums = torch.empty(L.gdm_bn_sums_len(B, C, inner), dtype=torch.float64, device=x.device)
        saved = torch.empty(5 * C, dtype=torch.float32, device=x.device)       # a | b | fp32 mean | rstd | mean - fp32 mean
        y = torch.empty_like(x)
        call("gdm_bn_stats_hip", x, B, C, inner, sums)
        groups = 0
        if group is not None:                               # SyncBatchNorm: statistics over the whole data-parallel batch
            sums, groups = _fold_and_all_reduce(sums, C, group), 1
        call("gdm_bn_fwd_apply_hip", x, sums, groups, weight, bias, B, C, inner, float(eps), float(momentum), act, float(slope), saved,
             running_mean, running_var, y)
        ctx.save_for_backward(x, weight, saved)
        ctx.act, ctx.slope, ctx.group = act, float(slope), group
        return y

    @staticmethod
    def backward(ctx, go):
        x, weight, saved = ctx.saved_tensors
        go = _dev(go, torch.float32, "grad")
        B, C = x.shape[0], x.shape[1]
        inner = x.numel() // (B * C)
        L = _lib.lib()
        sums = torch.empty(L.gdm_bn_sums_len(B, C, inner), dtype=torch.float64, device=x.device)
        gw = torch.empty(C, dtype=torch.float32, device=x.device)
        gb = torch.empty(C, dtype=torch.float32, device=x.device)
        gx = torch.empty_like(x)
        call("gdm_bn_bwd_reduce_hip", x, go, saved, B, C, inner, ctx.act, ctx.slope, sums)
        groups = 0
        local = None
        if ctx.group is not None:
            # grad_x needs the sums over the whole batch; grad weight / bias stay LOCAL sums (DDP averages parameter gradients over
            # the ranks afterwards, as with nn.SyncBatchNorm)
            local = sums[:-2].view(-1, C, 2).sum(0)
            sums, groups = _fold_and_all_reduce(sums, C, ctx.group), 1
        call("gdm_bn_bwd_apply_hip", x, go, sums, groups, weight, saved, B, C, inner, ctx.act, ctx.slope, gw, gb, gx)
        if local is not None:
            mean, rstd = saved[2 * C:3 * C].double() + saved[4 * C:].double(), saved[3 * C:4 * C].double()
            gb = local[:, 0].float()
            gw = (rstd * (local[:, 1] - mean * local[:, 0])).float()
        return gx, gw, gb, None, None, None, None, None, None, None




def _sync_group(bn):
    """Process group of a SyncBatchNorm that actually spans several ranks, else None."""
    import torch.distributed as dist
    if not (isinstance(bn, torch.nn.SyncBatchNorm) and dist.is_available() and dist.is_initialized()):
        return None
    group = bn.process_group if bn.process_group is not None else dist.group.WORLD
    return group if dist.get_world_size(group) >= settings.SYNCBN_MIN_WORLD else None


def bn_train_supported(x, bn):
    """Affine BatchNorm{1,2}d -- or SyncBatchNorm -- in training mode with torch-style running statistics, on a contiguous f32 GPU map
    whose inner size is a multiple of 4."""
    if not (settings.USE_FUSED_BN_TRAIN and bn.training and x.is_cuda and x.dtype == torch.float32 and x.dim() >= 3 and x.is_contiguous()):
        return False
    if type(bn) not in (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d) and not (settings.USE_FUSED_SYNCBN and type(bn) is torch.nn.SyncBatchNorm):
        return False
    if not bn.affine or bn.momentum is None or not bn.track_running_stats:
        return False
    B, C = x.shape[0], x.shape[1]
    inner = x.numel() // max(B * C, 1)
    return B * C <= 65535 and inner >= 4 and inner % 4 == 0 and x.data_ptr() % 16 == 0 and B * inner > 1


def batch_norm_act_train(x, bn, act=ACT_NONE, slope=0.0):
    """Training-mode `act(bn(x))` (batch statistics -- over all ranks for a SyncBatchNorm -- and running statistics updated as the
    module does) with a fused backward.  act: ACT_NONE / ACT_RELU / ACT_LEAKY(slope).  Caller checks bn_train_supported."""
    y = _BatchNormAct.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum, act, slope, _sync_group(bn))
    if bn.num_batches_tracked is not None:
        if _bn_counters is not None:
            _bn_counters.append(bn.num_batches_tracked)           # one multi-tensor add for the whole forward (batched_bn_counters)
        else:
            bn.num_batches_tracked.add_(1)
    return y


_bn_counters = None


class batched_bn_counters:
    """with ops.batched_bn_counters(): ... -- the `num_batches_tracked += 1` of every fused training BatchNorm inside the scope is applied
    at its exit as ONE multi-tensor add instead of one tiny launch per layer (91 launches, 0.34 ms of a training step).  Same values
    after the scope as the modules leave; nothing reads the counters inside a forward (momentum is a number in every layer here)."""

    def __enter__(self):
        global _bn_counters
        self.prev, _bn_counters = _bn_counters, []
        return self

    def __exit__(self, *exc):
        global _bn_counters
        pending, _bn_counters = _bn_counters, self.prev
        if pending:
            torch._foreach_add_(pending, 1)
        return False


def upconv3x3_gather(z, scale, shift, cout, out_size, act=ACT_NONE, slope=0.0, packed=False):
    """z f32[B, 9*cout, H, W] (low-resolution tap-major channel mixes) -> f32[B, cout, OH, OW]: the 9-tap bilinear
    gather that completes conv3x3(upsample(x)) + folded BN + activation.  Inference only.  packed: the eight-channel form, which also
    writes the packed split-bf16 operand of the GEMM that reads the map next (hung on the result as `_gdm_packed`)."""
    z = _dev(z, torch.float32, "z")
    B, c9, H, W = z.shape
    assert c9 == 9 * cout
    OH, OW = int(out_size[0]), int(out_size[1])
    out = torch.empty((B, cout, OH, OW), dtype=torch.float32, device=z.device)
    if packed and packed_out_supported(B, cout, OH, OW, grid_groups=True) and (OH, OW) == (2 * H, 2 * W):   # (blockIdx.z = group; x2: its LDS tile)
        opk = _packed_out(B, cout, OH, OW, z.device)
        call("gdm_upconv3x3_gather2_hip", z, scale, shift, B, cout, H, W, OH, OW, act, float(slope), out, opk.buf)
        return carry_packed(out, opk)
    call("gdm_upconv3x3_gather_hip", z, scale, shift, B, cout, H, W, OH, OW, act, float(slope), out)
    return out


def upconv_fused64_pack_weight(weight):
    """conv weight f32[64,64,3,3] -> packed split-bf16 rows for upconv_fused64."""
    w = _dev(weight.detach(), torch.float32, "weight")
    if tuple(w.shape) != (64, 64, 3, 3):
        raise ValueError("upconv_fused64_pack_weight: weight must be [64,64,3,3], got %s" % (tuple(w.shape),))
    L = _lib.lib()
    wpk = torch.empty(L.gdm_upconv_fused64_weight_bytes(), dtype=torch.uint8, device=w.device)
    call("gdm_upconv_fused64_pack_weight_hip", w, wpk)
    return wpk


def upconv_fused64(x, wpk, scale, shift, out_size, act=0, slope=0.0):
    """act(scale * conv3x3(upsample_bilinear_ac(x)) + shift) for 64 -> 64 channels in one kernel.  Inference only."""
    x = _dev(x, torch.float32, "x")
    B, C, H, W = x.shape
    OH, OW = int(out_size[0]), int(out_size[1])
    out = torch.empty((B, C, OH, OW), dtype=torch.float32, device=x.device)
    call("gdm_upconv_fused64_hip", x, wpk, scale, shift, B, C, H, W, OH, OW, act, float(slope), out)
    return out


class _UpconvGather(torch.autograd.Function):
    """out = 9-tap bilinear gather of z (+ bias[co]); differentiable in z and bias (training form of PSPUpsample)."""

    @staticmethod
    def forward(ctx, z, bias, cout, OH, OW):
        z = z.contiguous()
        B, c9, H, W = z.shape
        ones = torch.ones(cout, dtype=torch.float32, device=z.device)
        shift = bias.detach().contiguous() if bias is not None else torch.zeros(cout, dtype=torch.float32, device=z.device)
        out = torch.empty((B, cout, OH, OW), dtype=torch.float32, device=z.device)
        call("gdm_upconv3x3_gather_hip", z, ones, shift, B, cout, H, W, OH, OW, ACT_NONE, 0.0, out)
        ctx.shape = (B, cout, H, W, OH, OW)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, go):
        B, cout, H, W, OH, OW = ctx.shape
        go = go.contiguous()
        gz = torch.empty((B, 9 * cout, H, W), dtype=torch.float32, device=go.device)
        call("gdm_upconv3x3_gather_bwd_hip", go, B, cout, H, W, OH, OW, gz)
        return gz, (channel_sum(go) if ctx.has_bias else None), None, None, None


def upconv3x3_gather_train(z, bias, cout, out_size):
    """Differentiable form of upconv3x3_gather without the folded BN / activation: z f32[B,9*cout,H,W] -> f32[B,cout,OH,OW] (+ bias)."""
    z = _dev(z, torch.float32, "z")
    assert z.shape[1] == 9 * cout
    return _UpconvGather.apply(z, bias, cout, int(out_size[0]), int(out_size[1]))


def wx(w2d, x3):
    """W f32[Cout,Cin] . x f32[B,Cin,n] -> f32[B,Cout,n] as ONE batched GEMM on the shared weight.  torch.matmul(2-D, 3-D) folds the
    batch into GEMM rows instead and pays a transposing copy of the product (and of its gradient) to get back to [B,Cout,n]:
    2 ms of an 83 ms training step on the 9*Cout-channel tap tensors of PSPUpsample.  Under autograd: _WxTrain (train_plan)."""
    if torch.is_grad_enabled() and (w2d.requires_grad or x3.requires_grad) and x3.is_cuda and x3.dtype == torch.float32:
        return _WxTrain.apply(x3.contiguous(), w2d.contiguous())
    return torch.bmm(w2d.unsqueeze(0).expand(x3.shape[0], -1, -1), x3)


OPERAND_LIMIT = 1 << 31


def operands_fit(*nbytes):
    """The convolution / GEMM kernel (csrc/gdm_conv.hip conv_mfma16_kernel) addresses its packed activations and its packed weights with
    32-bit byte offsets: each operand must stay below 2 GiB, and the library refuses a launch that does not.  nbytes: what the library's
    own size functions give for the operands of one launch (0 = a shape they do not take).  Every wrapper below asks this before it
    allocates anything, and every *_supported predicate asks it so that the modules take their torch path past the limit."""
    return all(0 < n < OPERAND_LIMIT for n in nbytes)


def _require_fit(who, what, args, act_bytes, weight_bytes=None):
    """ValueError unless the operands of a launch fit (weight_bytes None: a pack launch, which has the activations only).  `what % args`
    describes the shapes; it is formatted only for the message."""
    if not operands_fit(act_bytes, *(() if weight_bytes is None else (weight_bytes,))):
        raise ValueError("%s: %s needs packed activations of %d bytes%s; a packed operand must be above 0 and below 2 GiB (%d bytes)"
                         % (who, what % args, act_bytes, "" if weight_bytes is None else " and packed weights of %d bytes" % weight_bytes,
                            OPERAND_LIMIT))


def _map_bytes(B, C, H, W):
    """Bytes of the packed operand of a [B,C,H,W] map (0: not a map the pack kernel takes)."""
    return _lib.lib().gdm_conv3x3_act_bytes(B, C, H, W)


def _wgrad_parts(nchunk, tiles):
    """K split of a pixel-contraction GEMM: the largest divisor of the chunk count that keeps the launch near one round of
    workgroups (a part has `tiles` of them) and at least four chunks per part."""
    parts = 1
    for d in range(1, nchunk + 1):
        if nchunk % d == 0 and d * tiles <= 320 and nchunk // d >= 4:
            parts = d
    return parts


def _wgrad_packed(who, x, go, taps, parts=None):
    """The weight-gradient launch of the split-bf16 MFMA GEMM with the pixels as the contraction axis, for a 1x1 product (taps 1:
    x f32[B,Cin,P], go f32[B,Cout,P]) or a 3x3 / stride 1 / pad 1 convolution (taps 9: x f32[B,Cin,H,W], go f32[B,Cout,H,W])
    -> f32[Cout,taps,Cin].  Sizes, fit check, two packs, one launch over `parts` equal parts of the contraction (_wgrad_parts unless
    given), whose partial products are added in a fixed order (deterministic).  Every ValueError comes from the shapes alone."""
    B, Cin, Cout = x.shape[0], x.shape[1], go.shape[1]
    H, W = (x.shape[2] // 32, 32) if taps == 1 else (x.shape[2], x.shape[3])      # a 1x1 product packs grad_out as rows of 32 pixels
    P = x.shape[2] if taps == 1 else H * W
    L = _lib.lib()
    nx = L.gdm_wgrad_x1_bytes(B, Cin, P) if taps == 1 else L.gdm_wgrad_x_bytes(B, Cin, H, W)
    ng = L.gdm_wgrad_go_bytes(B, Cout, H, W)
    if nx == 0 or ng == 0 or (taps * Cin) % 256 != 0:
        raise ValueError("%s: unsupported shape x %s grad_out %s" % (who, tuple(x.shape), tuple(go.shape)))
    _require_fit(who, "x %s grad_out %s", (tuple(x.shape), tuple(go.shape)), nx, ng)
    nchunk = B * P // 128
    if parts is None:
        parts = _wgrad_parts(nchunk, (taps * Cin // 256) * ((Cout + 127) // 128))
    if nchunk % parts != 0:
        raise ValueError("%s: %d parts do not divide the %d chunks of the contraction" % (who, parts, nchunk))
    x, go = _dev(x, torch.float32, "x"), _dev(go, torch.float32, "grad_out")
    xpk, gpk = torch.empty(nx, dtype=torch.uint8, device=x.device), torch.empty(ng, dtype=torch.uint8, device=x.device)
    if taps == 1:
        call("gdm_wgrad_pack_x1_hip", x, B, Cin, P, xpk)
    else:
        call("gdm_wgrad_pack_x_hip", x, B, Cin, H, W, xpk)
    call("gdm_wgrad_pack_go_hip", go, B, Cout, H, W, gpk)
    n = nchunk // parts
    coutp = (Cout + 127) // 128 * 128
    out = torch.empty((parts, Cout, taps, Cin), dtype=torch.float32, device=x.device)
    call("gdm_conv1x1_packed_wb_hip", xpk, gpk, n * coutp * 512, parts, 128 * n, Cout, taps, Cin, out)
    return out[0] if parts == 1 else out.sum(0)


def gemm_wgrad(x3, go3):
    """dW f32[Cout,Cin] = sum_b go3[b] . x3[b]^T (x3 f32[B,Cin,P], go3 f32[B,Cout,P]) on the split-bf16 MFMA GEMM with the pixels as the
    contraction axis (include/gdm.h gdm_wgrad_pack_x1_hip): the weight gradient of a 1x1 convolution / of `wx`."""
    B, Cin, P = x3.shape
    return _wgrad_packed("gemm_wgrad", x3, go3, 1).view(go3.shape[1], Cin)


def _rows_ok(t):
    """[B,C,P] with contiguous rows of P floats, channel stride P, any batch stride (a channel slice of a concatenation qualifies)."""
    return t.stride(2) == 1 and t.stride(1) == t.shape[2] and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0


def wgrad_direct(x3, go3, bias=False):
    """(dW f32[Cout,Cin], db f32[Cout] or None) = (sum_{b,p} go3[b,:,p] x3[b,:,p]^T, sum_{b,p} go3[b,:,p]) in one pass over the fp32
    rows (split-bf16 MFMA, K split over workgroups, partials added in fixed order)."""
    B, Cin, P = x3.shape
    Cout = go3.shape[1]
    nsteps = B * (P // 32)
    bm, bn = (64 if Cout > 32 else 32), (64 if Cin > 32 else 32)        # the workgroup's block of dW (csrc/gdm_wgrad.hip)
    blocks = -(-Cout // bm) * -(-Cin // bn)
    slices = 4 // ((2 if Cout > 32 else 1) * (2 if Cin > 32 else 1))    # pixel slices inside a workgroup
    nsplit = max(1, min(nsteps // (8 * slices), 512 // blocks))           # >= 8 steps per wave, two workgroups per CU = one resident round
    part = torch.empty((nsplit, Cout, Cin), dtype=torch.float32, device=x3.device)
    bpart = torch.empty((nsplit, Cout), dtype=torch.float32, device=x3.device) if bias else None
    call("gdm_wgrad_direct_hip", go3, go3.stride(0), x3, x3.stride(0), B, Cout, Cin, P, nsplit, part, bpart)
    return part.sum(0), (bpart.sum(0) if bias else None)


TrainPlan = collections.namedtuple("TrainPlan", "function fwd dgrad wgrad asks_mfma fits")


def train_plan(entry, B, cin, cout, n, cuda=True, bias_grad=False):
    """Which engine makes each product of one training step of a 1x1 layer x f32[B,cin,n] -> cout channels, from what is known before a
    tensor is touched.  entry: "wx", "conv1x1_train" or "conv1x1_train_w"; cuda: the operands are fp32 tensors on the GPU (anything else
    goes to torch); bias_grad: the layer has a bias whose gradient is wanted.  -> TrainPlan (cached: layer shapes repeat every step):
      function   the autograd Function the entry point applies, "_WxTrain" or "_Conv1x1Train"
      fwd dgrad  the engine of W . x and of W^T . go: "gemm_bf16x3" (>= 2 GFLOP) before "pointwise" before "torch.bmm"
      wgrad      the engines of sum_b go . x^T in order of preference: "gemm_wgrad" (>= 2 GFLOP), "wgrad_direct", "torch.bmm".  Row layout
                 is the one run-time condition (wgrad_direct wants _rows_ok of x and go; go exists only in the backward): _train_wgrad
      asks_mfma  False: no product is offered to the split-bf16 MFMA GEMM;  fits: False when a product that GEMM takes by shape and
                 size has an operand of 2 GiB or more (conv1x1_train_supported)"""
    return _train_plan(entry, int(B), int(cin), int(cout), int(n), bool(cuda), bool(bias_grad),
                       settings.USE_MFMA_GEMM_TRAIN, settings.USE_POINTWISE_TRAIN, settings.USE_DIRECT_WGRAD)


@functools.lru_cache(maxsize=4096)
def _train_plan(entry, B, cin, cout, n, cuda, bias_grad, use_mfma, use_pointwise, use_direct):
    L = _lib.lib()
    big = use_mfma and cuda and 2.0 * B * n * cin * cout >= 2e9
    # per product (the MFMA GEMM takes it by shape and size, its operands fit): W . x on x, W^T . go on go, go . x^T
    mfma = [(big and gemm_shape_supported(ci, co, n), operands_fit(_map_bytes(B, ci, 1, n), L.gdm_conv1x1_weight_bytes(co, ci)))
            for ci, co in ((cin, cout), (cout, cin))]
    mfma.append((big and n % 128 == 0 and cin % 256 == 0 and cout >= 64,
                 operands_fit(L.gdm_wgrad_x1_bytes(B, cin, n), L.gdm_wgrad_go_bytes(B, cout, n // 32, 32))))
    fwd_mfma, dgrad_mfma, wgrad_mfma = (takes and fits for takes, fits in mfma)
    function = "_WxTrain" if entry == "wx" or (entry == "conv1x1_train" and (fwd_mfma or dgrad_mfma)) else "_Conv1x1Train"
    # INHERITED, NOT DESIGNED: _Conv1x1Train (always applied by conv1x1_train_w) never asked the MFMA GEMM for anything.  conv1x1_train
    # chooses it exactly when neither W . x nor W^T . go is a product that GEMM takes, so there the flag decides the weight gradient alone:
    # Cin % 256 == 0, Cout in [64, 192) other than 64 and 128, n % 128 == 0, >= 2 GFLOP goes to gemm_wgrad through wx, to torch.bmm through
    # conv1x1_train.  True everywhere needs a GPU measurement of gemm_wgrad against torch.bmm / wgrad_direct in that class first.
    asks_mfma = function == "_WxTrain"
    other = "pointwise" if use_pointwise and cuda else "torch.bmm"
    # wgrad_direct: up to 64 x 64 channels, 128 x 128 when the bias gradient rides along in the call (measurements: DESIGN.md 6o)
    lim = 128 if bias_grad and not asks_mfma else 64
    direct = use_direct and cuda and n % 32 == 0 and cin <= lim and cout <= lim and B * n >= 16384
    return TrainPlan(function, "gemm_bf16x3" if asks_mfma and fwd_mfma else other, "gemm_bf16x3" if asks_mfma and dgrad_mfma else other,
                     (("gemm_wgrad",) if asks_mfma and wgrad_mfma else ()) + (("wgrad_direct",) if direct else ()) + ("torch.bmm",),
                     asks_mfma, not any(takes and not fits for takes, fits in mfma))


def gemm_wgrad_supported(x3, go3):
    """gemm_wgrad is what a Function that asks the MFMA GEMM (the wx route) takes for this weight gradient."""
    B, Cin, P = x3.shape
    return "gemm_wgrad" in train_plan("wx", B, Cin, go3.shape[1], P, cuda=x3.is_cuda and x3.dtype == torch.float32).wgrad


def wgrad_direct_supported(x3, go3, bias=False):
    """Small-channel, many-pixel products in rows wgrad_direct can read (the shape rule and its measurements: train_plan)."""
    B, Cin, P = x3.shape
    plan = train_plan("conv1x1_train_w", B, Cin, go3.shape[1], P, cuda=x3.is_cuda and x3.dtype == go3.dtype == torch.float32, bias_grad=bias)
    return "wgrad_direct" in plan.wgrad and _rows_ok(x3) and _rows_ok(go3)


def _train_fwd(plan, x3, w2, bias=None, out=None):
    """W . x3 (+ bias) on plan.fwd, into `out` f32[B,Cout,n] where given."""
    if plan.fwd == "gemm_bf16x3":
        assert bias is None and out is None                    # (only _WxTrain asks this engine: its bias is added outside)
        return gemm_bf16x3(x3, gemm_pack_weight(w2), w2.shape[0])
    if plan.fwd == "pointwise":                                # the module's [Cout, Cin] weight read in place, the bias in the epilogue
        return pointwise([x3], w2, None, bias, ACT_NONE, 0.0, out=out, w_rowmajor=True)
    y = torch.bmm(w2.unsqueeze(0).expand(x3.shape[0], -1, -1), x3, out=out)
    if bias is not None:
        y += bias.view(1, -1, 1)
    return y


def _train_dgrad(plan, go3, w2):
    """W^T . go3 on plan.dgrad -> f32[B,Cin,n]."""
    if plan.dgrad == "gemm_bf16x3":
        return gemm_bf16x3(go3, conv_pack_weight_dgrad(w2), w2.shape[1])
    if plan.dgrad == "pointwise":
        return pointwise([go3.contiguous()], w2)                # the same weight read as [K = Cout][Cin]
    return torch.bmm(w2.t().unsqueeze(0).expand(go3.shape[0], -1, -1), go3)


def _train_wgrad(plan, x3, go3, bias_grad=False):
    """(sum_b go3[b] . x3[b]^T, db or None) on the first engine of plan.wgrad whose run-time condition holds; db only from wgrad_direct."""
    for engine in plan.wgrad:
        if engine == "gemm_wgrad":
            return gemm_wgrad(x3, go3), None
        if engine == "wgrad_direct" and _rows_ok(x3) and _rows_ok(go3):
            return wgrad_direct(x3, go3, bias=bias_grad)
    return torch.bmm(go3, x3.transpose(1, 2)).sum(0), None        # [B, Cout, Cin] partials: <= 25 MB for every layer but one


class _WxTrain(torch.autograd.Function):
    """y[b] = W . x[b] under autograd, every product offered to the split-bf16 MFMA GEMM first (train_plan; >= 2 GFLOP: the tap GEMMs of
    PSPUpsample, the PSP bottleneck, the 512 / 1024-channel fusion convolutions).  No bias: a caller adds it outside, and its gradient
    is autograd's own sum."""

    @staticmethod
    def forward(ctx, x3, w2):
        ctx.save_for_backward(x3, w2)
        ctx.plan = train_plan("wx", x3.shape[0], x3.shape[1], w2.shape[0], x3.shape[2], cuda=x3.is_cuda and x3.dtype == torch.float32)
        return _train_fwd(ctx.plan, x3, w2)

    @staticmethod
    def backward(ctx, go):
        x3, w2 = ctx.saved_tensors
        go = go.contiguous()
        gx = _train_dgrad(ctx.plan, go, w2) if ctx.needs_input_grad[0] else None
        gw = _train_wgrad(ctx.plan, x3, go)[0] if ctx.needs_input_grad[1] else None
        return gx, gw


class _Conv1x1Train(torch.autograd.Function):
    """y[b] = W . x[b] (+ bias) for a 1x1 convolution, with all three products as batched GEMMs on the NCHW tensors as they lie and none
    of them on the split-bf16 MFMA GEMM (train_plan, asks_mfma).  torch's convolution backward sends a 1x1 convolution to MIOpen's
    implicit-GEMM wgrad / bwd-data kernels, which want NHWC and pay a transposing copy of every operand (181 `batched_transpose`
    launches, 2.7 ms of a 56 ms training step) around fp32 kernels slower than the GEMM library's."""

    @staticmethod
    def forward(ctx, x, w2, bias):
        B, Cin = x.shape[0], x.shape[1]
        x3 = x.reshape(B, Cin, -1)
        ctx.save_for_backward(x3, w2)
        ctx.xshape = x.shape
        ctx.bias_grad = bias is not None and ctx.needs_input_grad[2]
        ctx.plan = train_plan("conv1x1_train_w", B, Cin, w2.shape[0], x3.shape[2], x.is_cuda and x.dtype == torch.float32, ctx.bias_grad)
        y = torch.empty((B, w2.shape[0]) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)   # returned as it is (not a view: the
        _train_fwd(ctx.plan, x3, w2, bias, out=y.view(B, w2.shape[0], -1))                          # modules' in-place activations follow)
        return y

    @staticmethod
    def backward(ctx, go):
        x3, w2 = ctx.saved_tensors
        go3 = go.reshape(x3.shape[0], w2.shape[0], -1)
        gx = _train_dgrad(ctx.plan, go3, w2).view(ctx.xshape) if ctx.needs_input_grad[0] else None
        gw, gb = _train_wgrad(ctx.plan, x3, go3, ctx.bias_grad) if ctx.needs_input_grad[1] else (None, None)
        if ctx.bias_grad and gb is None:
            gb = go3.sum((0, 2))
        return gx, gw, gb


def conv1x1_train_supported(conv, x):
    """Past the operand limit of the split-bf16 GEMM (train_plan's fits; the backward's operands count too) the module runs its torch path."""
    return (settings.USE_GEMM_CONV1X1_TRAIN and x.is_cuda and x.dtype == torch.float32 and all(k == 1 for k in conv.kernel_size)
            and all(st == 1 for st in conv.stride) and all(p == 0 for p in conv.padding) and conv.groups == 1 and x.dim() in (3, 4)
            and train_plan("conv1x1_train", x.shape[0], x.shape[1], conv.weight.shape[0], x.numel() // max(1, x.shape[0] * x.shape[1])).fits)


def conv1x1_train(conv, x):
    """Differentiable 1x1 convolution of an nn.Conv1d / nn.Conv2d module.  Where the split-bf16 MFMA GEMM takes the forward or the input
    gradient (train_plan) the layer goes through _WxTrain with the bias added here; every other layer through _Conv1x1Train."""
    w = conv.weight
    B, Cin, Cout = x.shape[0], x.shape[1], w.shape[0]
    n = x.numel() // (B * Cin)
    if train_plan("conv1x1_train", B, Cin, Cout, n, cuda=x.is_cuda and x.dtype == torch.float32).function == "_WxTrain":
        y = _WxTrain.apply(x.reshape(B, Cin, n).contiguous(), w.reshape(Cout, Cin).contiguous())
        if conv.bias is not None:
            y = y + conv.bias.view(1, -1, 1)
        return y.view(B, Cout, *x.shape[2:])
    return _Conv1x1Train.apply(x.contiguous(), w.reshape(Cout, Cin), conv.bias)


def conv1x1_train_w(x, w2, bias=None):
    """`conv1x1_train` for a weight TENSOR f32[Cout,Cin] (a slice of a module's weight, say) instead of a module: x f32[B,Cin,n].
    Always _Conv1x1Train."""
    return _Conv1x1Train.apply(x.contiguous(), w2, bias)


class _PointwisePmTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return pointwise([x], w.t().contiguous(), point_major=True)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        gx = torch.matmul(g, w).transpose(1, 2).contiguous() if ctx.needs_input_grad[0] else None      # [B,n,C] -> [B,C,n]
        gw = torch.bmm(x, g).sum(0).t() if ctx.needs_input_grad[1] else None                           # sum_b x[b] g[b] = [C,Cout]
        return gx, gw


def pointwise_pm_train(x, w):
    """Differentiable per-point layer with a POINT-MAJOR result: x f32[B,C,n], w f32[Cout,C] -> f32[B,n,Cout] = (W x)^T, the forward on
    the exact-fp32 MFMA kernel of `pointwise`, the two gradient products (2 B n C Cout flops each) as batched GEMMs."""
    return _PointwisePmTrain.apply(_dev(x, torch.float32, "x"), w)


def upconv_train_supported(B, cout):
    return B * 9 * cout <= 65535


def psp_combine(g, ys, bias, packed=False):
    """out = relu(g + bias + sum_k bilinear_up(ys[k])); g f32[B,C,H,W], ys four f32[B,C,s,s].  Inference only, in place on g.
    packed: the kernel also writes the packed split-bf16 operand of the GEMMs that read the map next (hung on the result as
    `_gdm_packed`, see gemm_bf16x3_map) -- no pack launch in front of them."""
    g = _dev(g, torch.float32, "g")
    B, C, H, W = g.shape
    ys = [_dev(y, torch.float32, "y") for y in ys]
    assert len(ys) == 4
    opk = _packed_out(B, C, H, W, g.device) if packed and packed_out_supported(B, C, H, W, grid_groups=True) else None   # (blockIdx.y = group)
    call("gdm_psp_combine2_hip", g, ys[0], ys[0].shape[2], ys[1], ys[1].shape[2], ys[2], ys[2].shape[2], ys[3], ys[3].shape[2], bias, B, C,
         H, W, g, opk.buf if opk is not None else None)
    return carry_packed(g, opk)


def packed_out_supported(B, C, H, W, row=32, grid_groups=False):
    """The shapes for which a producer (gather_add_affine_act with the defaults) writes the packed operand of its [B,C,H,W] map: a
    channel count of the format, whole 256-pixel workgroup tiles of the reader, image rows in whole runs of `row` pixels (32: the
    reader may be the 1x1 GEMM, gemm_bf16x3_map; 16: a 3x3 convolution, whose 16-pixel operand fragment lies inside one image row).
    grid_groups: the producer launches one grid row per (image, 8-channel group), which must fit a grid dimension."""
    return (C == 64 or C % 128 == 0) and W % row == 0 and (B * H * W) % 256 == 0 and (not grid_groups or B * C // 8 <= 65535)


def gather_add_affine_act(x, t, idx, scale, shift, act=ACT_NONE, slope=0.0, hw=None, f32_out=True):
    """y[b,c,j] = act(scale[c]*(x[b,c,j] + t[b,c,idx[b,j]]) + shift[c]); x f32[B,C,m], t f32[B,C,n], idx int[B,m(,1)].
    Inference only, in place on x.  With hw = (H, W) of the pixel map (m = H*W) the kernel also writes the packed split-bf16 operand
    of the next convolution / GEMM over it; the caller hangs the returned PackedAct on the map it hands on (`_gdm_packed`).
    f32_out=False (needs hw and packed_out_supported): the PackedAct is the only output and the only return value -- no fp32 store,
    x is left as it was -- for a map whose only reader is a GEMM on the packed operand.
    x may be a GemmMap (the 1x1 GEMM that would produce x, not yet run): the whole call is then that GEMM with this tail as its
    epilogue, conv1x1_packed_gather_add_act -- one launch, same bits, x never stored."""
    if isinstance(x, GemmMap):
        if hw is None:
            raise ValueError("gather_add_affine_act: a GemmMap needs hw")
        return conv1x1_packed_gather_add_act(x.x, x.wpk, x.cout, t, idx, scale, shift, act, hw=hw, f32_out=f32_out)
    x = _dev(x, torch.float32, "x")
    t = _dev(t, torch.float32, "t")
    idx = _idx32(idx, "idx")
    B, C, m = x.shape
    n = t.shape[2]
    opk = _packed_out(B, C, hw[0], hw[1], x.device) if hw is not None and hw[0] * hw[1] == m and packed_out_supported(B, C, hw[0], hw[1]) else None
    if not f32_out and opk is None:
        raise ValueError("gather_add_affine_act: f32_out=False needs a map the packed operand is built for, got x %s hw %s" % (tuple(x.shape), hw))
    call("gdm_gather_add_affine_act2_hip", x, t, idx, scale, shift, B, C, n, m, act, float(slope), x if f32_out else None,
         opk.buf if opk is not None else None, hw[1] if opk is not None else 0)
    if not f32_out:
        return opk
    return (x, opk) if hw is not None else x


def lfa_stage(xyz, idx, feat, w1t, s1, b1, w2t, s2, b2, wft, wmt, sm, bm, slope=0.2):
    """One attentive-pooling stage of RandLA's local feature aggregation in one launch (see include/gdm.h gdm_lfa_stage_hip).
    xyz f32[B,n,3], idx int[B,n,16], feat f32[B,D/2,n(,1)] -> f32[B,OUT,n].  Inference only."""
    xyz = _dev(xyz, torch.float32, "xyz")
    feat = _dev(feat, torch.float32, "feat")
    idx = _idx32(idx, "idx")
    B, n, K = idx.shape
    H = feat.shape[1]
    D, OUT = 2 * H, wmt.shape[1]
    out = torch.empty((B, OUT, n), dtype=torch.float32, device=feat.device)
    if w2t is None:
        s2 = b2 = None
    call("gdm_lfa_stage_hip", xyz, idx, feat, w1t, s1, b1, w2t, s2, b2, wft, wmt, sm, bm, B, n, K, D, OUT, float(slope), out)
    return out


def lfa_supported(d_out, K):
    return K == 16 and d_out in (32, 64, 128, 256)


def conv64_gather_add_act_mfma(x, wpk, t, idx, scale, shift, act=ACT_NONE, slope=0.0, pixel_major=False, t_point_major=False, hw=None):
    """conv1x1_gather_add_act with the 64 x 64 channel mix on split-bf16 MFMA: wpk = pack_rows64(W[64,64]) (row = output channel).
    t f32[B,64,n], or f32[B,n,64] with t_point_major (the gathered term is then one contiguous row per pixel).  Inference only.
    hw = (H, W) of the pixel map (NCHW form): the kernel also writes the packed operand of the next convolution (`_gdm_packed`)."""
    x = _dev(x, torch.float32, "x")
    t = _dev(t, torch.float32, "t")
    idx = _idx32(idx, "idx")
    B, C, m = x.shape
    n = t.shape[1] if t_point_major else t.shape[2]
    if t_point_major and t.data_ptr() % 16:
        t = t.clone()                                # the kernel reads a point's row four channels at a time
    if C != 64 or t.shape[2 if t_point_major else 1] != 64 or wpk.numel() != 64 * 256:
        raise ValueError("conv64_gather_add_act_mfma: built for 64 -> 64 channels, got x %s t %s" % (tuple(x.shape), tuple(t.shape)))
    y = torch.empty((B, m, C), dtype=torch.float32, device=x.device) if pixel_major else torch.empty_like(x)
    want = hw is not None and not pixel_major and hw[0] * hw[1] == m and packed_out_supported(B, C, hw[0], hw[1])
    opk = _packed_out(B, C, hw[0], hw[1], x.device) if want else None
    call("gdm_conv64_gather_add_act_mfma2_hip", x, wpk, t, idx, scale, shift, B, n, m, act, float(slope), int(bool(pixel_major)),
         int(bool(t_point_major)), y, opk.buf if opk is not None else None, int(hw[1]) if opk is not None else 0)
    return carry_packed(y, opk)


def conv1x1_gather_add_act(x, wt, t, idx, scale, shift, act=ACT_NONE, slope=0.0, pixel_major=False):
    """y[b,co,j] = act(scale[co]*(sum_ci W[co,ci] x[b,ci,j] + t[b,co,idx[b,j]]) + shift[co]) in one pass for the 64-channel fusion
    levels.  x f32[B,64,m], wt f32[64,64] = W transposed (contiguous), t f32[B,64,n], idx int[B,m(,1)].  Inference only.
    pixel_major: y comes back as f32[B,m,64] (a 256-byte row per pixel: what upconv_final_points reads)."""
    x = _dev(x, torch.float32, "x")
    t = _dev(t, torch.float32, "t")
    wt = _dev(wt, torch.float32, "wt")
    idx = _idx32(idx, "idx")
    B, C, m = x.shape
    if C != 64 or tuple(wt.shape) != (64, 64) or t.shape[1] != 64:
        raise ValueError("conv1x1_gather_add_act: built for 64 -> 64 channels, got x %s wt %s t %s" % (tuple(x.shape), tuple(wt.shape), tuple(t.shape)))
    y = torch.empty((B, m, C), dtype=torch.float32, device=x.device) if pixel_major else torch.empty_like(x)
    call("gdm_conv1x1_gather_add_act2_hip", x, wt, t, idx, scale, shift, B, C, t.shape[2], m, act, float(slope), int(bool(pixel_major)), y)
    return y


def heads_rows_buffer(R, device):
    """u8[R * 512]: where point_heads(rows=True) writes the matching rows of R points.  It belongs to the current BufferPool (one per
    row count), so a captured step allocates nothing for it; its contents hold until the next point_heads(rows=True) of the same
    pool and row count."""
    nbytes = _lib.lib().gdm_match_rows_bytes(R)
    if _capturing_unscoped():
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    key = ("heads_rows", device.index, R)
    buf = _pool.workspace.get(key)
    if buf is None:
        buf = _pool.workspace[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return buf


def point_heads(a, b, layers, last, feat_layer, res_layer, residual=None, rows=False):
    """The per-point 1x1-convolution chain of GeoMatch.forward in one launch (inference).  a f32[B,Ca,N] (+ b f32[B,128-Ca,N] or None);
    layers = [(wpk, scale|None, shift|None, act)] of 128 -> 128 layers (wpk from gemm_pack_weight, act ACT_NONE / ACT_RELU);
    last = (wpk, bias|None, c_last) or None (the chain ends with its hidden layers).  residual = (ra, rb|None): the tensor added at
    res_layer (default: the input).  -> (out_feat f32[B,128,N] = output of layer feat_layer or None, out_last f32[B,c_last,N] or None).
    rows=True (with feat_layer >= 0): the kernel also writes the matching rows of out_feat, the bytes match_pack(out_feat, MATCH_BF16X3)
    would (gdm_point_heads3_hip), into heads_rows_buffer(B * N) -> (out_feat, out_last, rows u8[B*N*512])."""
    import ctypes
    a = _dev(a, torch.float32, "a")
    B, Ca, N = a.shape
    if b is not None:
        b = _dev(b, torch.float32, "b")
        if b.shape[0] != B or b.shape[2] != N or b.shape[1] + Ca != 128:
            raise ValueError("point_heads: a %s + b %s must make 128 channels" % (tuple(a.shape), tuple(b.shape)))
    elif Ca != 128:
        raise ValueError("point_heads: a must have 128 channels when b is None, got %d" % Ca)
    n = len(layers)
    vp, fp = ctypes.c_void_p, ctypes.c_void_p
    w_arr = (vp * n)(*[l[0].data_ptr() for l in layers])
    sc_arr = (fp * n)(*[(l[1].data_ptr() if l[1] is not None else None) for l in layers])
    sh_arr = (fp * n)(*[(l[2].data_ptr() if l[2] is not None else None) for l in layers])
    act_arr = (ctypes.c_int * n)(*[int(l[3]) for l in layers])
    for l in layers:
        if l[3] not in (ACT_NONE, ACT_RELU):
            raise ValueError("point_heads: activations are none / ReLU")
    wl, bl, c_last = last if last is not None else (None, None, 0)
    out_feat = torch.empty((B, 128, N), dtype=torch.float32, device=a.device) if feat_layer >= 0 else None
    out_last = torch.empty((B, int(c_last), N), dtype=torch.float32, device=a.device) if c_last else None
    ra, rb = (None, None)
    if residual is not None:
        ra = _dev(residual[0], torch.float32, "residual")
        rb = _dev(residual[1], torch.float32, "residual") if residual[1] is not None else None
        if ra.shape[0] != B or ra.shape[2] != N or ra.shape[1] + (rb.shape[1] if rb is not None else 0) != 128:
            raise ValueError("point_heads: the residual source must make 128 channels of the same points")
    if rows:
        if feat_layer < 0:
            raise ValueError("point_heads: rows are the matching rows of out_feat and need feat_layer >= 0")
        out_rows = heads_rows_buffer(B * N, a.device)
        call("gdm_point_heads3_hip", a, b, Ca, ra, rb, ra.shape[1] if ra is not None else 0, B, N, n, w_arr, sc_arr, sh_arr, act_arr,
             int(feat_layer), int(res_layer), wl, bl, int(c_last), out_feat, out_last, out_rows)
        return out_feat, out_last, out_rows
    call("gdm_point_heads2_hip", a, b, Ca, ra, rb, ra.shape[1] if ra is not None else 0, B, N, n, w_arr, sc_arr, sh_arr, act_arr,
         int(feat_layer), int(res_layer), wl, bl, int(c_last), out_feat, out_last)
    return out_feat, out_last


def pack_rows64(w2d):
    """f32[R,64] -> R packed split-bf16 rows of 256 B (64 bf16 hi | 64 bf16 lo), u8 tensor."""
    w = _dev(w2d.detach(), torch.float32, "w")
    if w.dim() != 2 or w.shape[1] != 64:
        raise ValueError("pack_rows64: expected [R,64], got %s" % (tuple(w.shape),))
    out = torch.empty(w.shape[0] * 256, dtype=torch.uint8, device=w.device)
    call("gdm_pack_rows64_hip", w, w.shape[0], out)
    return out


def upconv_final_points(x_pm, hw, choose, wpk, scale, shift, act, slope, wf_pk, fbias, out_size):
    """The last image stage at the sampled pixels (inference): log_softmax(Wf . act(scale * conv3x3(up(x)) + shift) + fbias) at pixel
    choose[b,n] of the out_size map -> f32[B,64,N].  x_pm f32[B,H*W,64] pixel-major, hw = (H, W); wpk from
    upconv_fused64_pack_weight, wf_pk from pack_rows64(final_weight[64,64])."""
    x_pm = _dev(x_pm, torch.float32, "x_pm")
    choose = _idx32(choose, "choose")
    B = x_pm.shape[0]
    H, W = int(hw[0]), int(hw[1])
    if tuple(x_pm.shape) != (B, H * W, 64):
        raise ValueError("upconv_final_points: x_pm must be [B,H*W,64] with (H, W) = %s, got %s" % ((H, W), tuple(x_pm.shape)))
    choose = choose.reshape(B, -1)
    N = choose.shape[1]
    OH, OW = int(out_size[0]), int(out_size[1])
    out = torch.empty((B, 64, N), dtype=torch.float32, device=x_pm.device)
    call("gdm_upconv_final_points_hip", x_pm, choose, wpk, scale, shift, act, float(slope), wf_pk, fbias, B, H, W, OH, OW, N, out)
    return out




def stem_pack_weight(weight):
    """w f32[64,3,7,7] -> fragment-ordered split-bf16 weights of the stem kernel (u8 tensor); cache it per weight version."""
    w = _dev(weight.detach(), torch.float32, "weight")
    if tuple(w.shape) != (64, 3, 7, 7):
        raise ValueError("stem_pack_weight: the stem kernel is built for a [64,3,7,7] filter, got %s" % (tuple(w.shape),))
    L = _lib.lib()
    wpk = torch.empty(L.gdm_stem_weight_bytes(), dtype=torch.uint8, device=w.device)
    call("gdm_stem_pack_weight_hip", w, wpk)
    return wpk


def stem(x, wpk, scale, shift, packed=True):
    """maxpool3x3/2(relu(scale * conv7x7/2(x) + shift)) in one launch (include/gdm.h gdm_stem_hip).  x f32[B,3,H,W] ->
    f32[B,64,PH,PW]; with `packed` the result also carries (`_gdm_packed`) the split-bf16 operand of the next 3x3 convolution."""
    x = _dev(x, torch.float32, "x")
    B, C, H, W = x.shape
    if C != 3:
        raise ValueError("stem: 3 input channels, got %d" % C)
    PH, PW = ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1
    out = torch.empty((B, 64, PH, PW), dtype=torch.float32, device=x.device)
    opk = _packed_out(B, 64, PH, PW, x.device) if packed and packed_out_supported(B, 64, PH, PW, row=16) else None   # (read by a 3x3 convolution)
    call("gdm_stem_hip", x, wpk, scale, shift, B, H, W, out, opk.buf if opk is not None else None)
    return carry_packed(out, opk)


def affine_relu_maxpool(x, scale, shift):
    """MaxPool2d(3, 2, 1)(relu(scale[c] * x + shift[c])) in one pass (the ResNet stem behind conv1).  Inference only."""
    x = _dev(x, torch.float32, "x")
    B, C, H, W = x.shape
    y = torch.empty((B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
    call("gdm_affine_relu_maxpool_hip", x, scale, shift, B, C, H, W, y)
    return y


def _final_weight_t(weight):
    """W^T of the 64 -> 64 `final` weight (the kernels read 64 contiguous scalars per ci), cached ON the weight tensor: it lives and
    dies with it.  (A module-level dict keyed by id(weight) served a NEW tensor that got a dead one's id, address and version the old
    one's transpose: wrong output, found by a test that builds several weights in a row.)"""
    C = weight.shape[0]
    return derived(weight, "final_wt", (weight,), lambda: weight.reshape(C, C).t().contiguous())


def conv1x1_logsoftmax(x, weight, bias):
    """log_softmax over channels of a 64->64 1x1 convolution, one pass (the `final` stage, pspnet.py:108-112). Inference only."""
    x = _dev(x, torch.float32, "x")
    B, C, H, W = x.shape
    w = _final_weight_t(weight)
    out = torch.empty_like(x)
    call("gdm_conv1x1_logsoftmax_hip", x, w, bias, B, C, H * W, out)
    return out


def conv64_gather_add_final(x, wpk, t, idx, scale, shift, act, slope, final_weight, final_bias):
    """conv1x1_logsoftmax(conv64_gather_add_act_mfma(x, wpk, t, idx, scale, shift, act, slope, t_point_major=True), final_weight,
    final_bias) in one launch, bit for bit, without the fused map between the two (nobody else reads it).  x f32[B,64,m],
    t f32[B,n,64] point-major, final_weight [64,64(,1,1)] -> f32[B,64,m].  Inference only."""
    x = _dev(x, torch.float32, "x")
    t = _dev(t, torch.float32, "t")
    idx = _idx32(idx, "idx")
    B, C, m = x.shape
    if C != 64 or t.dim() != 3 or t.shape[2] != 64 or wpk.numel() != 64 * 256 or final_weight.numel() != 64 * 64:
        raise ValueError("conv64_gather_add_final: built for 64 -> 64 -> 64 channels, got x %s t %s final %s"
                         % (tuple(x.shape), tuple(t.shape), tuple(final_weight.shape)))
    wft = _final_weight_t(final_weight)
    if t.data_ptr() % 16:
        t = t.clone()                                # the kernel reads a point's row four channels at a time
    out = torch.empty_like(x)
    call("gdm_conv64_gather_add_final_hip", x, wpk, t, idx, scale, shift, B, t.shape[1], m, act, float(slope), wft, final_bias, out)
    return out


def channel_sum(t):
    """t f32[B,C,...] -> f32[C] sums over batch and inner dimensions (bias gradients): the streaming reduction of the BatchNorm kernels
    (accumulated in double) where its shape rules hold -- torch's generic reduce_kernel moves these maps at 0.7 TB/s."""
    B, C = t.shape[0], t.shape[1]
    inner = t.numel() // max(B * C, 1)
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and B * C <= 65535 and inner >= 4 and inner % 4 == 0
            and t.data_ptr() % 16 == 0):
        return t.sum(dim=[0] + list(range(2, t.dim())))
    L = _lib.lib()
    sums = torch.empty(L.gdm_bn_sums_len(B, C, inner), dtype=torch.float64, device=t.device)
    call("gdm_bn_stats_hip", t, B, C, inner, sums)
    return sums[:-2].view(-1, C, 2)[:, :, 0].sum(0).float()


class _PspPools(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _dev(x, torch.float32, "x")
        B, C, H, W = x.shape
        outs = [torch.empty((B, C, s_, s_), dtype=torch.float32, device=x.device) for s_ in (1, 2, 3, 6)]
        call("gdm_psp_pools_hip", x, B * C, H, W, outs[0], outs[1], outs[2], outs[3])
        ctx.shape = (B, C, H, W)
        return tuple(outs)

    @staticmethod
    def backward(ctx, g1, g2, g3, g6):
        B, C, H, W = ctx.shape
        gs = [_dev(g, torch.float32, "grad") for g in (g1, g2, g3, g6)]
        gx = torch.empty((B, C, H, W), dtype=torch.float32, device=gs[0].device)
        call("gdm_psp_pools_bwd_hip", gs[0], gs[1], gs[2], gs[3], B * C, H, W, gx)
        return gx


def psp_pools_supported(h, w):
    return 36 <= h * w <= 4096 and h >= 6 and w >= 6


def psp_pools(x):
    """Adaptive average pools to 1,2,3,6 bins in one pass: x f32[B,C,H,W] -> four f32[B,C,s,s] (differentiable)."""
    return list(_PspPools.apply(x))


class _PspCombine(torch.autograd.Function):
    """out = relu(g + bias + sum_k bilinear_up(ys[k])) with its backward: the training form of psp_combine."""

    @staticmethod
    def forward(ctx, g, bias, y1, y2, y3, y4):
        g = _dev(g, torch.float32, "g")
        ys = [_dev(y, torch.float32, "y") for y in (y1, y2, y3, y4)]
        B, C, H, W = g.shape
        out = torch.empty_like(g)
        call("gdm_psp_combine2_hip", g, ys[0], ys[0].shape[2], ys[1], ys[1].shape[2], ys[2], ys[2].shape[2], ys[3], ys[3].shape[2], bias,
             B, C, H, W, out, None)
        ctx.save_for_backward(out)
        ctx.sizes = [y.shape[2] for y in ys]
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, go):
        (out,) = ctx.saved_tensors
        B, C, H, W = out.shape
        gpre = torch.where(out > 0, go, torch.zeros((), dtype=go.dtype, device=go.device)).contiguous()
        gys = []
        for s_ in ctx.sizes:
            gy = torch.empty((B, C, s_, s_), dtype=torch.float32, device=go.device)
            call("gdm_upsample_bilinear_bwd_hip", gpre, B * C, s_, s_, H, W, gy)
            gys.append(gy)
        gb = channel_sum(gpre) if ctx.has_bias else None
        return gpre, gb, gys[0], gys[1], gys[2], gys[3]


def psp_combine_train(g, ys, bias):
    """Differentiable psp_combine (not in place): relu(g + bias + sum_k bilinear_up(ys[k]))."""
    assert len(ys) == 4
    return _PspCombine.apply(g, bias, ys[0], ys[1], ys[2], ys[3])


class BufferPool:
    """Owner-held scratch buffers of the split-bf16 kernels (zero-bordered packed activation maps, matching workspaces).  Whoever
    captures a step in a hipGraph owns one (infer.GraphedPipeline, train_graph.GraphedTrainStep, bench.py's step) and enters it
    with `ops.buffer_pool(pool)` around warm-up, capture and any later eager call of the same step: the buffers -- and the zero
    fill of their borders, captured once per buffer -- then belong to that graph's private memory pool and to nothing else.
    Eager code outside any scope uses the process-wide default pool."""

    def __init__(self):
        self.packed = {}
        self.workspace = {}


_default_pool = BufferPool()
_pool = _default_pool
_warned_capture = []


class buffer_pool:
    def __init__(self, pool):
        self.pool, self.prev = pool, None

    def __enter__(self):
        global _pool
        self.prev, _pool = _pool, self.pool
        return self.pool

    def __exit__(self, *exc):
        global _pool
        _pool = self.prev
        return False


def _capturing_unscoped():
    """A hipGraph capture that runs outside any buffer_pool scope: its scratch buffers must not enter (or come from) the
    process-wide pool -- they would live in this graph's private memory pool, and a later capture of the same shape would
    silently write into them -- so they are allocated per call (each zero fill is then replayed with the graph: slower, correct)."""
    if _pool is _default_pool and torch.cuda.is_current_stream_capturing():
        if not _warned_capture:
            _warned_capture.append(1)
            import warnings
            warnings.warn("geometric_aware_dense_matching_amd.ops: hipGraph capture outside ops.buffer_pool(...): scratch buffers "
                          "are allocated per call inside the graph; give the capture a BufferPool of its own")
        return True
    return False


def conv3x3_wgrad_supported(x, go):
    """The split-bf16 MFMA weight-gradient path: 32- or 64-wide maps, Cin a multiple of 256 (the per-part weights of the GEMM want
    whole 256-row tiles per part) -- the 32 x 32 half of the trunk, where torch's path (MIOpen fp32 implicit GEMM) is 2.5x slower."""
    B, Cin, H, W = x.shape
    return (settings.USE_MFMA_WGRAD and x.is_cuda and x.dtype == torch.float32 and go.shape[0] == B and tuple(go.shape[2:]) == (H, W)
            and W in (32, 64) and (H * W) % 128 == 0 and Cin % 256 == 0 and go.shape[1] % 8 == 0
            and operands_fit(_lib.lib().gdm_wgrad_x_bytes(B, Cin, H, W), _lib.lib().gdm_wgrad_go_bytes(B, go.shape[1], H, W)))


def conv3x3_wgrad(x, go, parts=None):
    """dW f32[Cout,Cin,3,3] of a 3x3 / stride 1 / pad 1 convolution from its input x f32[B,Cin,H,W] and output gradient go
    f32[B,Cout,H,W], on the split-bf16 MFMA GEMM (include/gdm.h gdm_wgrad_*): the contraction runs over the B*H*W pixels, split
    into `parts` equal parts (one launch, _wgrad_packed), whose [Cout,9,Cin] partial products are added in a fixed order."""
    B, Cin, H, W = x.shape
    return _wgrad_packed("conv3x3_wgrad", x, go, 9, parts).view(go.shape[1], 3, 3, Cin).permute(0, 3, 1, 2).contiguous()


def conv3x3_supported(x, weight, stride=(1, 1), padding=(1, 1), dilation=(1, 1)):
    """3x3 / pad 1 / no dilation, stride 1 or 2 (output width a multiple of 32), Cin 64 or a multiple of 128, both packed operands
    below 2 GiB (operands_fit)."""
    cin = weight.shape[1]
    st = tuple(stride)
    if st not in ((1, 1), (2, 2)):
        return False
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and tuple(weight.shape[2:]) == (3, 3)
            and tuple(padding) == (1, 1) and tuple(dilation) == (1, 1)
            and x.shape[2] % st[0] == 0 and x.shape[3] % st[1] == 0 and (x.shape[3] // st[1]) % 32 == 0
            and (cin == 64 or cin % 128 == 0) and weight.shape[0] % 8 == 0 and x.shape[0] <= 65535
            and operands_fit(_map_bytes(x.shape[0], cin, x.shape[2], x.shape[3]), _lib.lib().gdm_conv3x3_weight_bytes(weight.shape[0], cin)))


def conv3x3_train_supported(x, weight):
    """conv3x3_train(x, weight): conv3x3_supported at stride 1, and the backward's launch too -- the input gradient is the same convolution
    of grad_out f32[B,Cout,H,W] with the flipped, transposed filter, whose operands can be over the limit when the forward's are not."""
    cout, cin = weight.shape[0], weight.shape[1]
    return (conv3x3_supported(x, weight)
            and operands_fit(_map_bytes(x.shape[0], cout, x.shape[2], x.shape[3]), _lib.lib().gdm_conv3x3_weight_bytes(cin, cout)))


def conv_pack_weight_dgrad(weight):
    """The packed weights of the input-gradient convolution of a 3x3/s1/p1 (w f32[Cout,Cin,3,3]) or 1x1 (w f32[Cout,Cin]) layer, straight
    from the forward weight: one launch instead of flip + transpose + contiguous + pack (include/gdm.h gdm_conv_pack_weight_dgrad_hip)."""
    weight = _dev(weight.detach(), torch.float32, "weight")
    Cout, Cin = weight.shape[0], weight.shape[1]
    taps = 9 if weight.dim() == 4 else 1
    L = _lib.lib()
    nbytes = L.gdm_conv3x3_weight_bytes(Cin, Cout) if taps == 9 else L.gdm_conv1x1_weight_bytes(Cin, Cout)
    wpk = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    call("gdm_conv_pack_weight_dgrad_hip", weight, Cout, Cin, taps, wpk)
    return wpk


def conv3x3_pack_weight(weight):
    """w f32[Cout,Cin,3,3] -> packed split-bf16 rows (u8 tensor); cache it per weight version."""
    weight = _dev(weight.detach(), torch.float32, "weight")
    Cout, Cin = weight.shape[0], weight.shape[1]
    L = _lib.lib()
    wpk = torch.empty(L.gdm_conv3x3_weight_bytes(Cout, Cin), dtype=torch.uint8, device=weight.device)
    call("gdm_conv3x3_pack_weight_hip", weight, Cout, Cin, wpk)
    return wpk


class PackedAct:
    """An activation map in the convolution kernel's operand layout (bf16 hi / lo planes of 8 channels, one-pixel zero border):
    what conv3x3_bf16x3(..., out_packed=True) hands to the next convolution instead of a pack launch."""
    __slots__ = ("buf", "shape")

    def __init__(self, buf, shape):
        self.buf, self.shape = buf, tuple(shape)


def carry_packed(t, opk):
    """Hangs the packed operand opk (a PackedAct, or None) on the fp32 map t of the same producer, for the next reader (packed_of)."""
    if opk is not None:
        t._gdm_packed = opk
    return t


def packed_of(x, shape=None):
    """The PackedAct that x is, or carries (carry_packed) for a map of its own shape (or `shape`: x is a view of that map); else None."""
    if isinstance(x, PackedAct):
        return x
    xp = getattr(x, "_gdm_packed", None)
    return xp if isinstance(xp, PackedAct) and xp.shape == tuple(x.shape if shape is None else shape) else None


def _packed_out(B, C, H, W, device, avoid=None):
    """A PackedAct of a [B,C,H,W] map for a producer to write: a zero-bordered buffer of the pool (_packed_buffer) and its shape."""
    return PackedAct(_packed_buffer(B, C, H, W, device, avoid=avoid), (B, C, H, W))


def _packed_buffer(B, C, H, W, device, avoid=None):
    """Zero-bordered operand buffer for [B,C,H,W] from the current BufferPool (two per shape and stream: a layer reads one and
    writes the other).  Only interior pixels are ever written, so the border stays zero."""
    nbytes = _lib.lib().gdm_conv3x3_act_bytes(B, C, H, W)
    if _capturing_unscoped():
        return torch.zeros(nbytes, dtype=torch.uint8, device=device)
    key = (B, C, H, W, device.index, _stream_lane(device))
    pool = _pool.packed.setdefault(key, [])
    for buf in pool:
        if avoid is None or buf.data_ptr() != avoid.data_ptr():
            return buf
    buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    pool.append(buf)
    return buf


def conv3x3_pack_act(x):
    """x f32[B,C,H,W] -> PackedAct (one launch)."""
    B, C, H, W = x.shape
    _require_fit("conv3x3_pack_act", "x %s", (tuple(x.shape),), _map_bytes(B, C, H, W))       # (in front of _dev, which may copy x)
    x = _dev(x, torch.float32, "x")
    xp = _packed_out(B, C, H, W, x.device)
    call("gdm_conv3x3_pack_act_hip", x, B, C, H, W, xp.buf)
    return xp


def conv3x3_bf16x3(x, wpk, cout, scale=None, shift=None, act=ACT_NONE, res=None, out_f32=True, out_packed=False, stride=1):
    """3x3/p1 convolution (stride 1 or 2) of x f32[B,Cin,H,W] (or a PackedAct) with packed weights on split-bf16 MFMA (+ per-channel
    scale/shift, optional residual, optional ReLU).  Returns the fp32 map, or -- out_packed -- (fp32 map or None, PackedAct of the
    result): the epilogue writes the next convolution's operand itself.  Inference only."""
    _require_fit("conv3x3_bf16x3", "x %s -> %d channels", (tuple(x.shape), cout), _map_bytes(*x.shape), wpk.numel())
    xp = x if isinstance(x, PackedAct) else conv3x3_pack_act(x)
    B, Cin, H, W = xp.shape
    if stride != 1:
        if stride != 2 or H % 2 or W % 2:
            raise ValueError("conv3x3_bf16x3: stride %r on a %dx%d map" % (stride, H, W))
        H, W = H // 2, W // 2
    dev = xp.buf.device
    out = torch.empty((B, cout, H, W), dtype=torch.float32, device=dev) if out_f32 else None
    opk = None
    if out_packed:
        if (B * H * W) % 256 != 0 or cout % 8 != 0:
            raise ValueError("conv3x3_bf16x3: packed output needs B*H*W %% 256 == 0 and Cout %% 8 == 0")
        opk = _packed_out(B, cout, H, W, dev, avoid=xp.buf)
    if res is not None:
        res = _dev(res, torch.float32, "res")
        if res.data_ptr() % 16:
            res = res.clone()                        # the epilogue reads the residual four pixels at a time
        assert tuple(res.shape) == (B, cout, H, W)
    call("gdm_conv3x3_strided_hip", xp.buf, wpk, scale, shift, res, B, Cin, cout, H, W, int(stride), act, out,
         opk.buf if opk is not None else None)
    return (out, opk) if out_packed else out


def gemm_bf16x3_map(x, wpk, cout):
    """W @ x over the channels of a map x f32[B,Cin,H,W] -> f32[B,cout,H,W] on split-bf16 MFMA.  If x carries the packed operand its
    producer wrote (`_gdm_packed`, the trunk's residual blocks), or is that PackedAct itself, the GEMM reads that and no pack launch
    is needed."""
    B, Cin, H, W = x.shape
    xp = _packed_operand(x)
    if xp is not None:
        return conv1x1_packed2d(xp, wpk, cout)
    if isinstance(x, PackedAct):                     # a map that exists as the packed operand only
        raise ValueError("gemm_bf16x3_map: a packed-only map needs W %% 32 == 0, got %s" % (x.shape,))
    return gemm_bf16x3(x.reshape(B, Cin, H * W), wpk, cout).view(B, cout, H, W)


def _packed_operand(x):
    """The packed operand gemm_bf16x3_map would read for the map x (a PackedAct, or a tensor that carries its producer's `_gdm_packed`),
    or None where it would pack x itself."""
    xp = packed_of(x)
    return xp if xp is not None and xp.shape[3] % 32 == 0 else None


def conv1x1_gather_add_supported(x, cout, act, f32_out=True):
    """True when conv1x1_packed_gather_add_act(x, ...) replaces gemm_bf16x3_map + gather_add_affine_act: the map exists as a packed
    operand, the GEMM is one gemm_supported takes (K in whole 128-channel chunks), the activation is none or ReLU, and the pair would
    give the same outputs -- the packed operand where packed_out_supported, which f32_out=False needs."""
    xp = _packed_operand(x)
    if xp is None or act not in (ACT_NONE, ACT_RELU):
        return False
    B, cin, H, W = xp.shape
    if cin % 128 != 0 or not gemm_shape_supported(cin, cout, H * W) or cout % 8 != 0 or (B * H * W) % 256 != 0:
        return False
    if not operands_fit(_map_bytes(B, cin, H, W), _lib.lib().gdm_conv1x1_weight_bytes(cout, cin)):
        return False
    return bool(f32_out) or packed_out_supported(B, cout, H, W)


class GemmMap:
    """gemm_bf16x3_map(x, wpk, cout) not yet run: what _p2r_fuse hands to gather_add_affine_act in place of the fp32 map where
    conv1x1_gather_add_supported, so that the GEMM and the fusion tail are one launch."""
    __slots__ = ("x", "wpk", "cout", "shape")

    def __init__(self, x, wpk, cout):
        B, _, H, W = x.shape
        self.x, self.wpk, self.cout, self.shape = x, wpk, cout, (B, cout, H * W)


def conv1x1_packed_gather_add_act(x, wpk, cout, t, idx, scale, shift, act=ACT_NONE, hw=None, f32_out=True):
    """act(scale[c] * ((W @ x)[b,c,j] + t[b,c,idx[b,j]]) + shift[c]) in ONE launch: gemm_bf16x3_map(x, wpk, cout) followed by
    gather_add_affine_act(., t, idx, scale, shift, act, hw=hw, f32_out=f32_out), bit for bit, with the gather, the folded BatchNorm and
    the activation in the GEMM's epilogue -- the fp32 map between the two launches is never written.  x: a PackedAct or a map that
    carries one (conv1x1_gather_add_supported); t f32[B,cout,n]; idx int[B,H*W(,1)]; hw = (H, W) of the map.  Returns what
    gather_add_affine_act returns: (y f32[B,cout,H*W], PackedAct or None), or the PackedAct alone with f32_out=False.  Inference only."""
    if not conv1x1_gather_add_supported(x, cout, act, f32_out):
        raise ValueError("conv1x1_packed_gather_add_act: not built for x %s -> %d channels, act %r, f32_out %r"
                         % (tuple(x.shape), cout, act, f32_out))
    xp = _packed_operand(x)
    B, Cin, H, W = xp.shape
    _require_fit("conv1x1_packed_gather_add_act", "x %s -> %d channels", (xp.shape, cout), _map_bytes(B, Cin, H, W), wpk.numel())
    if hw is not None and tuple(hw) != (H, W):
        raise ValueError("conv1x1_packed_gather_add_act: hw %s of a %dx%d map" % (tuple(hw), H, W))
    t = _dev(t, torch.float32, "t")
    idx = _idx32(idx, "idx")
    if tuple(t.shape[:2]) != (B, cout) or idx.numel() != B * H * W:
        raise ValueError("conv1x1_packed_gather_add_act: t %s idx %s for a [%d,%d,%d,%d] result" % (tuple(t.shape), tuple(idx.shape), B, cout, H, W))
    if idx.data_ptr() % 16:
        idx = idx.clone()                            # the epilogue loads four indices at once
    dev = xp.buf.device
    y = torch.empty((B, cout, H * W), dtype=torch.float32, device=dev) if f32_out else None
    opk = _packed_out(B, cout, H, W, dev, avoid=xp.buf) if packed_out_supported(B, cout, H, W) else None
    call("gdm_conv1x1_gather_add_hip", xp.buf, wpk, idx, t, t.shape[2], scale, shift, B, Cin, cout, H, W, act, y,
         opk.buf if opk is not None else None)
    return (y, opk) if f32_out else opk


def conv1x1_packed2d(xp, wpk, cout, scale=None, shift=None, act=ACT_NONE, stride=1):
    """1x1 convolution (stride 1 or 2) of a PackedAct map with gemm_pack_weight'ed weights -> f32[B,cout,H/stride,W/stride]: the
    downsample branch of a residual block on the packed operand its 3x3 convolution already reads.  Inference only."""
    B, Cin, H, W = xp.shape
    _require_fit("conv1x1_packed2d", "x %s -> %d channels", (xp.shape, cout), _map_bytes(B, Cin, H, W), wpk.numel())
    if stride not in (1, 2) or H % stride or W % stride:
        raise ValueError("conv1x1_packed2d: stride %r on a %dx%d map" % (stride, H, W))
    H, W = H // stride, W // stride
    out = torch.empty((B, cout, H, W), dtype=torch.float32, device=xp.buf.device)
    call("gdm_conv1x1_strided_hip", xp.buf, wpk, scale, shift, B, Cin, cout, H, W, int(stride), act, out)
    return out


class _Conv3x3Train(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        return conv3x3_bf16x3(x, conv3x3_pack_weight(weight), weight.shape[0])

    @staticmethod
    def backward(ctx, go):
        x, weight = ctx.saved_tensors
        go = _dev(go, torch.float32, "grad")
        gx = gw = None
        if ctx.needs_input_grad[0]:
            # dgrad of a 3x3/s1/p1 convolution = the same convolution of grad_out with the flipped, transposed filter
            gx = conv3x3_bf16x3(go, conv_pack_weight_dgrad(weight), weight.shape[1])
        if ctx.needs_input_grad[1]:
            if conv3x3_wgrad_supported(x, go):
                gw = conv3x3_wgrad(x, go)
            else:
                gw = torch.ops.aten.convolution_backward(go, x, weight, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])[1]
        return gx, gw


def conv3x3_train(x, weight):
    """Differentiable 3x3/s1/p1 convolution without bias: forward and input gradient on the split-bf16 MFMA kernel (same error bound as
    the inference kernel, ~1e-5 relative), weight gradient on MIOpen.  Shapes as conv3x3_supported."""
    return _Conv3x3Train.apply(x, weight)


def gemm_shape_supported(cin, cout, npix):
    """K in whole 128-channel chunks (or exactly 64); output channels are padded to 128 inside the kernel (zero weight rows, masked stores), which
    pays once the padding wastes at most a third of the MFMA work."""
    return (cin % 128 == 0 or cin == 64) and (cout % 128 == 0 or cout >= 192) and npix % 32 == 0


def gemm_supported(cin, cout, npix, batch):
    """gemm_bf16x3 on x f32[batch,cin,npix] -> cout channels: a shape the kernel takes (gemm_shape_supported) whose packed operands
    stay below 2 GiB (operands_fit).  The activations count as gemm_bf16x3 packs them, a map of one row per image: three rows of
    npix + 2 with the zero border, which is also an upper bound for the same pixels packed as a two-dimensional map."""
    return (gemm_shape_supported(cin, cout, npix)
            and operands_fit(_map_bytes(batch, cin, 1, npix), _lib.lib().gdm_conv1x1_weight_bytes(cout, cin)))


def gemm_pack_weight(weight2d):
    """W f32[Cout,Cin] -> packed split-bf16 rows for gemm_bf16x3."""
    w = _dev(weight2d.detach(), torch.float32, "weight")
    Cout, Cin = w.shape
    L = _lib.lib()
    wpk = torch.empty(L.gdm_conv1x1_weight_bytes(Cout, Cin), dtype=torch.uint8, device=w.device)
    call("gdm_conv1x1_pack_weight_hip", w, Cout, Cin, wpk)
    return wpk


def gemm_bf16x3(x, wpk, cout, scale=None, shift=None, act=ACT_NONE, pixel_major=False):
    """out[b] = act(scale * (W @ x[b]) + shift) on split-bf16 MFMA.  x f32[B,Cin,n] (channel-major, n % 32 == 0) ->
    f32[B,cout,n], or f32[B*n, cout] when pixel_major.  Inference only."""
    B, Cin, n = x.shape
    _require_fit("gemm_bf16x3", "x %s -> %d channels", (tuple(x.shape), cout), _map_bytes(B, Cin, 1, n), wpk.numel())
    x = _dev(x, torch.float32, "x")
    xpk = _packed_buffer(B, Cin, 1, n, x.device)
    call("gdm_conv3x3_pack_act_hip", x, B, Cin, 1, n, xpk)
    out = torch.empty((B * n, cout) if pixel_major else (B, cout, n), dtype=torch.float32, device=x.device)
    call("gdm_conv1x1_packed_hip", xpk, wpk, scale, shift, B, Cin, cout, 1, n, act, 1 if pixel_major else 0, out)
    return out


def spline_packed_buffer(C, M, device, avoid=None):
    """The zero-bordered operand buffer a SplineConv layer's kernels write for the NEXT layer's grouped GEMM (a [1, C, 1, M] map)."""
    return _packed_buffer(1, C, 1, M, device, avoid=avoid)


def spline_packed_supported(C):
    """The layer widths whose SplineConv kernels write that buffer: whole 128-channel chunks, a vertex's channels within one workgroup."""
    return C % 128 == 0 and C <= 512


def gemm_grouped(x_cm, wpk, rowidx, tile_co0, cout_total, xpk=None):
    """Grouped, gathered GEMM on the split-bf16 MFMA kernel (include/gdm.h gdm_gemm_grouped_hip): x_cm f32[1,Cin,M] (channel-major),
    wpk = gemm_pack_weight of a [cout_total, Cin] matrix, rowidx i32[R] (R % 256 == 0), tile_co0 i32[R/256] -> Y f32[R,128].
    xpk: the packed operand of x_cm when its producer wrote it (gdm_spline_*3_hip); otherwise one pack launch makes it here."""
    _, Cin, M = x_cm.shape
    R = rowidx.shape[0]
    _require_fit("gemm_grouped", "x %s, %d rows -> %d channels", (tuple(x_cm.shape), R, cout_total), _map_bytes(1, Cin, 1, M), wpk.numel())
    x_cm = _dev(x_cm, torch.float32, "x")
    if xpk is None:
        xpk = _packed_buffer(1, Cin, 1, M, x_cm.device)
        call("gdm_conv3x3_pack_act_hip", x_cm, 1, Cin, 1, M, xpk)
    Y = torch.empty((R, 128), dtype=torch.float32, device=x_cm.device)
    call("gdm_gemm_grouped_hip", xpk, wpk, rowidx, tile_co0, R, M, Cin, cout_total, Y)
    return Y


class _UpsampleBilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, OH, OW):
        x = _dev(x, torch.float32, "x")
        B, C, H, W = x.shape
        out = torch.empty((B, C, OH, OW), dtype=torch.float32, device=x.device)
        call("gdm_upsample_bilinear_hip", x, B * C, H, W, OH, OW, out)
        ctx.hw = (H, W)
        return out

    @staticmethod
    def backward(ctx, go):
        go = go.contiguous()
        B, C, OH, OW = go.shape
        H, W = ctx.hw
        g = torch.empty((B, C, H, W), dtype=torch.float32, device=go.device)
        call("gdm_upsample_bilinear_bwd_hip", go, B * C, H, W, OH, OW, g)
        return g, None, None


class _PReLU1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slope):
        x = x.contiguous()
        y = torch.empty_like(x)
        call("gdm_prelu1_hip", x, slope, x.numel(), y)
        ctx.save_for_backward(x, slope)
        return y

    @staticmethod
    def backward(ctx, go):
        x, slope = ctx.saved_tensors
        go = go.contiguous()
        gx = torch.empty_like(x)
        gs = torch.zeros_like(slope)
        call("gdm_prelu1_bwd_hip", x, go, slope, x.numel(), gx, gs)
        return gx, gs


def prelu1(x, slope):
    """Single-parameter PReLU with a streaming HIP backward (training path of PSPUpsample). x f32 cuda, numel % 4 == 0."""
    x = _dev(x, torch.float32, "x")
    return _PReLU1.apply(x, slope)


def upsample_bilinear(x, size):
    """x f32[B,C,H,W] -> f32[B,C,OH,OW], bilinear, align_corners=True (pspnet.py:26-29,38)."""
    return _UpsampleBilinear.apply(x, int(size[0]), int(size[1]))


# --------------------------------------------------------------------------------------
# matching
# --------------------------------------------------------------------------------------
def _workspace(nbytes, device):
    if _capturing_unscoped():
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
    key = (device.index, _stream_lane(device))
    ws = _pool.workspace.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _pool.workspace[key] = ws
    return ws


def match(scene, model, precision=MATCH_BF16X3, return_sim=False):
    """scene f32[B,128,N] (end_points['rgbd']), model f32[128,M] (end_points['mesh'][0]).
    Returns best_idx i32[B,N], best_sim f32[B,N] (and sim f32[B,N,M] when return_sim)."""
    scene = _dev(scene, torch.float32, "scene")
    model = _dev(model, torch.float32, "model")
    if model.dim() == 3:
        assert model.shape[0] == 1
        model = model[0]
    B, D, N = scene.shape
    M = model.shape[1]
    assert model.shape[0] == D
    L = _lib.lib()
    nbytes = L.gdm_match_workspace_bytes(B, N, M)
    ws = _workspace(nbytes, scene.device)
    best_idx = torch.empty((B, N), dtype=torch.int32, device=scene.device)
    best_sim = torch.empty((B, N), dtype=torch.float32, device=scene.device)
    sim = torch.empty((B, N, M), dtype=torch.float32, device=scene.device) if return_sim else None
    call("gdm_match_hip", scene, model, B, D, N, M, precision, best_idx, best_sim, sim, ws, ws.numel())
    return (best_idx, best_sim, sim) if return_sim else (best_idx, best_sim)


def match_pack(x, precision=MATCH_BF16X3, out=None):
    """x f32[R,128,n] (or [128,n]) channel-major -> u8[R*n, 512] normalised packed rows (stage 1 of match)."""
    x = _dev(x, torch.float32, "x")
    if x.dim() == 2:
        x = x.unsqueeze(0)
    R, D, n = x.shape
    L = _lib.lib()
    if out is None:
        out = torch.empty((L.gdm_match_rows_bytes(R * n),), dtype=torch.uint8, device=x.device)
    call("gdm_match_pack_hip", x, R, D, n, precision, out)
    return out


def match_pack2(x1, x2, precision=MATCH_BF16X3):
    """match_pack(x1), match_pack(x2) in one launch (include/gdm.h gdm_match_pack2_hip): the scene and the model descriptors of a step."""
    x1 = _dev(x1, torch.float32, "x1")
    x2 = _dev(x2, torch.float32, "x2")
    x1 = x1.unsqueeze(0) if x1.dim() == 2 else x1
    x2 = x2.unsqueeze(0) if x2.dim() == 2 else x2
    (R1, D, n1), (R2, D2, n2) = x1.shape, x2.shape
    if D != D2:
        raise ValueError("match_pack2: %d vs %d channels" % (D, D2))
    L = _lib.lib()
    o1 = torch.empty((L.gdm_match_rows_bytes(R1 * n1),), dtype=torch.uint8, device=x1.device)
    o2 = torch.empty((L.gdm_match_rows_bytes(R2 * n2),), dtype=torch.uint8, device=x1.device)
    call("gdm_match_pack2_hip", x1, R1, n1, o1, x2, R2, n2, o2, D, precision)
    return o1, o2


def match_packed(scene_rows, model_rows, B, N, M, precision=MATCH_BF16X3, return_sim=False, sim_out=None):
    """Stage 2 of match on packed rows: the MFMA similarity + arg-max kernel (+ split merge)."""
    L = _lib.lib()
    dev = scene_rows.device
    part = _workspace(L.gdm_match_partial_bytes(B, N), dev)
    best_idx = torch.empty((B, N), dtype=torch.int32, device=dev)
    best_sim = torch.empty((B, N), dtype=torch.float32, device=dev)
    sim = None
    if return_sim:
        sim = sim_out if sim_out is not None else torch.empty((B, N, M), dtype=torch.float32, device=dev)
    call("gdm_match_packed_hip", scene_rows, model_rows, B * N, M, precision, best_idx, best_sim, sim,
         part, part.numel())
    return (best_idx, best_sim, sim) if return_sim else (best_idx, best_sim)


MATCH_SOFT_MAX_GAMMA = _lib.GDM_MATCH_SOFT_MAX_GAMMA
MATCH_SOFT_MAX_M = _lib.GDM_MATCH_SOFT_MAX_M


def match_soft_packed(scene_rows, model_rows, model_xyz, B, N, M, precision=MATCH_BF16X3, gamma=16.0):
    """match_packed plus the soft assignment at temperature gamma (include/gdm.h gdm_match_soft_packed_hip): model_xyz f32[M,3] ->
    best_idx i32[B,N], best_sim f32[B,N] (the bits of match_packed), lse f32[B,N], conf f32[B,N], soft_xyz f32[B,N,3].  No [N, M]
    tensor; 0 < gamma <= 40 and M <= 16384, refused otherwise."""
    L = _lib.lib()
    model_xyz = _dev(model_xyz, torch.float32, "model_xyz")
    if tuple(model_xyz.shape) != (M, 3):
        raise ValueError("match_soft_packed: model_xyz is %s, expected (%d, 3)" % (tuple(model_xyz.shape), M))
    dev = scene_rows.device
    part = _workspace(L.gdm_match_soft_partial_bytes(B, N), dev)
    best_idx = torch.empty((B, N), dtype=torch.int32, device=dev)
    best_sim = torch.empty((B, N), dtype=torch.float32, device=dev)
    lse = torch.empty((B, N), dtype=torch.float32, device=dev)
    conf = torch.empty((B, N), dtype=torch.float32, device=dev)
    soft_xyz = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    call("gdm_match_soft_packed_hip", scene_rows, model_rows, model_xyz, B * N, M, precision, float(gamma), best_idx, best_sim, lse, conf,
         soft_xyz, part, part.numel())
    return best_idx, best_sim, lse, conf, soft_xyz


def match_soft(scene, model, model_xyz, precision=MATCH_BF16X3, gamma=16.0):
    """scene f32[B,128,N], model f32[128,M], model_xyz f32[M,3] -> (best_idx, best_sim, lse, conf, soft_xyz): both packs, then
    match_soft_packed."""
    scene = _dev(scene, torch.float32, "scene")
    model = _dev(model, torch.float32, "model")
    if model.dim() == 3:
        assert model.shape[0] == 1
        model = model[0]
    B, D, N = scene.shape
    assert model.shape[0] == D
    srows, mrows = match_pack2(scene, model, precision)
    return match_soft_packed(srows, mrows, model_xyz, B, N, model.shape[1], precision, gamma)


def match_score(conf, mask):
    """conf f32[B,N], mask u8[B,N] -> score f32[B]: the mean confidence of the masked points, 0 for a crop with none."""
    conf = _dev(conf, torch.float32, "conf")
    mask = _dev(mask, torch.uint8, "mask")
    B, N = conf.shape
    score = torch.empty((B,), dtype=torch.float32, device=conf.device)
    call("gdm_match_score_hip", conf, mask, B, N, score)
    return score


def match_twoway_packed(scene_rows, model_rows, mask, B, N, M, precision=MATCH_BF16X3):
    """match_packed plus the reverse direction under mask u8[B,N] (include/gdm.h THE TWO-WAY RULE): -> best_idx i32[B,N], best_sim
    f32[B,N] (the bits of match_packed), col_idx i32[B,M] = per crop and vertex the masked point with the largest similarity (the
    lowest on ties, -1 where there is none), col_sim f32[B,M] (-inf there).  No [N, M] tensor; M <= 16384, refused otherwise."""
    L = _lib.lib()
    mask = _dev(mask, torch.uint8, "mask")
    if tuple(mask.shape) != (B, N):
        raise ValueError("match_twoway_packed: mask is %s, expected (%d, %d)" % (tuple(mask.shape), B, N))
    dev = scene_rows.device
    part = _workspace(L.gdm_match_twoway_partial_bytes(B, N, M), dev)
    best_idx = torch.empty((B, N), dtype=torch.int32, device=dev)
    best_sim = torch.empty((B, N), dtype=torch.float32, device=dev)
    col_idx = torch.empty((B, M), dtype=torch.int32, device=dev)
    col_sim = torch.empty((B, M), dtype=torch.float32, device=dev)
    call("gdm_match_twoway_packed_hip", scene_rows, model_rows, mask, B, N, M, precision, best_idx, best_sim, col_idx, col_sim, part,
         part.numel())
    return best_idx, best_sim, col_idx, col_sim


def match_twoway(scene, model, mask, precision=MATCH_BF16X3):
    """scene f32[B,128,N], model f32[128,M], mask u8[B,N] -> (best_idx, best_sim, col_idx, col_sim): both packs, then
    match_twoway_packed."""
    scene = _dev(scene, torch.float32, "scene")
    model = _dev(model, torch.float32, "model")
    if model.dim() == 3:
        assert model.shape[0] == 1
        model = model[0]
    B, D, N = scene.shape
    assert model.shape[0] == D
    srows, mrows = match_pack2(scene, model, precision)
    return match_twoway_packed(srows, mrows, mask, B, N, model.shape[1], precision)


DUAL_KEYS = ("best_idx", "best_sim", "lse", "conf", "soft_xyz", "col_idx", "col_sim", "col_lse", "col_conf", "dual")


def match_dual_packed(scene_rows, model_rows, model_xyz, mask, B, N, M, precision=MATCH_BF16X3, gamma=16.0):
    """Soft matching in both directions from one pass (include/gdm.h THE DUAL RULE): match_soft_packed's five outputs and
    match_twoway_packed's col_idx / col_sim, bit for bit, plus col_lse f32[B,M] (the log-sum-exp of a vertex's column over the masked
    points of the crop, -inf where there is none), col_conf f32[B,M] (the share of that column its best point holds, 0 where
    col_idx = -1) and dual f32[B,N] (conf times the share of the arg-max vertex's column that the point holds; 0 for an unmasked
    point; 0 <= dual <= conf).  -> the ten tensors in the order of DUAL_KEYS.  No [N, M] tensor; 0 < gamma <= 40 and M <= 16384,
    refused otherwise."""
    L = _lib.lib()
    model_xyz = _dev(model_xyz, torch.float32, "model_xyz")
    mask = _dev(mask, torch.uint8, "mask")
    if tuple(model_xyz.shape) != (M, 3):
        raise ValueError("match_dual_packed: model_xyz is %s, expected (%d, 3)" % (tuple(model_xyz.shape), M))
    if tuple(mask.shape) != (B, N):
        raise ValueError("match_dual_packed: mask is %s, expected (%d, %d)" % (tuple(mask.shape), B, N))
    dev = scene_rows.device
    part = _workspace(L.gdm_match_dual_partial_bytes(B, N, M), dev)
    f32, i32 = torch.float32, torch.int32
    out = [torch.empty(shape, dtype=dt, device=dev) for shape, dt in
           (((B, N), i32), ((B, N), f32), ((B, N), f32), ((B, N), f32), ((B, N, 3), f32),
            ((B, M), i32), ((B, M), f32), ((B, M), f32), ((B, M), f32), ((B, N), f32))]
    call("gdm_match_dual_packed_hip", scene_rows, model_rows, model_xyz, mask, B, N, M, precision, float(gamma), *out, part, part.numel())
    return tuple(out)


def match_dual(scene, model, model_xyz, mask, precision=MATCH_BF16X3, gamma=16.0):
    """scene f32[B,128,N], model f32[128,M], model_xyz f32[M,3], mask u8[B,N] -> the ten tensors of match_dual_packed: both packs,
    then match_dual_packed."""
    scene = _dev(scene, torch.float32, "scene")
    model = _dev(model, torch.float32, "model")
    if model.dim() == 3:
        assert model.shape[0] == 1
        model = model[0]
    B, D, N = scene.shape
    assert model.shape[0] == D
    srows, mrows = match_pack2(scene, model, precision)
    return match_dual_packed(srows, mrows, model_xyz, mask, B, N, model.shape[1], precision, gamma)


def match_cycle(cld_rgb_nrm, best_idx, col_idx, mask, radius):
    """The cycle-consistency filter (include/gdm.h THE CYCLE RULE): cld_rgb_nrm f32[B,9,N] (rows 0-2 = xyz), best_idx i32[B,N], col_idx
    i32[B,M], mask u8[B,N]; a masked point is kept iff the point its vertex picks back lies within `radius` of it (radius = 0: the
    mutual best pairs).  -> pair_mask u8[B,N], pair_count i32[B], cycle_d2 f32[B,N] (+inf where no distance was formed)."""
    cld = _dev(cld_rgb_nrm, torch.float32, "cld_rgb_nrm")
    best_idx = _dev(best_idx, torch.int32, "best_idx")
    col_idx = _dev(col_idx, torch.int32, "col_idx")
    mask = _dev(mask, torch.uint8, "mask")
    B, N = mask.shape
    if cld.dim() != 3 or cld.shape[0] != B or cld.shape[1] < 3 or cld.shape[2] != N or best_idx.shape != mask.shape or col_idx.shape[0] != B:
        raise ValueError("match_cycle: cld_rgb_nrm %s, best_idx %s, col_idx %s do not go with mask %s" %
                         (tuple(cld.shape), tuple(best_idx.shape), tuple(col_idx.shape), (B, N)))
    pair_mask = torch.empty((B, N), dtype=torch.uint8, device=mask.device)
    pair_count = torch.empty((B,), dtype=torch.int32, device=mask.device)
    cycle_d2 = torch.empty((B, N), dtype=torch.float32, device=mask.device)
    call("gdm_match_cycle_hip", cld, cld.stride(0), 1, cld.shape[2], best_idx, col_idx, mask, B, N, col_idx.shape[1], float(radius),
         pair_mask, pair_count, cycle_d2)
    return pair_mask, pair_count, cycle_d2


def seg_mask(seg):
    """seg f32[B,2,N] -> (mask u8[B,N] = argmax==1, count i32[B])."""
    seg = _dev(seg, torch.float32, "seg")
    B, two, N = seg.shape
    assert two == 2
    mask = torch.empty((B, N), dtype=torch.uint8, device=seg.device)
    count = torch.empty((B,), dtype=torch.int32, device=seg.device)
    call("gdm_seg_mask_hip", seg, B, N, mask, count)
    return mask, count


# --------------------------------------------------------------------------------------
# front end: hash-sampled points and the assembled item (gdm_sample.hip)
# --------------------------------------------------------------------------------------
def sample_assemble(valid_depth, dpt_xyz, rgb, normals, n_points, mask=None, seed=0):
    """The N points of every crop by the counter-based rule of include/gdm.h (gdm_sample_assemble_hip) and the assembled item, one
    launch: valid_depth f32[B,S,S] (a pixel is valid where it is > 1e-6), dpt_xyz f32[B,S,S,3], rgb f32[B,3,S,S], normals
    f32[B,3,S,S], mask u8[B,S,S] or None -> choose i32[B,N], cld_rgb_nrm f32[B,9,N], labels u8[B,N] (None without a mask),
    n_valid i32[B].  seed: an int (its low 32 bits), or a one-element int32 device tensor whose word the kernel reads when it runs
    (a captured graph then draws differently on every replay).  The scratch buffer comes from the current BufferPool."""
    valid_depth = _dev(valid_depth, torch.float32, "valid_depth")
    dpt_xyz = _dev(dpt_xyz, torch.float32, "dpt_xyz")
    rgb = _dev(rgb, torch.float32, "rgb")
    normals = _dev(normals, torch.float32, "normals")
    if valid_depth.dim() != 3 or valid_depth.shape[1] != valid_depth.shape[2]:
        raise ValueError("valid_depth must be [B,S,S], got %s" % (tuple(valid_depth.shape),))
    B, S, N = valid_depth.shape[0], valid_depth.shape[1], int(n_points)
    for t, shape, name in ((dpt_xyz, (B, S, S, 3), "dpt_xyz"), (rgb, (B, 3, S, S), "rgb"), (normals, (B, 3, S, S), "normals")):
        if tuple(t.shape) != shape:
            raise ValueError("%s must be %s, got %s" % (name, list(shape), tuple(t.shape)))
    if not 1 <= N <= _lib.GDM_SAMPLE_MAX_N:
        raise ValueError("n_points=%d not in [1, %d]" % (N, _lib.GDM_SAMPLE_MAX_N))
    dev = valid_depth.device
    seed_val, seed_ptr = _seed_args(seed)
    labels = None
    if mask is not None:
        mask = _dev(mask, torch.uint8, "mask")
        if tuple(mask.shape) != (B, S, S):
            raise ValueError("mask must be [B=%d,S=%d,S=%d], got %s" % (B, S, S, tuple(mask.shape)))
        labels = torch.empty((B, N), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    need = L.gdm_sample_assemble_workspace_bytes(B, S)
    if need == 0:
        raise ValueError("sample_assemble: unsupported shape B=%d S=%d" % (B, S))
    ws = _workspace(need, dev)
    choose = torch.empty((B, N), dtype=torch.int32, device=dev)
    cld_rgb_nrm = torch.empty((B, 9, N), dtype=torch.float32, device=dev)
    n_valid = torch.empty((B,), dtype=torch.int32, device=dev)
    call("gdm_sample_assemble_hip", valid_depth, dpt_xyz, rgb, normals, mask, B, S, N, seed_val, seed_ptr, choose, cld_rgb_nrm, labels,
         n_valid, ws, ws.numel())
    return choose, cld_rgb_nrm, labels, n_valid


def _seed_args(seed):
    """seed -> (value, device pointer or None): an int (its low 32 bits) or a one-element int32 device tensor read when the kernel runs."""
    if torch.is_tensor(seed):
        if not seed.is_cuda or seed.dtype != torch.int32 or seed.numel() != 1:
            raise ValueError("a tensor seed must be a one-element int32 device tensor")
        return 0, seed.data_ptr()
    return int(seed) & 0xffffffff, None


def augment_crops(rgb, depth, mask=None, background=None, enable=None, seed=0):
    """The YCB-V training item's colour, noise and background augmentation of the crop by the integer rule of include/gdm.h
    (gdm_augment_crops_hip), two launches whatever B: rgb f32[B,3,S,S] as crop_from_boxes wrote it, depth f32[B,S,S], mask u8[B,S,S]
    (needed with a background), background = (bg_rgb u8[Nb,Hb,Wb,3], bg_depth f32[Nb,Hb,Wb], bg_mask u8[Nb,Hb,Wb]) or None,
    enable u8[B] or None (0 = the crop is copied bit for bit) -> (rgb f32[B,3,S,S], depth f32[B,S,S]).  seed as for sample_assemble.
    The uint8 image between the passes lives in the current BufferPool's scratch buffer."""
    rgb = _dev(rgb, torch.float32, "rgb")
    depth = _dev(depth, torch.float32, "depth")
    if depth.dim() != 3 or depth.shape[1] != depth.shape[2]:
        raise ValueError("depth must be [B,S,S], got %s" % (tuple(depth.shape),))
    B, S = depth.shape[0], depth.shape[1]
    if tuple(rgb.shape) != (B, 3, S, S):
        raise ValueError("rgb must be %s, got %s" % ([B, 3, S, S], tuple(rgb.shape)))
    if not _lib.GDM_AUG_MIN_S <= S <= _lib.GDM_AUG_MAX_S:
        raise ValueError("augment_crops: S=%d not in [%d, %d] (a blur reaches 15 pixels)" % (S, _lib.GDM_AUG_MIN_S, _lib.GDM_AUG_MAX_S))
    if mask is not None:
        mask = _dev(mask, torch.uint8, "mask")
        if tuple(mask.shape) != (B, S, S):
            raise ValueError("mask must be [B=%d,S=%d,S=%d], got %s" % (B, S, S, tuple(mask.shape)))
    if enable is not None:
        enable = _dev(enable, torch.uint8, "enable")
        if tuple(enable.shape) != (B,):
            raise ValueError("enable must be [B=%d], got %s" % (B, tuple(enable.shape)))
    bg_rgb, bg_depth, bg_mask, Nb, Hb, Wb = None, None, None, 0, 0, 0
    if background is not None:
        if mask is None:
            raise ValueError("augment_crops: the background paste needs the crop's mask")
        bg_rgb = _dev(background[0], torch.uint8, "bg_rgb")
        bg_depth = _dev(background[1], torch.float32, "bg_depth")
        bg_mask = _dev(background[2], torch.uint8, "bg_mask")
        if bg_rgb.dim() != 4 or bg_rgb.shape[3] != 3:
            raise ValueError("bg_rgb must be [Nb,Hb,Wb,3], got %s" % (tuple(bg_rgb.shape),))
        Nb, Hb, Wb = bg_rgb.shape[:3]
        if tuple(bg_depth.shape) != (Nb, Hb, Wb) or tuple(bg_mask.shape) != (Nb, Hb, Wb):
            raise ValueError("bg_depth and bg_mask must be %s, got %s and %s" % ([Nb, Hb, Wb], tuple(bg_depth.shape), tuple(bg_mask.shape)))
        if Nb < 1 or Hb < S + 2 or Wb < S + 2:
            raise ValueError("the bank's frames must be at least S + 2 = %d a side, got %d x %d (Nb = %d)" % (S + 2, Hb, Wb, Nb))
    seed_val, seed_ptr = _seed_args(seed)
    L = _lib.lib()
    ws = _workspace(L.gdm_augment_workspace_bytes(B, S), rgb.device)
    out_rgb, out_depth = torch.empty_like(rgb), torch.empty_like(depth)
    call("gdm_augment_crops_hip", rgb, depth, mask, bg_rgb, bg_depth, bg_mask, enable, B, S, Nb, Hb, Wb, seed_val, seed_ptr, out_rgb,
         out_depth, ws, ws.numel())
    return out_rgb, out_depth


# --------------------------------------------------------------------------------------
# a structured-light depth sensor on a depth frame (gdm_sensor.hip; sensor.py is the interface with names and defaults)
# --------------------------------------------------------------------------------------
def _header_enums(prefix):
    """{name: value} of the `enum { NAME = int, ... };` constants of include/gdm.h whose names start with `prefix` (the header keeps
    some limits as enumerators; _lib reads the #defines)."""
    import re
    with open(_lib.HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    found = {}
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        for name, val in re.findall(r"\b(%s\w+)\s*=\s*(-?\d+)" % re.escape(prefix), body):
            found[name] = int(val)
    return found


SENSOR = _header_enums("GDM_SENSOR_")          # the stage bits, GDM_SENSOR_MAX_DISP, GDM_SENSOR_TILE_W / _H, GDM_SENSOR_MAX_K


def depth_sensor(depth, K, baseline, z_min, z_max, sigma_d, subpixel, cos_min, cos_soft, p_shift, stages, seed=0, out=None):
    """THE SENSOR RULE of include/gdm.h (gdm_depth_sensor_hip), one launch: depth f32[n,H,W] on the device (metres), K a HOST
    float32 tensor [3,3] or [n,3,3] (the library checks the shadow window from it before the launch), the rule's scalars, stages the
    sum of the GDM_SENSOR_* stage bits, seed as for sample_assemble -> (out_depth f32[n,H,W], cause u8[n,H,W]).  out = (out_depth,
    cause) to write into given tensors.  What the rule does not allow the library refuses (GdmError)."""
    depth = _dev(depth, torch.float32, "depth")
    if depth.dim() != 3:
        raise ValueError("depth must be [n,H,W], got %s" % (tuple(depth.shape),))
    n, H, W = depth.shape
    if not isinstance(K, torch.Tensor) or K.is_cuda or K.dtype != torch.float32:
        raise TypeError("K must be a float32 tensor on the host (the shadow window is checked before the launch)")
    if tuple(K.shape) not in ((3, 3), (n, 3, 3)):
        raise ValueError("K must be [3,3] or [n=%d,3,3], got %s" % (n, tuple(K.shape)))
    K = K.contiguous()
    seed_val, seed_ptr = _seed_args(seed)
    if out is None:
        out_depth, cause = torch.empty_like(depth), torch.empty((n, H, W), dtype=torch.uint8, device=depth.device)
    else:
        out_depth, cause = _dev(out[0], torch.float32, "out_depth"), _dev(out[1], torch.uint8, "cause")
        if tuple(out_depth.shape) != (n, H, W) or tuple(cause.shape) != (n, H, W):
            raise ValueError("out_depth and cause must be %s" % ([n, H, W],))
    call("gdm_depth_sensor_hip", depth, K, int(K.dim() == 3), n, H, W, float(baseline), float(z_min), float(z_max), float(sigma_d),
         float(subpixel), float(cos_min), float(cos_soft), float(p_shift), int(stages), seed_val, seed_ptr, out_depth, cause)
    return out_depth, cause


# --------------------------------------------------------------------------------------
# BOP pose errors (lib/pysixd/pose_error.py:22-179): gdm_bop.hip


def _k64(K, n, name):
    """K f64[3,3] or f64[n,3,3] on the device -> (tensor, k_per_instance)."""
    K = _dev(K, torch.float64, name)
    if tuple(K.shape) == (3, 3):
        return K, 0
    if tuple(K.shape) == (n, 3, 3):
        return K, 1
    raise ValueError("%s must be [3,3] or [n=%d,3,3], got %s" % (name, n, tuple(K.shape)))


def mssd_mspd(RT_est, RT_gt, pts, sym_R, sym_t, K):
    """MSSD / MSPD of n pose pairs of one object (gdm_mssd_mspd_hip): RT_est, RT_gt f64[n,3,4], pts f64[M,3], sym_R f64[S,3,3],
    sym_t f64[S,3], K f64[3,3] or f64[n,3,3] -> mssd f64[n], mspd f64[n], best_sym_mssd i32[n], best_sym_mspd i32[n].  The largest
    temporary is the per-symmetry maxima f64[2,n,S]."""
    RT_est = _dev(RT_est, torch.float64, "RT_est")
    RT_gt = _dev(RT_gt, torch.float64, "RT_gt")
    pts = _dev(pts, torch.float64, "pts")
    sym_R = _dev(sym_R, torch.float64, "sym_R")
    sym_t = _dev(sym_t, torch.float64, "sym_t")
    if RT_est.dim() != 3 or tuple(RT_est.shape[1:]) != (3, 4) or RT_est.shape[0] < 1:
        raise ValueError("RT_est must be [n,3,4], got %s" % (tuple(RT_est.shape),))
    n = RT_est.shape[0]
    if tuple(RT_gt.shape) != (n, 3, 4):
        raise ValueError("RT_gt must be [n=%d,3,4], got %s" % (n, tuple(RT_gt.shape)))
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError("pts must be [M,3], got %s" % (tuple(pts.shape),))
    if sym_R.dim() != 3 or tuple(sym_R.shape[1:]) != (3, 3) or sym_R.shape[0] < 1:
        raise ValueError("sym_R must be [S,3,3], got %s" % (tuple(sym_R.shape),))
    S = sym_R.shape[0]
    if tuple(sym_t.shape) != (S, 3):
        raise ValueError("sym_t must be [S=%d,3], got %s" % (S, tuple(sym_t.shape)))
    K, kpi = _k64(K, n, "K")
    dev = RT_est.device
    err = torch.empty((2, n, S), dtype=torch.float64, device=dev)
    out = torch.empty((2, n), dtype=torch.float64, device=dev)
    best = torch.empty((2, n), dtype=torch.int32, device=dev)
    call("gdm_mssd_mspd_hip", RT_est, RT_gt, pts, sym_R, sym_t, K, kpi, n, pts.shape[0], S, err, out[0], out[1], best[0], best[1])
    return out[0], out[1], best[0], best[1]


def render_depth(verts, faces, RT, K, H, W, near, keep_inf=False):
    """Depth images of one mesh in n poses by the pixel rule of include/gdm.h (gdm_render_depth_hip): verts f32|f64[V,3], faces
    i32[F,3], RT f64[n,3,4], K f64[3,3] or f64[n,3,3] -> f32[n,H,W], 0 where nothing is drawn (+inf with keep_inf, for
    vsd_counts(inf_is_empty=True))."""
    if not isinstance(verts, torch.Tensor) or verts.dtype not in (torch.float32, torch.float64):
        _dev(verts, torch.float32, "verts")
        raise TypeError("verts must be float32 or float64")
    verts = _dev(verts, verts.dtype, "verts")
    faces = _dev(faces, torch.int32, "faces")
    RT = _dev(RT, torch.float64, "RT")
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] < 1:
        raise ValueError("verts must be [V,3], got %s" % (tuple(verts.shape),))
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError("faces must be [F,3], got %s" % (tuple(faces.shape),))
    if RT.dim() != 3 or tuple(RT.shape[1:]) != (3, 4) or RT.shape[0] < 1:
        raise ValueError("RT must be [n,3,4], got %s" % (tuple(RT.shape),))
    n, H, W = RT.shape[0], int(H), int(W)
    K, kpi = _k64(K, n, "K")
    depth = torch.empty((n, H, W), dtype=torch.float32, device=RT.device)
    call("gdm_render_depth_hip", verts, int(verts.dtype == torch.float64), faces, RT, K, kpi, n, verts.shape[0], faces.shape[0], H, W,
         float(near), int(bool(keep_inf)), depth)
    return depth


def vsd_counts(depth_est, depth_gt, depth_test, K, delta, taus, diameter=None, tlinear=False, inf_is_empty=False):
    """The integer counts of the VSD error (gdm_vsd_counts_hip): depth_est, depth_gt f32[n,H,W], depth_test f32[H,W] or f32[n,H,W],
    K f64[3,3] or f64[n,3,3], taus a sequence of at most 16 floats -> union i32[n], inter i32[n], cost i32[n,T] (and, with tlinear,
    the truncated-linear cost sums f64[n,T])."""
    depth_est = _dev(depth_est, torch.float32, "depth_est")
    depth_gt = _dev(depth_gt, torch.float32, "depth_gt")
    depth_test = _dev(depth_test, torch.float32, "depth_test")
    if depth_est.dim() != 3 or depth_est.shape[0] < 1:
        raise ValueError("depth_est must be [n,H,W], got %s" % (tuple(depth_est.shape),))
    n, H, W = depth_est.shape
    if tuple(depth_gt.shape) != (n, H, W):
        raise ValueError("depth_gt must be %s, got %s" % ([n, H, W], tuple(depth_gt.shape)))
    if tuple(depth_test.shape) == (H, W):
        tpi = 0
    elif tuple(depth_test.shape) == (n, H, W):
        tpi = 1
    else:
        raise ValueError("depth_test must be [H,W] or %s, got %s" % ([n, H, W], tuple(depth_test.shape)))
    K, kpi = _k64(K, n, "K")
    taus = [float(t) for t in taus]
    T = len(taus)
    if not 1 <= T <= 16:
        raise ValueError("vsd_counts takes 1 to 16 taus, got %d" % T)
    dev = depth_est.device
    counts = torch.empty((n, 2 + T), dtype=torch.int32, device=dev)
    tl = torch.empty((n, T), dtype=torch.float64, device=dev) if tlinear else None
    call("gdm_vsd_counts_hip", depth_est, depth_gt, depth_test, tpi, K, kpi, n, H, W, float(delta), (ctypes.c_double * T)(*taus), T,
         float(diameter) if diameter else 0.0, int(bool(inf_is_empty)), counts, tl)
    if tlinear:
        return counts[:, 0], counts[:, 1], counts[:, 2:], tl
    return counts[:, 0], counts[:, 1], counts[:, 2:]


RENDER_MAX_SLOTS = 8          # GDM_RENDER_MAX_SLOTS / GDM_RENDER_MAX_OBJECTS of include/gdm.h (an enum there; the library refuses beyond)
RENDER_MAX_OBJECTS = 256


def render_frames(verts, vcol, vnrm, faces, obj_face0, slot_obj, RT, K, light, H, W, ambient, near, textures=None):
    """Colour, depth, instance mask, face ids and per-slot statistics of n frames of S posed objects by the rule of include/gdm.h
    (gdm_render_frames_hip): verts f32|f64[Vt,3], vcol u8[Vt,3], vnrm f32[Vt,3], faces i32[Ft,3] on the device; obj_face0 a HOST
    sequence of O+1 ascending face offsets; slot_obj i32[n,S] (-1: empty), RT f64[n,S,3,4], K f64[3,3] or f64[n,3,3], light f64[n,3]
    -> rgb u8[n,H,W,3], depth f32[n,H,W], inst u8[n,H,W], face i32[n,H,W], stats i32[n,S,6] = (px_all, px_vis, xmin, ymin, xmax,
    ymax).  render.render_frames is the interface with defaults and the derived outputs.  textures = (fuv f32[Ft,3,2], tex u8[T,4],
    tex_tab i64[O,4], flip_v), all three tensors on the device: the textured entry (gdm_render_frames_tex_hip) instead."""
    if not isinstance(verts, torch.Tensor) or verts.dtype not in (torch.float32, torch.float64):
        _dev(verts, torch.float32, "verts")
        raise TypeError("verts must be float32 or float64")
    verts = _dev(verts, verts.dtype, "verts")
    vcol = _dev(vcol, torch.uint8, "vcol")
    vnrm = _dev(vnrm, torch.float32, "vnrm")
    faces = _dev(faces, torch.int32, "faces")
    slot_obj = _dev(slot_obj, torch.int32, "slot_obj")
    RT = _dev(RT, torch.float64, "RT")
    light = _dev(light, torch.float64, "light")
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] < 1:
        raise ValueError("verts must be [Vt,3], got %s" % (tuple(verts.shape),))
    Vt = verts.shape[0]
    if tuple(vcol.shape) != (Vt, 3) or tuple(vnrm.shape) != (Vt, 3):
        raise ValueError("vcol and vnrm must be [Vt=%d,3], got %s and %s" % (Vt, tuple(vcol.shape), tuple(vnrm.shape)))
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError("faces must be [Ft,3], got %s" % (tuple(faces.shape),))
    if RT.dim() != 4 or tuple(RT.shape[2:]) != (3, 4) or RT.shape[0] < 1 or RT.shape[1] < 1:
        raise ValueError("RT must be [n,S,3,4], got %s" % (tuple(RT.shape),))
    n, S = RT.shape[:2]
    if S > RENDER_MAX_SLOTS:
        raise ValueError("S=%d slots, at most %d" % (S, RENDER_MAX_SLOTS))
    if tuple(slot_obj.shape) != (n, S):
        raise ValueError("slot_obj must be [n=%d,S=%d], got %s" % (n, S, tuple(slot_obj.shape)))
    if tuple(light.shape) != (n, 3):
        raise ValueError("light must be [n=%d,3], got %s" % (n, tuple(light.shape)))
    table = [int(v) for v in obj_face0]
    O = len(table) - 1
    if not 1 <= O <= RENDER_MAX_OBJECTS:
        raise ValueError("obj_face0 must hold O+1 offsets for 1 <= O <= %d objects, got %d values" % (RENDER_MAX_OBJECTS, len(table)))
    K, kpi = _k64(K, n, "K")
    H, W = int(H), int(W)
    dev = RT.device
    nbytes = call("gdm_render_frames_workspace_bytes", n, S, H, W)
    if nbytes == 0:
        raise ValueError("render_frames: n=%d S=%d H=%d W=%d outside what gdm_render_frames_hip addresses" % (n, S, H, W))
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
    rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    inst = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    face = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    stats = torch.empty((n, S, 6), dtype=torch.int32, device=dev)
    args = (verts, int(verts.dtype == torch.float64), vcol, vnrm, faces, (ctypes.c_int32 * (O + 1))(*table), slot_obj, RT, K, kpi, light,
            float(ambient), float(near), n, S, O, Vt, faces.shape[0], H, W, ws, nbytes, rgb, depth, inst, face, stats)
    if textures is None:
        call("gdm_render_frames_hip", *args)
    else:
        fuv, tex, tex_tab, flip_v = textures
        fuv = _dev(fuv, torch.float32, "fuv")
        tex = _dev(tex, torch.uint8, "tex")
        tex_tab = _dev(tex_tab, torch.int64, "tex_tab")
        if tuple(fuv.shape) != (faces.shape[0], 3, 2):
            raise ValueError("fuv must be [Ft=%d,3,2], got %s" % (faces.shape[0], tuple(fuv.shape)))
        if tex.dim() != 2 or tex.shape[1] != 4 or not 1 <= tex.shape[0] < 1 << 31:
            raise ValueError("tex must be u8[T,4] with 1 <= T < 2^31, got %s" % (tuple(tex.shape),))
        if tuple(tex_tab.shape) != (O, 4):
            raise ValueError("tex_tab must be [O=%d,4], got %s" % (O, tuple(tex_tab.shape)))
        call("gdm_render_frames_tex_hip", *args, fuv, tex, tex_tab, tex.shape[0], int(bool(flip_v)))
    return rgb, depth, inst, face, stats


def texture_mips(image, L=None):
    """The texture pyramid of image u8[H,W,3] (device) by THE TEXTURE RULE of include/gdm.h (gdm_texture_mips_hip): u8[T,4], level 0
    the image, every further level the 2 x 2 mean of the one before; L levels, default all 1 + floor(log2(max(W, H)))."""
    image = _dev(image, torch.uint8, "image")
    if image.dim() != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError("image must be u8[H,W,3], got %s" % (tuple(image.shape),))
    H, W = image.shape[:2]
    L = max(H, W).bit_length() if L is None else int(L)
    T = call("gdm_texture_pyramid_texels", H, W, L)
    if T == 0:
        raise ValueError("texture_mips: H=%d W=%d L=%d outside what gdm_texture_mips_hip builds" % (H, W, L))
    pyr = torch.empty((T, 4), dtype=torch.uint8, device=image.device)
    call("gdm_texture_mips_hip", image, H, W, L, pyr, T)
    return pyr
