"""Guard bands round the tensors a library call is given: does a kernel stay inside them?

Every tensor of the suite comes from torch's caching allocator: it starts on a 512-byte boundary inside a large segment, next to
other live blocks.  A store one tile past the end of `out` then corrupts some other tensor or none, and no fp64 comparison sees it.
This module places a tensor between two bands of known bytes and looks at the bands afterwards.

  Guarded                    one uint8 allocation of G + skew + nbytes + G bytes filled with 0xFF (NaN as fp32, -1 as int32), a typed
                             view of the interior strided like the original, and check()
  guard(t) / guard_like()    explicit placement, for the tensors whose addresses travel inside job structures (gdm_pw_seg,
                             gdm_pw_job, gdm_knn_job, gdm_copy_job, the layer arrays of gdm_point_heads2_hip), which the generic
                             wrapper cannot see
  guarded_calls(monkeypatch) a context that replaces `call` in the six modules that bind it: every torch.Tensor argument of every
                             library call is copied into a guarded buffer, the real entry runs on the copies, the device is
                             synchronised, and then both bands of every argument must still be 0xFF and the interior of every
                             argument that include/gdm.h declares `const` must be unchanged; the other spans are copied back

What it proves, and what it cannot:
  * a WRITE within G = 1 MiB of either edge of an argument is caught.  G is a condition, not a measurement: it exceeds one whole
    row block of the convolution tile (256 pixels x 128 channels x 4 B = 128 KiB).  An access that strays further than G lands
    outside what this harness can see.
  * a write of the byte 0xFF over 0xFF is invisible (an fp32 NaN with all mantissa bits set, an int32 -1).
  * an over-READ into a band brings NaN / -1 into the kernel.  If the value is used, the fp64 comparison of the test fails; if it is
    clamped or multiplied away it stays invisible.  That is why inputs are surrounded by NaN and not by a plausible number.
  * bytes of a strided view's span that lie between its rows (the other channels of a channel slice) travel with the copy and are
    not checked.

skew: 0 keeps the original address modulo 16 (G is a multiple of 512).  skew = 4 moves the arguments that SKEW_BRANCH names for the
entry -- or the ones given as skew_params -- by 4 bytes (8 for 8-byte elements), so a tensor that was 16-byte aligned sits at an
address = 4 (mod 16).  The two tables hold what reading the launchers of csrc/*.hip found and the GPU tests exercise, row by row;
they do not claim to be complete (packed outputs from the operand pool, for one, are not listed).  An argument in neither table is
never skewed.

Aliasing or overlapping arguments share one copy: a violation then names them together ("x/y"), its before / after offsets count
from the edges of their union, and the const-interior check is left out as soon as one of them is writable -- a write into a const
tensor that merely overlaps an output is not attributed.  That is exact for the in-place y == x case it exists for.

Not for use inside hipGraph capture (it allocates and synchronises): guarded_calls refuses while the current stream captures.

guarded_calls(record=True) also keeps the bytes of every output of every call, and guard=False does only that: a test runs one body
plain and under guards and compares the two recordings bit for bit (assert_same_record), inside filled_empties() so that what a
kernel leaves unwritten holds the same bytes in both runs.  Exceptions a target raises (a GdmError refusal) pass through, after the
wrapper has verified that nothing at all was written.
"""
import collections
import contextlib
import re

import torch

from geometric_aware_dense_matching_amd import _lib

G = 1 << 20          # bytes of guard on each side
FILL = 0xFF

MODULES = ("ops", "pose", "splinecnn", "pointops", "frontend", "targets")          # the modules that bind `call` (from ._lib import call)

# ---- alignment tables: entry -> the parameters (as include/gdm.h spells them) whose ADDRESS the launcher looks at ----------------
# the launcher (or its kernel) BRANCHES on the address: under skew the other path must give the right answer
SKEW_BRANCH = {
    "gdm_gather_max_hip": ("feat", "idx"),                                # gdm_gather.hip gather_max_rowlds_kernel: float4 staging, int4 index rows
    "gdm_group_gather_bwd2_hip": ("grad_out", "idx"),                     # gdm_gather.hip: group_gather_bwd_lds_kernel<vec>
    "gdm_att_pool_hip": ("att", "feat"),                                  # gdm_gather.hip: att_pool16_kernel or att_pool_kernel<16>
    "gdm_att_pool_bwd_hip": ("att", "feat", "grad_att", "grad_feat"),     # gdm_gather.hip: att_pool16_bwd_kernel or att_pool_bwd_kernel<16>
    "gdm_upsample_bilinear_hip": ("out",),                                # gdm_image.hip upsample_bilinear_kernel: one float4 store or four scalar ones
    "gdm_upconv3x3_gather_hip": ("out",),                                 # gdm_image.hip upconv3x3_gather(_lds)_kernel: the same choice per quad
    "gdm_feature_knn_hip": ("x",),                                        # gdm_dgcnn.hip: `vec` of the Gram tile loads
    "gdm_pointwise2_hip": ("wt",),                                        # gdm_pointwise.hip: `vec` (FMA form); the segments' x are guarded by hand
    # gdm_spline.hip: the 16-byte or the one-channel-per-thread kernel (only with the row-major `out` alone: out_t / out_packed are
    # refused off the 16-byte path)
    "gdm_spline_pairs_aggregate3_hip": ("Y", "out", "root", "bias"),
    "gdm_spline_direct3_hip": ("weight", "out", "root_t", "bias"),
}
# the launcher REFUSES an unaligned address (GDM_CHECK_ARG before any launch): with one of these 4 bytes off (guarded_calls(skew=4,
# skew_params=(name,))) `call` raises GdmError and nothing is touched.  tests/test_gpu_guard_bands.py exercises every row, parameter
# by parameter.  An entry may be in both tables with different parameters (gdm_pointwise2_hip).
SKEW_REFUSE = {
    "gdm_affine_act_hip": ("x", "y", "res"),
    "gdm_affine_act_maxk_hip": ("x",),
    "gdm_prelu1_hip": ("x", "y"),
    "gdm_prelu1_bwd_hip": ("x", "grad_out", "grad_x"),
    "gdm_psp_combine2_hip": ("g", "out", "outpk"),
    "gdm_edge_block_hip": ("pq", "scale1", "shift1", "w2"),
    # csrc/gdm_conv.hip conv_launch, behind every convolution / GEMM entry: the packed operands, the residual and the output
    "gdm_conv3x3_strided_hip": ("xpk", "wpk", "res", "out"),
    "gdm_conv1x1_strided_hip": ("xpk", "wpk", "out"),
    "gdm_conv1x1_packed_hip": ("xpk", "wpk", "out"),
    "gdm_conv1x1_packed_wb_hip": ("xpk", "wpk", "out"),
    "gdm_conv1x1_gather_add_hip": ("xpk", "wpk", "gidx", "out"),
    "gdm_gemm_grouped_hip": ("xpk", "wpk", "out"),
    "gdm_pointwise2_hip": ("out",),
    "gdm_wgrad_direct_hip": ("go", "x"),
    "gdm_knn_jobs_ws_hip": ("workspace",),
    "gdm_gather_add_affine_act2_hip": ("y_packed",),
    "gdm_match_packed_hip": ("scene_rows", "model_rows"),
    "gdm_circle_match_pack_hip": ("rows", "tp"),
    "gdm_circle_match_fwd2_hip": ("xrows", "xtp", "yrows", "ytp"),
    "gdm_circle_match_bwd2_hip": ("xrows", "xtp", "yrows", "ytp"),
    "gdm_soft_coord_fwd_hip": ("xrows", "xtp", "yrows", "ytp"),
    "gdm_edge_stats_hip": ("pq", "st1", "w2"),
    "gdm_edge_bwd_reduce_hip": ("pq", "st1", "w2"),
    "gdm_edge_bwd_mid_hip": ("pq", "st1", "w2"),
    "gdm_edge_bwd_scatter_hip": ("pq", "st1", "w2"),
    "gdm_conv1x1_gather_add_act2_hip": ("y",),                            # with pixel_major
    "gdm_conv64_gather_add_act_mfma2_hip": ("t", "y", "ypk"),             # t with t_point_major, y with pixel_major
    "gdm_conv64_gather_add_final_hip": ("t",),
    "gdm_soft_coord_bwd_hip": ("xrows", "xtp", "yrows", "ytp", "kb", "gy_part", "gy"),
    "gdm_upconv3x3_gather2_hip": ("outpk",),
    "gdm_stem_hip": ("wpk", "out_packed"),
    "gdm_bn_stats_hip": ("x",),
    "gdm_bn_fwd_apply_hip": ("x", "y"),
    "gdm_bn_bwd_reduce_hip": ("x", "grad_out"),
    "gdm_bn_bwd_apply_hip": ("x", "grad_out", "grad_x"),
    "gdm_match_pack_hip": ("rows",),
    "gdm_match_pack2_hip": ("rows1", "rows2"),
    "gdm_match_hip": ("workspace",),
    "gdm_match_soft_packed_hip": ("partial", "scene_rows", "model_rows"),
    "gdm_stem_pack_weight_hip": ("wpk",),
    "gdm_wgrad_pack_x_hip": ("out",),
    "gdm_wgrad_pack_x1_hip": ("out",),
    "gdm_wgrad_pack_go_hip": ("out", "go"),
    "gdm_spline_segment_sum_hip": ("z", "add", "dx"),
    "gdm_spline_wgrad_hip": ("part", "dw"),
    "gdm_spline_pairs_grad_hip": ("grad_out", "out_mask", "gy"),
    "gdm_hpr_visible_hip": ("workspace",),
    "gdm_pose_targets_hip": ("workspace",),
    "gdm_ransac_pose_hip": ("workspace",),
}


def _parse_header(text):
    """{entry: {pointer parameter: declared const?}} of every `*_hip` entry, read from the header text itself (_lib.PARAMS keeps
    names only).  The stream is left out: it is no memory of the caller's."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    text = re.sub(r"^\s*#[^\n]*", "", text, flags=re.M)
    table = {}
    for _ret, name, params in re.findall(r"([\w\s*]+?)\b(gdm_\w+)\s*\(([^)]*)\)\s*;", text):
        if not name.endswith("_hip"):
            continue
        ptrs = {}
        for p in params.split(","):
            ctype, pname = re.fullmatch(r"(.*?)(\w+)", p.strip(), flags=re.S).groups()
            if "*" in ctype and pname != "stream":
                ptrs[pname] = re.search(r"\bconst\b", ctype) is not None
        table[name] = ptrs
    return table


with open(_lib.HEADER) as _f:
    CONST = _parse_header(_f.read())
HIP_ENTRIES = tuple(CONST)

COUNTS = collections.Counter()          # guarded calls per entry point, over the whole process (the coverage test reads it)


class GuardViolation(AssertionError):
    """A library call touched memory it was not given.  entry / param / side ('before', 'after', 'interior') / offset: the byte
    offset of the nearest touched byte from the tensor's edge -- negative before the start, counted from the end after it, from the
    start for the interior of a const argument."""

    def __init__(self, entry, param, side, offset, nbytes, scalars=()):
        self.entry, self.param, self.side, self.offset, self.nbytes, self.scalars = entry, param, side, offset, nbytes, tuple(scalars)
        where = {"before": "%d bytes relative to its start" % offset, "after": "%d bytes past its end" % offset,
                 "interior": "byte %d of a const argument" % offset}[side]
        super().__init__("%s: `%s` touched %s the tensor, at %s (%d bytes differ); scalars: %s" %
                         (entry, param, {"interior": "inside"}.get(side, side), where, nbytes,
                          ", ".join("%s=%r" % kv for kv in self.scalars) or "-"))


def _span(t):
    """Elements from the first to one past the last element the view covers."""
    if t.numel() == 0:
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride()))


def _bytes_at(storage, device, offset, nbytes):
    return torch.empty(0, dtype=torch.uint8, device=device).set_(storage, offset, (nbytes,), (1,))


class Guarded:
    """nbytes of payload between two bands of G bytes of 0xFF; `residue` (the original address modulo 16) and `skew` go in front of
    the payload, so the bands stay multiples of 512 and the payload's address modulo 16 is residue + skew."""

    def __init__(self, nbytes, device, skew=0, residue=0, entry="guard()", param="tensor", scalars=()):
        self.lo, self.nbytes = G + residue + skew, nbytes
        self.buf = torch.full((self.lo + nbytes + G,), FILL, dtype=torch.uint8, device=device)
        self.entry, self.param, self.scalars = entry, param, scalars
        self.t = None

    def payload(self):
        return self.buf[self.lo:self.lo + self.nbytes]

    def view(self, dtype, size, stride, byte_offset=0):
        """A typed view into the payload, `byte_offset` from its start."""
        item = torch.empty(0, dtype=dtype).element_size()
        assert (self.buf.data_ptr() + self.lo + byte_offset) % item == 0, "guarded view would not be element-aligned"
        return torch.empty(0, dtype=dtype, device=self.buf.device).set_(self.buf.untyped_storage(), (self.lo + byte_offset) // item, size, stride)

    def dirty(self):
        """0-dim tensor: how many band bytes are no longer 0xFF (no synchronisation)."""
        return (self.buf[:self.lo] != FILL).sum() + (self.buf[self.lo + self.nbytes:] != FILL).sum()

    def check(self, entry=None, param=None, scalars=None):
        entry, param = entry or self.entry, param or self.param
        scalars = self.scalars if scalars is None else scalars
        bad = (self.buf[:self.lo] != FILL).nonzero().flatten()
        if bad.numel():
            raise GuardViolation(entry, param, "before", int(bad.max()) - self.lo, int(bad.numel()), scalars)
        bad = (self.buf[self.lo + self.nbytes:] != FILL).nonzero().flatten()
        if bad.numel():
            raise GuardViolation(entry, param, "after", int(bad.min()), int(bad.numel()), scalars)


def _skew_for(t, skew):
    item = t.element_size()
    return skew if skew % item == 0 else (skew + item - 1) // item * item


def guard(t, skew=0):
    """A copy of `t` (same shape and strides) between guard bands: the Guarded, whose `.t` is the typed view."""
    nbytes = _span(t) * t.element_size()
    g = Guarded(nbytes, t.device, _skew_for(t, skew), t.data_ptr() % 16 if nbytes else 0)
    g.t = g.view(t.dtype, t.shape, t.stride())
    if nbytes:
        g.payload().copy_(_bytes_at(t.untyped_storage(), t.device, t.data_ptr() - t.untyped_storage().data_ptr(), nbytes))
    return g


def guard_like(shape, dtype, skew=0, device="cuda"):
    """A contiguous tensor of `shape` between guard bands whose interior keeps the fill: an output element that is never written
    reads back as NaN (-1 for an integer type)."""
    proto = torch.empty(0, dtype=dtype)
    n = 1
    for s in shape:
        n *= s
    g = Guarded(n * proto.element_size(), torch.device(device), _skew_for(proto, skew))
    g.t = g.view(dtype, tuple(shape), torch.empty(tuple(shape), device="meta").stride())
    return g


class _Calls:
    """What guarded_calls yields: `counts` (calls per entry point in this context) and, when recording, `record`: one
    (entry, {parameter: dense copy}) per call, of every tensor argument the header does not declare const, taken after the call."""

    def __init__(self, record=False):
        self.counts = collections.Counter()
        self.refused = {}          # entry -> the error a guarded call of it raised (kept even where a caller wraps the exception)
        self.record = [] if record else None

    def keep(self, name, args):
        if self.record is not None:
            const = CONST.get(name, {})
            self.record.append((name, {p: a.detach().contiguous().clone() for p, a in zip(_lib.PARAMS[name], args)
                                       if isinstance(a, torch.Tensor) and a.numel() and not const.get(p, False)}))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def assert_same_record(a, b, skip=(), what="guarded"):
    """Two recordings of the same test body hold the same calls and, outside the entries in `skip`, the same bytes in every output."""
    assert [n for n, _ in a.record] == [n for n, _ in b.record], "the %s run made other library calls" % what
    for k, ((name, outs_a), (_, outs_b)) in enumerate(zip(a.record, b.record)):
        if name in skip:
            continue
        for p in outs_a:
            assert same_bits(outs_a[p], outs_b[p]), "call %d, %s: `%s` of the %s run differs from the plain run" % (k, name, p, what)


@contextlib.contextmanager
def filled_empties():
    """torch.empty() comes back filled (NaN / the largest integer) instead of holding whatever the allocator last had there, so
    that two runs of one body see the same bytes in what a kernel leaves unwritten (workspace tails, padding)."""
    import warnings
    was = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
           torch.utils.deterministic.fill_uninitialized_memory)
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message=".*does not have a deterministic implementation.*")
        torch.use_deterministic_algorithms(True, warn_only=True)
        torch.utils.deterministic.fill_uninitialized_memory = True
        try:
            yield
        finally:
            torch.use_deterministic_algorithms(was[0], warn_only=was[1])
            torch.utils.deterministic.fill_uninitialized_memory = was[2]


def _sync(tensors):
    if any(t.is_cuda for t in tensors):
        torch.cuda.synchronize()


def _guarded_call(target, name, args, skew, state, skew_params=None):
    params = _lib.PARAMS[name]
    const = CONST.get(name, {})
    scalars = [(p, a) for p, a in zip(params, args) if type(a) in (int, float, bool)]
    tens = [(i, a) for i, a in enumerate(args) if isinstance(a, torch.Tensor) and a.numel() > 0]
    if torch.cuda.is_available() and any(a.is_cuda for _, a in tens) and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("guarded_calls cannot be used inside hipGraph capture (%s)" % name)
    skewed = (SKEW_BRANCH.get(name, ()) if skew_params is None else tuple(skew_params)) if skew else ()
    # arguments that alias or overlap (an in-place y == x) share one copy: merge address intervals per storage
    groups = {}
    for i, a in tens:
        st = a.untyped_storage()
        groups.setdefault((str(a.device), st.data_ptr()), []).append((a.data_ptr(), a.data_ptr() + _span(a) * a.element_size(), i, a))
    unions = []          # [lo, hi, members]
    for members in groups.values():
        members.sort(key=lambda m: m[0])
        for lo, hi, i, a in members:
            if unions and unions[-1][3] is members and lo < unions[-1][1]:
                unions[-1][1] = max(unions[-1][1], hi)
                unions[-1][2].append((lo, hi, i, a))
            else:
                unions.append([lo, hi, [(lo, hi, i, a)], members])
    argv = list(args)
    placed = []          # (Guarded, original bytes, members)
    for lo, hi, members, _ in unions:
        a0 = members[0][3]
        sk = max([_skew_for(a, skew) for _, _, i, a in members if params[i] in skewed] or [0])
        g = Guarded(hi - lo, a0.device, sk, lo % 16, name, "/".join(params[i] for _, _, i, _ in members), scalars)
        orig = _bytes_at(a0.untyped_storage(), a0.device, lo - a0.untyped_storage().data_ptr(), hi - lo)
        g.payload().copy_(orig)
        for mlo, _mhi, i, a in members:
            argv[i] = g.view(a.dtype, a.shape, a.stride(), mlo - lo)
        placed.append((g, orig, members))
    all_t = [a for _, a in tens]
    try:
        ret = target(name, *argv)
    except Exception as e:
        # refused: nothing may have been launched, so every guarded buffer, interior included, is as it was
        state.refused[name] = "%s: %s" % (type(e).__name__, e)
        _sync(all_t)
        for g, orig, members in placed:
            g.check()
            diff = (g.payload() != orig).nonzero().flatten()
            if diff.numel():
                raise GuardViolation(name, g.param, "interior", int(diff.min()), int(diff.numel()), scalars)
        raise
    _sync(all_t)
    state.counts[name] += 1
    COUNTS[name] += 1
    state.keep(name, argv)
    if placed:
        if int(torch.stack([g.dirty().to("cpu") for g, _, _ in placed]).sum()):
            for g, _, _ in placed:
                g.check()
    for g, orig, members in placed:
        writable = [m for m in members if not const.get(params[m[2]], False)]
        if not writable:
            diff = (g.payload() != orig).nonzero().flatten()
            if diff.numel():
                first = int(diff.min())
                owner = next((m for m in members if m[0] - members[0][0] <= first < m[1] - members[0][0]), members[0])
                raise GuardViolation(name, params[owner[2]], "interior", first - (owner[0] - members[0][0]), int(diff.numel()), scalars)
        else:
            orig.copy_(g.payload())
    return ret


@contextlib.contextmanager
def guarded_calls(monkeypatch, skew=0, only=None, target=None, record=False, guard=True, skew_params=None):
    """Within the context every library call of the package (or only the entries named in `only`) runs on guarded copies of its
    tensor arguments.  `target(name, *args)` is what is finally called: `_lib.call`, or a stand-in for the tests of this module.
    skew_params: the parameters to move under skew instead of the entry's row of SKEW_BRANCH (the refusal tests move one at a time).
    record: keep a copy of every output of every `*_hip` call (see _Calls).  guard=False: calls go through as they are, for the
    plain recording a guarded one is compared with."""
    import importlib
    real = target or _lib.call
    state = _Calls(record)
    only = None if only is None else frozenset(only)

    def call(name, *args):
        if not name.endswith("_hip"):
            return real(name, *args)
        if not guard or (only is not None and name not in only):
            ret = real(name, *args)
            if record:
                _sync([a for a in args if isinstance(a, torch.Tensor)])
                state.keep(name, args)
            return ret
        return _guarded_call(real, name, args, skew, state, skew_params)

    with monkeypatch.context() as mp:
        for m in MODULES:
            mp.setattr(importlib.import_module("geometric_aware_dense_matching_amd." + m), "call", call)
        state.call = call
        yield state
