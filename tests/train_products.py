"""Which engine runs each of the three products of a 1x1 layer's training step (forward W.x, input gradient W^T.go, weight gradient
sum_b go.x^T), recorded without computing anything: the engines the autograd Functions of ops.py call are replaced by stubs that note
their own name and return an uninitialised tensor of the right shape, and ops.wx / ops.conv1x1_train / ops.conv1x1_train_w are driven
forward and backward over a grid of shapes.  Shared by tools/record_train_products.py (writes tests/golden/train_products.json and
train_products_fits.json) and by the tests that hold the code to those files.

A case is (entry, B, Cin, Cout, n, bias, layout); its record the four letters  forward, input gradient, weight gradient, bias gradient:
  G ops.gemm_bf16x3   P ops.pointwise   B torch.bmm   W ops.gemm_wgrad   D ops.wgrad_direct
  bias gradient:  - no bias   D from the same wgrad_direct call   F summed inside the Function   A autograd's own sum outside it
layout is that of x and of the incoming gradient: contiguous, a channel slice of a wider tensor (rows intact, another batch stride:
what the gradient of a concatenation hands over), or a pixel slice (rows of n floats at a stride above n)."""
import contextlib
import itertools
import json
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENTRIES = ("wx", "conv1x1_train", "conv1x1_train_w")
LAYOUTS = ("contiguous", "channel_slice", "pixel_slice")
SWITCHES = ("USE_MFMA_GEMM_TRAIN", "USE_POINTWISE_TRAIN", "USE_DIRECT_WGRAD")
LETTER = {"gemm_bf16x3": "G", "pointwise": "P", "torch.bmm": "B", "gemm_wgrad": "W", "wgrad_direct": "D"}
MAX_TENSOR_BYTES = 1 << 30

# (B, Cin, Cout, n) of the existing tests of tests/test_gpu_train.py that reach these entry points or their engines, and of the
# product-equality test next to them
TEST_SHAPES = [(3, 16, 24, 50), (2, 32, 32, 640), (2, 64, 64, 576), (4, 1024, 2304, 256), (2, 512, 256, 4096), (2, 256, 512, 4096),
               (2, 64, 32, 1000), (2, 256, 256, 4096), (3, 1024, 2304, 256), (1, 512, 72, 16384), (24, 1024, 2304, 256), (3, 32, 32, 65536),
               (2, 64, 128, 16384), (24, 128, 128, 4096), (2, 40, 24, 8192), (1, 8, 3, 16384), (5, 64, 64, 4128), (2, 256, 72, 16384),
               (2, 64, 64, 8192)]
# both sides of the 2 GiB line of each product (tests/test_operand_limit_cpu.py _predicate_cases): forward, input gradient, weight
# gradient, and the forward of two long images
LIMIT_SHAPES = [(32, 64, 128, 43680), (33, 64, 128, 43680), (32, 128, 64, 43680), (33, 128, 64, 43680), (42, 256, 64, 16384),
                (43, 256, 64, 16384), (2, 128, 128, 699040), (2, 128, 128, 699072)]


def synthetic_grid():
    """The synthetic grid B x Cin x Cout x n, every tensor of a case below 1 GiB."""
    return [(B, ci, co, n) for B, ci, co, n in itertools.product((1, 2, 24), (10, 32, 64, 128, 256, 1024),
                                                                 (16, 32, 64, 72, 128, 136, 192, 256, 2304), (50, 1000, 4096, 16384, 65536))
            if 4 * B * (max(ci, co) + 8) * (n + 32) < MAX_TENSOR_BYTES]


def in_asymmetry_class(B, cin, cout, n):
    """The inherited class: gemm_wgrad takes the weight gradient through ops.wx, ops.conv1x1_train never asks it."""
    return (cin % 256 == 0 and 64 <= cout < 192 and cout not in (64, 128) and n % 128 == 0 and 2.0 * B * n * cin * cout >= 2e9)


def columns(layouts=LAYOUTS):
    """(entry, bias, layout) in the order of the letters groups of a golden row."""
    return [(e, b, lay) for e in ENTRIES for b in ((False,) if e == "wx" else (False, True)) for lay in layouts]


def key(shape):
    return ",".join(str(int(v)) for v in shape)


def shape_of(k):
    return tuple(int(v) for v in k.split(","))


class _Noted(list):
    def stub(self, name, result):
        def f(*args, **kw):
            self.append((name, kw.get("bias", args[2] if name == "wgrad_direct" and len(args) > 2 else False)))
            return result(*args, **kw)
        return f


@contextlib.contextmanager
def stubbed(ops):
    """-> the list of (engine name, bias flag) calls made inside the scope; the engines are put back whatever happens."""
    noted = _Noted()

    def empty(*shape, like):
        return torch.empty(shape, dtype=torch.float32, device=like.device)

    def pointwise(segs, wt, scale=None, shift=None, act=0, slope=0.0, point_major=False, out=None, out_c0=0, w_rowmajor=False):
        x = segs[0] if isinstance(segs, list) else segs
        return out if out is not None else empty(x.shape[0], wt.shape[0] if w_rowmajor else wt.shape[1], x.shape[2], like=x)

    def bmm(a, b, out=None):
        return out if out is not None else empty(a.shape[0], a.shape[1], b.shape[2], like=b)

    def wgrad_direct(x3, go3, bias=False):
        return empty(go3.shape[1], x3.shape[1], like=x3), (empty(go3.shape[1], like=x3) if bias else None)

    stubs = [(ops, "gemm_bf16x3", lambda x, wpk, cout, *a, **k: empty(x.shape[0], cout, x.shape[2], like=x)),
             (ops, "pointwise", pointwise), (torch, "bmm", bmm),
             (ops, "gemm_wgrad", lambda x3, go3: empty(go3.shape[1], x3.shape[1], like=x3)), (ops, "wgrad_direct", wgrad_direct),
             (ops, "gemm_pack_weight", lambda w: torch.empty(16, dtype=torch.uint8, device=w.device)),
             (ops, "conv_pack_weight_dgrad", lambda w: torch.empty(16, dtype=torch.uint8, device=w.device))]
    saved = [(mod, name, getattr(mod, name)) for mod, name, _ in stubs]
    try:
        for mod, name, fn in stubs:
            setattr(mod, name, noted.stub("torch.bmm" if mod is torch else name, fn))
        yield noted
    finally:
        for mod, name, fn in saved:
            setattr(mod, name, fn)


@contextlib.contextmanager
def noting_entries(ops):
    """-> the list of [entry, B, Cin, Cout, n, bias, "module:function" of the caller] of every call of the three entry points made
    inside the scope, in call order (the entry points themselves run as they are)."""
    import sys
    calls = []
    real = {e: getattr(ops, e) for e in ENTRIES}

    def note(entry, x, cout, bias):
        f = sys._getframe(2)
        calls.append([entry, x.shape[0], x.shape[1], cout, x.numel() // max(1, x.shape[0] * x.shape[1]), bool(bias),
                      "%s:%s" % (f.f_globals.get("__name__", "?").rsplit(".", 1)[-1], f.f_code.co_name)])

    def wx(w, x):
        note("wx", x, w.shape[0], False)
        return real["wx"](w, x)

    def conv1x1_train(conv, x):
        note("conv1x1_train", x, conv.weight.shape[0], conv.bias is not None)
        return real["conv1x1_train"](conv, x)

    def conv1x1_train_w(x, w2, bias=None):
        note("conv1x1_train_w", x, w2.shape[0], bias is not None)
        return real["conv1x1_train_w"](x, w2, bias)

    try:
        ops.wx, ops.conv1x1_train, ops.conv1x1_train_w = wx, conv1x1_train, conv1x1_train_w
        yield calls
    finally:
        for e, fn in real.items():
            setattr(ops, e, fn)


def laid_out(B, C, n, layout, device):
    if layout == "contiguous":
        return torch.empty(B, C, n, device=device)
    if layout == "channel_slice":
        return torch.empty(B, C + 8, n, device=device)[:, 4:4 + C]
    return torch.empty(B, C, n + 32, device=device)[:, :, :n]


def _graph_has(fn, name, seen=None):
    seen = set() if seen is None else seen
    if fn is None or fn in seen:
        return False
    seen.add(fn)
    return type(fn).__name__ == name or any(_graph_has(nxt, name, seen) for nxt, _ in fn.next_functions)


def _one(noted, names):
    got = [c for c in noted if c[0] in names]
    assert len(got) == 1, (noted, names)
    return got[0]


def record_case(ops, entry, bias, x, go, w, b):
    """The four letters of one case.  x f32[B,Cin,n] and go f32[B,Cout,n] in the case's layout, w f32[Cout,Cin,1], b f32[Cout]; one
    forward and backward in which x alone requires a gradient, one in which the parameters alone do (ctx.needs_input_grad tells the
    backward which product to make)."""
    products = ("gemm_bf16x3", "pointwise", "torch.bmm")
    conv = torch.nn.Conv1d(w.shape[1], w.shape[0], 1, bias=bias, device="meta")

    def forward_backward(noted, of_x):
        conv.weight, conv.bias = torch.nn.Parameter(w, requires_grad=not of_x), (torch.nn.Parameter(b, requires_grad=not of_x) if bias else None)
        xin = x.detach().requires_grad_(of_x)
        del noted[:]
        if entry == "wx":
            y = ops.wx(conv.weight.view(w.shape[0], w.shape[1]), xin)
        elif entry == "conv1x1_train":
            y = ops.conv1x1_train(conv, xin)
        else:
            y = ops.conv1x1_train_w(xin, conv.weight.view(w.shape[0], w.shape[1]), conv.bias)
        assert tuple(y.shape) == tuple(go.shape), (y.shape, go.shape)
        fwd = _one(noted, products)[0]
        del noted[:]
        in_function = _graph_has(y.grad_fn, "_Conv1x1TrainBackward")
        torch.autograd.grad(y, [xin] if of_x else [conv.weight] + ([conv.bias] if bias else []), go)
        return fwd, in_function

    with stubbed(ops) as noted:
        fwd, _ = forward_backward(noted, True)
        dgrad = _one(noted, products)[0]
        fwd2, in_function = forward_backward(noted, False)
        wgrad, rode = _one(noted, ("gemm_wgrad", "wgrad_direct", "torch.bmm"))
    assert fwd == fwd2, (fwd, fwd2)
    bsrc = "-" if not bias else "D" if rode else "F" if in_function else "A"
    return LETTER[fwd] + LETTER[dgrad] + LETTER[wgrad] + bsrc


def record_shape(ops, shape, layouts=LAYOUTS, device="cuda"):
    """One golden row: the letters of every column of `shape`, separated by blanks."""
    B, cin, cout, n = shape
    w, b = torch.empty(cout, cin, 1, device=device), torch.empty(cout, device=device)
    tensors = {lay: (laid_out(B, cin, n, lay, device), laid_out(B, cout, n, lay, device)) for lay in layouts}
    return " ".join(record_case(ops, e, bias, tensors[lay][0], tensors[lay][1], w, b) for e, bias, lay in columns(layouts))


@contextlib.contextmanager
def switched_off(settings, name):
    """`name` False inside the scope ("" : every switch at its default)."""
    old = getattr(settings, name) if name else None
    try:
        if name:
            setattr(settings, name, False)
        yield
    finally:
        if name:
            setattr(settings, name, old)


def record_all(ops, settings, shapes, device="cuda"):
    """{"" or the switch that is off: {shape key: row}}: every layout at the defaults, contiguous rows with one switch off."""
    out = {}
    for name in ("",) + SWITCHES:
        with switched_off(settings, name):
            out[name] = {key(s): record_shape(ops, s, LAYOUTS if not name else LAYOUTS[:1], device) for s in shapes}
    return out


class ShapeOnly:
    """What ops.conv1x1_train_supported reads of its input, for a tensor too large to exist: fp32, on the GPU."""
    is_cuda, dtype = True, torch.float32

    def __init__(self, *shape):
        self.shape = tuple(shape)

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for v in self.shape:
            n *= v
        return n


def supported_cases():
    """(B, Cin, Cout, n, kernel size, USE_GEMM_CONV1X1_TRAIN) asked of ops.conv1x1_train_supported."""
    return [s + (k, on) for s in LIMIT_SHAPES + [(2, 256, 72, 16384), (3, 16, 24, 50)] for k in (1, 3) for on in (True, False)]


def supported(ops, settings, case):
    B, cin, cout, n, k, on = case
    old = settings.USE_GEMM_CONV1X1_TRAIN
    settings.USE_GEMM_CONV1X1_TRAIN = on
    try:
        conv = torch.nn.Conv1d(cin, cout, k, device="meta")
        return bool(ops.conv1x1_train_supported(conv, ShapeOnly(B, cin, n)))
    finally:
        settings.USE_GEMM_CONV1X1_TRAIN = old


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)
