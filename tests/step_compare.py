"""Whole training steps compared PER PARAMETER (test helper; nothing in the product imports it).

Two arms of one step (fused kernels against torch modules, captured against eager, DDP + SyncBatchNorm against plain ...) are held
to each other tensor by tensor:

    ||got_k - ref_k|| / ||ref_k||  <=  margin * noise_k          for every parameter gradient and every running statistic k

noise_k is a REFERENCE-ONLY yardstick: the module path (the four training switches off) run again on inputs moved by a relative
`delta` per element with random signs, `patterns` independent sign patterns, the largest distance per tensor.  It measures how far
this step, on this data, carries an error of size delta that entered once; nothing of the code under test goes into it.

A step is only worth comparing where it is well conditioned.  Train-mode BatchNorm amplifies any difference by 1 / sqrt(var + eps),
and a randomly initialised network on a small batch has channels with var ~ eps: `condition(model, eps)` raises eps on every
BatchNorm of BOTH arms (the kernels read bn.eps at call time).  What remains after that is the network's own non-smoothness: a
forward difference of relative size e makes a share ~e of the ReLU / LeakyReLU / max-pool elements change side, and each of them
moves a gradient by a whole term, so the gradient noise is ~sqrt(e) (measured: profiles/step_compare.md).  `resolution(noise, margin)`
says what share of the parameters is held tightly enough that a 1 % error in that single gradient is rejected, `resolution(...,
below=COARSE)` for what share a zero, doubled or mis-wired gradient is; the tests assert both.

Gradients that are analytically zero (the bias of a convolution that feeds a train-mode BatchNorm) are pure rounding residue: they
are recognised from the REFERENCE arm alone (norm below ZERO_CLASS of the median gradient norm) and held in the absolute measure
||got_k - ref_k|| / median instead.
"""
import contextlib

import numpy as np
import torch

TRAIN_FLAGS = ("USE_LOWRES_UPCONV_TRAIN", "USE_SPLIT_PSP_TRAIN", "USE_MFMA_CONV_TRAIN", "USE_FUSED_BN_TRAIN")
EXACT_FLAGS = TRAIN_FLAGS[:2]                  # fp32 re-associations of the same arithmetic
DELTA_SAME = 2.0 ** -23                        # same arithmetic, other order or route: one fp32 rounding of the inputs
DELTA_OTHER = 2.0 ** -17                       # other arithmetic: split-bf16 products (<= 3 * 2^-16 per product: |lo| <= 2^-8 |v|, residual <= 2^-16 |v|), fp64 against fp32 sums
MARGIN = 10.0                                  # the project's standing factor for "number of re-associated sums"
ZERO_CLASS = 1e-6                              # ||ref_k|| below this share of the median gradient norm: an analytically zero gradient
# Two fp32 evaluations of one tensor differ by at least a rounding of its elements whatever the inputs do: no yardstick is below it.
NOISE_FLOOR = 2.0 ** -23
# An analytically zero gradient is a cancelling sum; its residue is one fp32 rounding (6e-8) of the sum of |summands|, which for a
# bias summed over every point or pixel of the batch may be ~1e3 of the median gradient norm: 1e-4 of the median, 1e-4 of what a
# gradient wired to the wrong tensor would put there.
ZERO_FLOOR = 1e-4
RESOLVED = 1e-2                                # a bound below this rejects a 1 % error in that single tensor
COARSE = 0.5                                   # ... and below this a gradient that is zero, doubled or wired to another tensor


class Step:
    """What one step leaves behind: the loss, {name: gradient} and {name: running statistic}, in fp64."""

    def __init__(self, loss, grads, stats):
        self.loss, self.grads, self.stats = float(loss), grads, stats

    def copy(self):
        return Step(self.loss, {k: v.clone() for k, v in self.grads.items()}, {k: v.clone() for k, v in self.stats.items()})


class Noise:
    """The yardstick: per tensor the largest distance of a perturbed reference run from the reference (`grads`, `stats`, `loss`), the
    names of the zero-gradient class and the median gradient norm their absolute measure is taken against."""

    def __init__(self, grads, stats, loss, zero, scale, delta=DELTA_SAME):
        self.grads, self.stats, self.loss, self.zero, self.scale = grads, stats, float(loss), frozenset(zero), float(scale)
        self.delta = float(delta)

    def bound(self, name, margin=MARGIN):
        if name in self.zero:
            return max(margin * self.grads[name], ZERO_FLOOR)
        if name in self.grads:
            return margin * max(self.grads[name], NOISE_FLOOR)
        # A running statistic is a mean over thousands of elements: the random signs of the perturbation cancel in it (delta / sqrt(n)),
        # while an error of the class that delta stands for need not (a rounding's bias has one sign).  So a statistic's yardstick is
        # never taken below delta itself: what the same error does to a mean when it enters every element with the same sign.
        return margin * max(self.stats[name], self.delta)

    def loss_bound(self, margin=MARGIN):
        return margin * max(self.loss, NOISE_FLOOR)


def condition(model, eps):
    """Set `eps` on every BatchNorm / SyncBatchNorm of the model; returns how many.  Before a GraphedTrainStep is built: a capture
    bakes eps in."""
    n = 0
    for mod in model.modules():
        if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
            mod.eps = float(eps)
            n += 1
    return n


@contextlib.contextmanager
def switches(on=()):
    """The four training switches: those named in `on` set, the others cleared; afterwards each has the value it had before."""
    from geometric_aware_dense_matching_amd import settings
    before = {name: getattr(settings, name) for name in TRAIN_FLAGS}
    try:
        for name in TRAIN_FLAGS:
            setattr(settings, name, name in on)
        yield
    finally:
        for name, value in before.items():
            setattr(settings, name, value)


@contextlib.contextmanager
def counting(*functions):
    """{class name: number of `apply` calls} of the given autograd Functions while the block runs: which route a step took."""
    counts = {f.__name__: 0 for f in functions}
    real = {f: f.apply for f in functions}

    def counted(f):
        def apply(*args, **kw):
            counts[f.__name__] += 1
            return real[f](*args, **kw)
        return apply

    try:
        for f in functions:
            f.apply = counted(f)
        yield counts
    finally:
        for f in functions:
            del f.apply                                   # the inherited classmethod again


def _package_forward(model, batch, dev):
    from geometric_aware_dense_matching_amd import train_lm
    out, _ = train_lm.model_fn_dec(model, batch, dev)
    return out["loss"]


def run_step(model, batch, dev, seed=1, state=None, forward=None):
    """One forward + backward of `forward(model, batch, dev) -> loss` (default: train_lm.model_fn_dec) from `state` (a state dict
    to load first, so that running statistics start equal in every arm) with the dropout seed `seed` -> Step."""
    core = model.module if hasattr(model, "module") else model
    if state is not None:
        core.load_state_dict(state)
    model.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    loss = (forward or _package_forward)(model, batch, dev)
    loss.backward()
    return Step(loss.detach(),
                {k: p.grad.detach().double().clone() for k, p in core.named_parameters() if p.grad is not None},
                {k: v.detach().double().clone() for k, v in core.state_dict().items() if k.endswith(("running_mean", "running_var"))})


def freeze_pyramid(batch, dev):
    """The batch with the FFB6D variant's neighbour pyramid built once and carried along (model_fn_dec then builds none): every arm and
    every perturbed copy runs on the SAME graphs, so that moving `cld_rgb_nrm` by a rounding moves features, never a neighbour."""
    from geometric_aware_dense_matching_amd import pyramid, train_lm
    cu = train_lm.to_device(batch, dev)
    out = dict(batch)
    out.update(pyramid.build_pyramid(pyramid.cloud_from_inputs(cu["cld_rgb_nrm"]), cu["dpt_xyz"]))
    return out


@contextlib.contextmanager
def dgcnn_graphs(graphs, record):
    """The DGCNN variant's six kNN graphs held fixed (feature-space graphs differ at fp32 near-ties otherwise: a property of the
    kNN): record=True appends what the fused path's search returns to `graphs`; record=False hands them to the module path's search,
    one per call, afresh for every forward."""
    from geometric_aware_dense_matching_amd import dgcnn
    real_fused, real_knn = dgcnn.knn_fused, dgcnn.knn
    pending = []

    def recording(feat, k):
        graphs.append(real_fused(feat, k))
        return graphs[-1]

    def replaying(x, k):
        if not pending:
            pending.extend(graphs)
        return pending.pop(0)

    try:
        if record:
            dgcnn.knn_fused = recording
        else:
            dgcnn.knn = replaying
        yield
        assert record or not pending, "the module path made fewer searches than the fused path"
    finally:
        dgcnn.knn_fused, dgcnn.knn = real_fused, real_knn


def perturbed(batch, keys, delta, pattern):
    """The batch with every element of batch[k], k in keys, multiplied by 1 +- delta (signs drawn from the pattern's own generator)."""
    out = dict(batch)
    for i, k in enumerate(keys):
        x = torch.as_tensor(batch[k])
        sign = np.where(np.random.RandomState(1009 * pattern + i + 3).rand(*x.shape) < 0.5, -1.0, 1.0)
        out[k] = (x.double() * (1.0 + torch.from_numpy(sign).to(x.device) * delta)).to(x.dtype)
    return out


def median_norm(grads):
    return float(np.median([v.norm().item() for v in grads.values()]))


def zero_class(ref_grads):
    """Names of the gradients that are analytically zero, decided on the reference arm alone."""
    cut = ZERO_CLASS * median_norm(ref_grads)
    return frozenset(k for k, v in ref_grads.items() if v.norm().item() < cut)


def distances(got, ref, zero=(), scale=1.0):
    """{name: ||got - ref|| / ||ref||}, for the names in `zero` ||got - ref|| / scale."""
    out = {}
    for k, r in ref.items():
        d = (got[k].double() - r).norm().item()
        out[k] = d / scale if k in zero else d / max(r.norm().item(), 1e-300)
    return out


def noise_from(ref, runs, delta=DELTA_SAME):
    """The yardstick from a reference Step and its repetitions on inputs perturbed by `delta`."""
    zero, scale = zero_class(ref.grads), median_norm(ref.grads)
    dg = [distances(r.grads, ref.grads, zero, scale) for r in runs]
    ds = [distances(r.stats, ref.stats) for r in runs]
    g = {k: max(d[k] for d in dg) for k in ref.grads}
    s = {k: max(d[k] for d in ds) for k in ref.stats}
    loss = max(abs(r.loss - ref.loss) for r in runs) / max(abs(ref.loss), 1e-300)
    return Noise(g, s, loss, zero, scale, delta)


def noise(model, batch, dev, seed=1, delta=DELTA_SAME, patterns=4, keys=("rgb", "cld_rgb_nrm"), state=None, forward=None, buffers=()):
    """(reference Step, Noise): the module path (the four training switches off) on the batch, and on `patterns` perturbed copies.
    `buffers` names entries of `state` that are inputs too (the mesh branch reads its vertices' features from a buffer, not from the
    batch): they are moved the same way, or that branch's forward pass would see no perturbation at all.  The model is left holding
    the last perturbed copy: every later run_step must load `state` again, as every arm of a comparison does anyway."""
    ctx = switches(()) if forward is None else contextlib.nullcontext()
    assert not buffers or state is not None

    def moved(p):
        return dict(state, **perturbed(state, buffers, delta, 100 + p)) if buffers else state

    with ctx:
        ref = run_step(model, batch, dev, seed, state, forward)
        runs = [run_step(model, perturbed(batch, keys, delta, p), dev, seed, moved(p), forward) for p in range(patterns)]
    return ref, noise_from(ref, runs, delta)


SHOWN = 25


class Report:
    def __init__(self, rows, what):
        self.rows, self.what = rows, what                     # rows: (name, distance, bound)
        self.failures = [r for r in rows if not r[1] <= r[2]]
        self.ok = not self.failures

    @property
    def worst(self):
        """(distance / bound, name) of the tensor closest to, or furthest beyond, its bound."""
        return max((d / b, n) for n, d, b in self.rows)

    def __str__(self):
        """The failing tensors, the worst first; at most `SHOWN` of them (a broad failure names hundreds)."""
        head = "%s: %d of %d tensors beyond their bound" % (self.what, len(self.failures), len(self.rows))
        worst = sorted(self.failures, key=lambda r: -(r[1] / r[2] if r[2] > 0 else float("inf")))
        more = ["  ... and %d more" % (len(worst) - SHOWN)] if len(worst) > SHOWN else []
        return "\n".join([head] + ["  %-70s distance %.3e  bound %.3e" % r for r in worst[:SHOWN]] + more)


def compare(got, ref, noise, margin=MARGIN, what="step"):
    """Hold Step `got` to Step `ref` per tensor -> Report (str() names every failing tensor with its distance and bound).  A name
    missing on either side fails."""
    rows = []
    for table, ref_t, got_t, zero in (("grad", ref.grads, got.grads, noise.zero), ("stat", ref.stats, got.stats, ())):
        for k in sorted(set(ref_t) ^ set(got_t)):
            rows.append(("%s %s (missing in one arm)" % (table, k), float("inf"), 0.0))
        both = {k: v for k, v in ref_t.items() if k in got_t}
        d = distances(got_t, both, zero, noise.scale)
        rows += [(k, d[k], noise.bound(k, margin)) for k in both]
    rows.append(("loss", abs(got.loss - ref.loss) / max(abs(ref.loss), 1e-300), noise.loss_bound(margin)))
    return Report(rows, what)


def resolution(noise, margin=MARGIN, below=RESOLVED):
    """Share of the parameters whose bound is below 1e-2: a 1 % error in that single gradient is rejected.  below=COARSE: the share
    for which a gradient that is zero, doubled or another tensor's (distance 1) is rejected with a factor of two to spare."""
    return float(np.mean([noise.bound(k, margin) < below for k in noise.grads]))


def largest_bound(noise, margin=MARGIN):
    """(bound, name) of the most loosely held parameter."""
    return max((noise.bound(k, margin), k) for k in noise.grads)


def global_l2(got, ref):
    """The measure of the four older whole-step tests: one relative L2 over all parameter gradients."""
    den = sum((v ** 2).sum().item() for v in ref.values()) ** 0.5
    return sum(((got[k] - ref[k]) ** 2).sum().item() for k in ref) ** 0.5 / den
