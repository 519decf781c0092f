"""No GPU: tests/step_compare.py proved on a plain torch stack (conv -> BatchNorm(eps 1e-6) -> ReLU -> ...), one of whose channels
is near-constant over the batch (mean thirty thousand standard deviations from zero, variance about eps) -- what the global
feature of a randomly initialised RandLA stage looks like.

  * the yardstick reports the parameters downstream of that channel as ill-conditioned, and `condition()` brings the resolution
    above the cap the GPU fixtures are held to;
  * four seeded faults in a copied gradient / statistics table are each rejected per parameter, with the parameter named -- and each
    is ACCEPTED by the older measure, one relative L2 over all gradients below 0.35: the gap the per-parameter comparison closes;
  * the zero-gradient class is found from the reference arm alone.
"""
import pytest
import torch

import step_compare as sc

DEV = torch.device("cpu")
CAP = 0.95                                     # the resolution a well-conditioned fixture is asked for
B, H, W = 4, 8, 8


class _Stack(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.conv1 = torch.nn.Conv2d(3, 6, 3, padding=1)
        self.bn1 = torch.nn.BatchNorm2d(6, eps=1e-6)
        self.conv2 = torch.nn.Conv2d(6, 6, 1)
        self.bn2 = torch.nn.BatchNorm2d(6, eps=1e-6)
        self.conv3 = torch.nn.Conv2d(6, 6, 1)                  # same shape as conv2: the pair the swap fault exchanges
        self.bn3 = torch.nn.BatchNorm2d(6, eps=1e-6)
        self.small = torch.nn.Conv2d(6, 2, 1)                  # the "small layer" with a live bias (no BatchNorm behind it)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 if p.dim() > 1 else 0.3))
            for bn in (self.bn1, self.bn2, self.bn3):
                bn.weight.add_(1.0)
            # channel 0 of the first layer passes input channel 0 through: near-constant where that input is
            self.conv1.weight[0].zero_()
            self.conv1.weight[0, 0, 1, 1] = 1.0
            self.conv1.bias[0] = 0.0

    def forward(self, x):
        x = torch.relu(self.bn1(self.conv1(x)))
        x = torch.relu(self.bn2(self.conv2(x)))
        x = torch.relu(self.bn3(self.conv3(x)))
        return self.small(x)


def _forward(model, batch, dev):
    return (torch.tanh(model(batch["x"])) * batch["w"]).mean()


def _fixture():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, H, W, generator=g)
    x[:, 0] = 30.0 + 1e-3 * torch.randn(B, H, W, generator=g)         # |mean| / std = 3e4, variance 1e-6 = eps
    batch = dict(x=x, w=torch.randn(B, 2, H, W, generator=g))
    model = _Stack().train()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    return model, batch, state


@pytest.fixture(scope="module")
def conditioned():
    """The conditioned step: the reference Step and its yardstick, computed once and left unchanged."""
    model, batch, state = _fixture()
    sc.condition(model, 1e-2)
    ref, nz = sc.noise(model, batch, DEV, state=state, keys=("x",), forward=_forward)
    return model, ref, nz


def test_condition_sets_eps_on_every_batchnorm_and_on_syncbatchnorm():
    model = torch.nn.Sequential(torch.nn.BatchNorm1d(3), torch.nn.Sequential(torch.nn.BatchNorm2d(3, eps=1e-6), torch.nn.SyncBatchNorm(3)),
                                torch.nn.Conv2d(3, 3, 1))
    assert sc.condition(model, 1e-3) == 3
    assert [m.eps for m in model.modules() if hasattr(m, "eps")] == [1e-3] * 3


def test_yardstick_reports_the_near_constant_channel_and_condition_cures_it(conditioned):
    model, batch, state = _fixture()
    _, raw = sc.noise(model, batch, DEV, state=state, keys=("x",), forward=_forward)
    print("unconditioned: resolution %.2f, largest bound %.2e at %s" % ((sc.resolution(raw),) + sc.largest_bound(raw)))
    # everything behind bn1's channel 0 (and, through the backward pass, bn1 and conv1 themselves) is ill-conditioned
    for k in ("conv2.weight", "bn2.weight", "conv3.weight", "small.weight", "bn1.weight", "conv1.weight"):
        assert raw.bound(k) > sc.RESOLVED, (k, raw.bound(k))
    assert sc.resolution(raw) < 0.5
    _, _, nz = conditioned
    print("conditioned:   resolution %.2f, largest bound %.2e at %s" % ((sc.resolution(nz),) + sc.largest_bound(nz)))
    assert sc.resolution(nz) >= CAP and sc.largest_bound(nz)[0] <= 0.1


def test_zero_gradient_class_is_found_from_the_reference_arm_only(conditioned):
    _, ref, nz = conditioned
    # the bias of a convolution that feeds a train-mode BatchNorm has an analytically zero gradient
    assert nz.zero == {"conv1.bias", "conv2.bias", "conv3.bias"}
    assert nz.zero == sc.zero_class(ref.grads)
    got = ref.copy()
    for k in nz.zero:                                       # whatever the other arm holds there does not change the class ...
        got.grads[k] = got.grads[k] + nz.scale
    rep = sc.compare(got, ref, nz)
    assert sorted(r[0] for r in rep.failures) == sorted(nz.zero)      # ... and is held in the absolute measure against the median
    got = ref.copy()
    for k in nz.zero:
        got.grads[k] = got.grads[k] + 1e-6 * nz.scale
    assert sc.compare(got, ref, nz).ok


def test_a_step_equals_itself_and_a_rounding_sized_difference_passes(conditioned):
    model, ref, nz = conditioned
    _, batch, state = _fixture()
    again = sc.run_step(model, batch, DEV, state=state, forward=_forward)
    rep = sc.compare(again, ref, nz)
    assert rep.ok, str(rep)
    moved = sc.run_step(model, sc.perturbed(batch, ("x",), sc.DELTA_SAME, 17), DEV, state=state, forward=_forward)   # a pattern the yardstick has not seen
    rep = sc.compare(moved, ref, nz)
    assert rep.ok, str(rep)


def _bias_zeroed(step, n):
    step.grads["small.bias"] = torch.zeros_like(step.grads["small.bias"])
    return "small.bias"


def _weight_doubled(step, n):
    step.grads["bn2.weight"] = 2.0 * step.grads["bn2.weight"]
    return "bn2.weight"


def _swapped(step, n):
    step.grads["conv2.weight"], step.grads["conv3.weight"] = step.grads["conv3.weight"], step.grads["conv2.weight"]
    return "conv2.weight"


def _count_plus_one(step, n):
    # bn2's statistics with a count of n + 1: mean = sum / (n + 1); unbiased variance = (sum of squares - (n + 1) mean^2) / n.
    # From fresh buffers (0, 1) with momentum 0.1 the batch part of each buffer is (running - 0.9 * initial) / 0.1.
    mean = step.stats["bn2.running_mean"] / 0.1
    var = (step.stats["bn2.running_var"] - 0.9) / 0.1 * (n - 1) / n                 # biased variance of the batch
    ssq = (var + mean ** 2) * n
    mean1 = mean * n / (n + 1)
    step.stats["bn2.running_mean"] = 0.1 * mean1
    step.stats["bn2.running_var"] = 0.9 + 0.1 * (ssq - (n + 1) * mean1 ** 2) / n
    return "bn2.running_mean"


@pytest.mark.parametrize("fault", [_bias_zeroed, _weight_doubled, _swapped, _count_plus_one])
def test_seeded_fault_is_rejected_per_parameter_and_accepted_by_the_global_bound(conditioned, fault):
    _, ref, nz = conditioned
    got = ref.copy()
    name = fault(got, B * H * W)
    rep = sc.compare(got, ref, nz)
    print(rep)
    assert not rep.ok and name in [r[0] for r in rep.failures] and name in str(rep)
    assert all(r[0].split(".")[0] in name or r[0] in ("conv3.weight", "bn2.running_var") for r in rep.failures)    # and nothing else is blamed
    # the older whole-step tests: one relative L2 over all gradients < 0.35, running variances to rtol 5e-2 -- all four faults pass
    d = sc.global_l2(got.grads, ref.grads)
    print("global relative L2 %.3e" % d)
    assert d < 0.35
    for k in ref.stats:
        if k.endswith("running_var"):
            assert torch.allclose(got.stats[k], ref.stats[k], rtol=5e-2, atol=1e-3), k


def test_a_gradient_missing_in_one_arm_fails_by_name(conditioned):
    _, ref, nz = conditioned
    got = ref.copy()
    del got.grads["small.bias"]
    rep = sc.compare(got, ref, nz)
    assert not rep.ok and "small.bias" in str(rep)
