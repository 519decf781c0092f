"""The derived-parameter cache (geometric_aware_dense_matching_amd/derived.py): its staleness rule on plain tensors, and every
call site that computes its value with torch alone -- warm it, change one dependency in place, and require the value a cold twin
built from the modified state_dict computes.  Host logic only: no GPU, no library."""
import copy

import pytest
import torch
import torch.nn as nn

from geometric_aware_dense_matching_amd import layers, ops
from geometric_aware_dense_matching_amd.cnn import PSPModule, PSPUpsample
from geometric_aware_dense_matching_amd.derived import derived, invalidate
from geometric_aware_dense_matching_amd.ffb6d import FFB6DEmb
from geometric_aware_dense_matching_amd.randla import BuildingBlock
from geometric_aware_dense_matching_amd.splinecnn import SplineConv


class _Counted:
    """make() that counts its calls and records the autograd mode it ran under."""

    def __init__(self, fn):
        self.fn, self.calls, self.grad_modes = fn, 0, []

    def __call__(self):
        self.calls += 1
        self.grad_modes.append(torch.is_grad_enabled())
        return self.fn()


# ---------------------------------------------------------------------------------------------- the helper on plain tensors
def test_hit_returns_the_same_object_without_calling_make():
    owner, t = nn.Module(), torch.arange(4.0)
    make = _Counted(lambda: t * 2)
    first = derived(owner, "x", (t,), make)
    assert derived(owner, "x", (t,), make) is first and make.calls == 1
    assert torch.equal(first, torch.arange(4.0) * 2)


def test_miss_after_in_place_change_under_no_grad():
    owner, t = nn.Module(), nn.Parameter(torch.arange(4.0))
    make = _Counted(lambda: t * 2)
    derived(owner, "x", (t,), make)
    with torch.no_grad():
        t.add_(1)
    assert torch.equal(derived(owner, "x", (t,), make), (torch.arange(4.0) + 1) * 2) and make.calls == 2


def test_miss_after_storage_replaced():
    owner, t = nn.Module(), nn.Parameter(torch.arange(4.0))
    make = _Counted(lambda: t * 2)
    derived(owner, "x", (t,), make)
    t.data = t.data.clone()
    derived(owner, "x", (t,), make)
    assert make.calls == 2


def test_miss_for_another_object_with_the_same_version_and_address():
    owner, a = nn.Module(), torch.arange(4.0)
    b = a.detach()
    assert b is not a and b._version == a._version and b.data_ptr() == a.data_ptr()      # the premise: only identity tells them apart
    make = _Counted(lambda: None)
    derived(owner, "x", (a,), make)
    derived(owner, "x", (b,), make)
    assert make.calls == 2
    derived(owner, "x", (b,), make)
    assert make.calls == 2


def test_miss_when_extra_changes():
    owner, t = nn.Module(), torch.arange(4.0)
    make = _Counted(lambda: None)
    derived(owner, "x", (t,), make, extra=(1, torch.device("cpu")))
    derived(owner, "x", (t,), make, extra=(1, torch.device("cpu")))
    assert make.calls == 1
    derived(owner, "x", (t,), make, extra=(2, torch.device("cpu")))
    assert make.calls == 2


def test_none_is_cached_and_make_runs_without_autograd():
    owner, t = nn.Module(), nn.Parameter(torch.arange(4.0))
    make = _Counted(lambda: None)
    assert torch.is_grad_enabled()
    assert derived(owner, "x", (t,), make) is None and derived(owner, "x", (t,), make) is None
    assert make.calls == 1 and make.grad_modes == [False]


def test_slots_and_owners_are_independent():
    a, b, t = nn.Module(), nn.Module(), torch.arange(4.0)
    assert derived(a, "x", (t,), lambda: 1) == 1 and derived(a, "y", (t,), lambda: 2) == 2 and derived(b, "x", (t,), lambda: 3) == 3
    assert derived(a, "x", (t,), lambda: 0) == 1 and derived(a, "y", (t,), lambda: 0) == 2 and derived(b, "x", (t,), lambda: 0) == 3


def test_tensor_owner_does_not_reference_itself():
    w = torch.arange(4.0)
    make = _Counted(lambda: w + 1)
    first = derived(w, "x", (w,), make)
    assert derived(w, "x", (w,), make) is first and make.calls == 1
    assert all(held is None for held in w.__dict__["_gdm_derived"]["x"][0])               # no cycle: the cache dies with the tensor


def test_invalidate_empties_a_module_tree_and_its_parameters():
    net = nn.Sequential(layers.pt_conv2d(4, 4, bn=True), nn.Sequential(nn.Conv2d(4, 4, 1)))
    conv = net[1][0]
    layers.folded_bn(net[0].normlayer.bn)
    net[0]._pointwise_params()
    wt = ops._final_weight_t(conv.weight)                                                  # this one is owned by the parameter
    assert ops._final_weight_t(conv.weight) is wt
    holders = [m for m in net.modules() if "_gdm_derived" in m.__dict__] + [p for p in net.parameters() if "_gdm_derived" in p.__dict__]
    assert len(holders) == 3
    invalidate(net)
    assert not any("_gdm_derived" in h.__dict__ for h in list(net.modules()) + list(net.parameters()))
    assert ops._final_weight_t(conv.weight) is not wt


def test_state_dict_of_a_warm_module_has_the_cold_keys():
    torch.manual_seed(0)
    warm, cold = layers.pt_conv1d(4, 6, bn=True), layers.pt_conv1d(4, 6, bn=True)
    warm._pointwise_params()
    layers.folded_bn(warm.normlayer.bn)
    assert list(warm.state_dict().keys()) == list(cold.state_dict().keys())
    cold.load_state_dict(warm.state_dict())


def test_deepcopy_of_a_warm_module_serves_its_own_values():
    torch.manual_seed(0)
    m = layers.pt_conv1d(4, 6, bn=True)
    warm = _snapshot(m._pointwise_params())
    c = copy.deepcopy(m)
    assert _same(c._pointwise_params(), warm)
    with torch.no_grad():
        c.conv.weight.add_(0.5)
        c.normlayer.bn.running_mean.add_(0.25)
    twin = layers.pt_conv1d(4, 6, bn=True)
    twin.load_state_dict(c.state_dict())
    assert _same(c._pointwise_params(), twin._pointwise_params())
    assert not _same(c._pointwise_params(), warm) and _same(m._pointwise_params(), warm)


def test_data_write_is_the_documented_hole_and_invalidate_closes_it():
    net = nn.Sequential(nn.Linear(3, 3))
    w = net[0].weight
    make = _Counted(lambda: w * 2)
    stale = derived(net[0], "x", (w,), make)
    version, ptr = w._version, w.data_ptr()
    w.data.mul_(2)
    assert (w._version, w.data_ptr()) == (version, ptr)                                    # why the rule cannot see it
    assert derived(net[0], "x", (w,), make) is stale and make.calls == 1
    invalidate(net)
    assert torch.equal(derived(net[0], "x", (w,), make), w.detach() * 2) and make.calls == 2


# ---------------------------------------------------------------------------------------------- every site that needs no library
def _tensors(v):
    if torch.is_tensor(v):
        return [v]
    if isinstance(v, dict):
        return [t for k in sorted(v) for t in _tensors(v[k])]
    if isinstance(v, (list, tuple)):
        return [t for x in v for t in _tensors(x)]
    return []


def _snapshot(v):
    if torch.is_tensor(v):
        return v.clone()
    if isinstance(v, dict):
        return {k: _snapshot(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_snapshot(x) for x in v)
    return v


def _same(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _residual_pair():
    return nn.ModuleDict(dict(main=layers.rl_conv2d(5, 6, bn=True, activation=None), other=layers.rl_conv2d(3, 6, bn=True, activation=None)))


_BN = ["weight", "bias", "running_mean", "running_var"]
_LFA_LAYERS = ["mlp1", "mlp2", "att_pooling_1.mlp", "att_pooling_2.mlp"]

# name -> (build the module, the call under test, the state_dict names of every dependency)
SITES = {
    "folded_bn": (lambda: nn.BatchNorm2d(5), layers.folded_bn, _BN),
    "folded_bn+conv_bias": (lambda: nn.Sequential(nn.Conv2d(3, 5, 1), nn.BatchNorm2d(5)), lambda m: layers.folded_bn(m[1], m[0].bias),
                            ["0.bias"] + ["1." + n for n in _BN]),
    "act_code": (lambda: nn.PReLU(), layers.act_code, ["weight"]),
    "pointwise_params/pt+bn": (lambda: layers.pt_conv1d(4, 6, bn=True), lambda m: m._pointwise_params(),
                               ["conv.weight"] + ["normlayer.bn." + n for n in _BN]),
    "pointwise_params/pt": (lambda: layers.pt_conv1d(4, 6, bn=False), lambda m: m._pointwise_params(), ["conv.weight", "conv.bias"]),
    "pointwise_params/rl+bn": (lambda: layers.rl_conv2d(4, 6, bn=True), lambda m: m._pointwise_params(),
                               ["conv.weight"] + ["bn.bn." + n for n in _BN]),
    "pointwise_params/rl": (lambda: layers.rl_conv2d(4, 6, bn=False), lambda m: m._pointwise_params(), ["conv.weight", "conv.bias"]),
    "residual_params": (_residual_pair, lambda m: m["main"]._residual_params(m["other"]),
                        [p + n for p in ("main.", "other.") for n in ["conv.weight"] + ["bn.bn." + b for b in _BN]]),
    "split_fuse_weight": (lambda: layers.pt_conv2d(10, 6, bn=True), lambda m: FFB6DEmb._split_fuse_weight(m, 4), ["conv.weight"]),
    "fuse_weight_t": (lambda: layers.pt_conv2d(10, 6, bn=True),
                      lambda m: [FFB6DEmb._fuse_weight_t(m, w, tag) for w, tag in zip(FFB6DEmb._split_fuse_weight(m, 4), "ab")], ["conv.weight"]),
    "psp_split_weights": (lambda: PSPModule(4, 6), lambda m: m._split_weights(), ["bottleneck.weight"] + ["stages.%d.1.weight" % k for k in range(4)]),
    "psp_split_weights_t": (lambda: PSPModule(4, 6), lambda m: m._split_weights_t(m._split_weights()[0]),
                            ["bottleneck.weight"] + ["stages.%d.1.weight" % k for k in range(4)]),
    "tap_major_weight": (lambda: PSPUpsample(3, 5), lambda m: m._tap_major_weight(), ["conv.1.weight"]),
    "lfa_fused_weights": (lambda: BuildingBlock(8), lambda m: m._fused_weights(),
                          ["att_pooling_1.fc.weight", "att_pooling_2.fc.weight"] + [l + ".conv.weight" for l in _LFA_LAYERS]
                          + [l + ".bn.bn." + n for l in _LFA_LAYERS for n in _BN]),
    "spline_root_t": (lambda: SplineConv(3, 5), lambda m: m._root_t(), ["lin.weight"]),
}


def _randomised(build, seed):
    """A module whose every tensor is off its initial value (BN statistics included; variances stay positive)."""
    m = build().eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in list(m.named_parameters()) + list(m.named_buffers()):
            if name.endswith("running_var"):
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
            elif t.is_floating_point():
                t.copy_(torch.randn(t.shape, generator=g))
    return m


@pytest.mark.parametrize("site,dep", [(s, d) for s, (_, _, deps) in SITES.items() for d in deps])
def test_site_follows_an_in_place_change_of_each_dependency(site, dep):
    build, call, _ = SITES[site]
    m = _randomised(build, seed=1)
    first = call(m)
    again = call(m)
    assert all(a is b for a, b in zip(_tensors(first), _tensors(again))) and _same(first, again)      # warm: the second call is a hit
    warm = _snapshot(first)
    t = dict(list(m.named_parameters()) + list(m.named_buffers()))[dep]
    with torch.no_grad():
        t.mul_(1.5) if dep.endswith("running_var") else t.add_(0.25)
    twin = build().eval()
    twin.load_state_dict(m.state_dict())
    got = call(m)
    assert _same(got, call(twin)), "stale value after %s changed" % dep
    assert not _same(got, warm), "%s does not reach the value: the case proves nothing" % dep


def test_every_site_dependency_list_is_complete():
    """The parametrisation above names every floating-point tensor of each site's module that its value depends on: changing any OTHER
    tensor leaves the value as it was (so no dependency is missing from the lists, and none of the cases is vacuous)."""
    for site, (build, call, deps) in SITES.items():
        m = _randomised(build, seed=2)
        warm = _snapshot(call(m))
        with torch.no_grad():
            for name, t in list(m.named_parameters()) + list(m.named_buffers()):
                if name not in deps and t.is_floating_point():
                    t.add_(0.25)
        twin = build().eval()
        twin.load_state_dict(m.state_dict())
        assert _same(call(twin), warm), site
