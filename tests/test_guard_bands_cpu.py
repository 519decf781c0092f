"""tests/guard_bands.py catches what it claims to: a stand-in `call` target (a Python function on CPU tensors) commits each kind
of violation, and each must be reported with the entry, the parameter as include/gdm.h spells it, the side and the byte offset.
No kernel runs here, and none is ever run out of bounds on the GPU as a positive control."""
import ctypes

import pytest
import torch

import guard_bands as gb
from geometric_aware_dense_matching_amd import _lib, ops

ENTRY = "gdm_group_gather_hip"          # (const float* feat, const int32_t* idx, B, C, n, m, K, float* out)
B, C, N, M, K = 2, 3, 5, 4, 2


def _flat_past(t, k):
    """The element k places past the end (k >= 0) or before the start (k < 0, from -1) of contiguous `t`, through its storage."""
    off = t.storage_offset() + (t.numel() + k if k >= 0 else k)
    return torch.empty(0, dtype=t.dtype).set_(t.untyped_storage(), off, (1,), (1,))


def _gather(feat, idx, out):
    out.copy_(torch.gather(feat.unsqueeze(2).expand(-1, -1, idx.shape[1], -1), 3,
                           idx.long().unsqueeze(1).expand(-1, feat.shape[1], -1, -1)))


def _args():
    g = torch.Generator().manual_seed(0)
    feat = torch.randn(B, C, N, generator=g)
    idx = torch.randint(0, N, (B, M, K), generator=g, dtype=torch.int32)
    out = torch.empty(B, C, M, K)
    return feat, idx, out


def _run(monkeypatch, target, feat, idx, out, skew=0):
    with gb.guarded_calls(monkeypatch, skew=skew, target=target) as calls:
        ops.call(ENTRY, feat, idx, B, C, N, M, K, out)
    return calls


def test_a_well_behaved_call_passes_and_is_counted(monkeypatch):
    feat, idx, out = _args()
    seen = {}

    def good(name, feat_g, idx_g, *rest):
        out_g = rest[-1]
        seen["ptrs"] = (feat_g.data_ptr(), out_g.data_ptr(), feat.data_ptr())
        seen["strides"] = (feat_g.stride(), out_g.stride())
        _gather(feat_g, idx_g, out_g)

    calls = _run(monkeypatch, good, feat, idx, out)
    want = torch.empty_like(out)
    _gather(feat, idx, want)
    assert torch.equal(out, want)          # the result was copied back into the caller's tensor
    assert calls.counts == {ENTRY: 1}
    assert seen["ptrs"][0] != seen["ptrs"][2] and seen["ptrs"][0] % 16 == feat.data_ptr() % 16
    assert seen["strides"] == (feat.stride(), out.stride())
    assert ops.call is _lib.call          # the patch is undone on leaving the context


def test_a_write_one_element_past_the_end_is_reported(monkeypatch):
    feat, idx, out = _args()

    def bad(name, feat_g, idx_g, *rest):
        _gather(feat_g, idx_g, rest[-1])
        _flat_past(rest[-1], 0).fill_(1.0)

    with pytest.raises(gb.GuardViolation) as e:
        _run(monkeypatch, bad, feat, idx, out)
    v = e.value
    assert (v.entry, v.param, v.side, v.offset) == (ENTRY, "out", "after", 0)
    assert ("K", K) in v.scalars and "gdm_group_gather_hip" in str(v) and "`out`" in str(v) and "n=5" in str(v)


def test_a_write_one_element_before_the_start_is_reported(monkeypatch):
    feat, idx, out = _args()

    def bad(name, feat_g, idx_g, *rest):
        _gather(feat_g, idx_g, rest[-1])
        _flat_past(rest[-1], -1).fill_(1.0)

    with pytest.raises(gb.GuardViolation) as e:
        _run(monkeypatch, bad, feat, idx, out)
    v = e.value
    # fp32 1.0 = 00 00 80 3f little-endian: all four bytes differ from 0xFF, the nearest one is the byte just before the tensor
    assert (v.entry, v.param, v.side, v.offset, v.nbytes) == (ENTRY, "out", "before", -1, 4)


def test_a_write_far_into_the_band_is_located(monkeypatch):
    feat, idx, out = _args()

    def bad(name, feat_g, idx_g, *rest):
        _flat_past(idx_g, 1000).fill_(7)

    with pytest.raises(gb.GuardViolation) as e:
        _run(monkeypatch, bad, feat, idx, out)
    assert (e.value.param, e.value.side, e.value.offset) == ("idx", "after", 4000)


def test_a_write_into_a_const_argument_is_reported(monkeypatch):
    feat, idx, out = _args()
    before = feat.clone()

    def bad(name, feat_g, idx_g, *rest):
        feat_g.view(-1)[3] = 9.0
        _gather(feat_g, idx_g, rest[-1])

    with pytest.raises(gb.GuardViolation) as e:
        _run(monkeypatch, bad, feat, idx, out)
    assert (e.value.entry, e.value.param, e.value.side, e.value.offset) == (ENTRY, "feat", "interior", 12)
    assert torch.equal(feat, before)          # the caller's tensor never saw it


def test_a_read_past_an_input_shows_as_nan_in_the_output(monkeypatch):
    """An over-read cannot be seen by the bands; what it reads is NaN (fp32) or -1 (int32), which the value comparison then meets."""
    feat, idx, out = _args()

    def bad(name, feat_g, idx_g, *rest):
        _gather(feat_g, idx_g, rest[-1])
        rest[-1].view(-1)[-1] = _flat_past(feat_g, 0)[0]
        rest[-1].view(-1)[0] = _flat_past(idx_g, -1)[0].float()

    _run(monkeypatch, bad, feat, idx, out)
    assert torch.isnan(out.view(-1)[-1]) and out.view(-1)[0] == -1.0
    assert torch.isfinite(out.view(-1)[1:-1]).all()


def test_an_in_place_pair_shares_one_copy(monkeypatch):
    x = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    s = torch.ones(3)
    seen = {}

    def inplace(name, x_g, scale, shift, res, rs, rb, planes, Cc, inner, act, slope, y_g):
        seen["same"] = x_g.data_ptr() == y_g.data_ptr()
        y_g.copy_(x_g * 2)

    with gb.guarded_calls(monkeypatch, target=inplace) as calls:
        ops.call("gdm_affine_act_hip", x, s, s, None, None, None, 6, 3, 4, 0, 0.0, x)
    assert seen["same"] and calls.counts["gdm_affine_act_hip"] == 1
    assert torch.equal(x, torch.arange(24, dtype=torch.float32).view(2, 3, 4) * 2)          # const x aliases y: written, and copied back

    def overlapping(name, x_g, scale, shift, res, rs, rb, planes, Cc, inner, act, slope, y_g):
        seen["delta"] = y_g.data_ptr() - x_g.data_ptr()
        _flat_past(y_g, 0).fill_(0.0)

    flat = torch.zeros(40)
    with pytest.raises(gb.GuardViolation) as e:
        with gb.guarded_calls(monkeypatch, target=overlapping):
            ops.call("gdm_affine_act_hip", flat[:24], s, s, None, None, None, 6, 3, 4, 0, 0.0, flat[8:32])
    assert seen["delta"] == 32 and e.value.side == "after" and e.value.offset == 0 and "y" in e.value.param.split("/")


def test_a_strided_view_keeps_its_strides_and_its_span(monkeypatch):
    """_GroupGather.backward passes a channel slice with a larger batch stride: the span it covers is copied, not numel."""
    wide = torch.arange(2 * 5 * 4, dtype=torch.float32).view(2, 5, 4)
    sl = wide[:, 1:3]
    seen = {}

    def reader(name, go, bstride, idx, *rest):
        seen["stride"], seen["equal"] = go.stride(), torch.equal(go, sl)
        rest[-1].fill_(1.0)

    g = torch.zeros(2, 2, 3)
    with gb.guarded_calls(monkeypatch, target=reader):
        ops.call("gdm_group_gather_bwd2_hip", sl, sl.stride(0), torch.zeros(2, 4, 1, dtype=torch.int32), 2, 2, 3, 4, 1, g)
    assert seen == {"stride": sl.stride(), "equal": True} and bool((g == 1).all())


def test_skew_moves_only_the_listed_arguments_and_a_refusal_leaves_everything_untouched(monkeypatch):
    x = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    s = torch.ones(3)
    y = torch.zeros(2, 3, 4)
    seen = {}

    def refuse(name, x_g, scale, *rest):
        seen["mod"] = (x_g.data_ptr() % 16, scale.data_ptr() % 16, rest[-1].data_ptr() % 16)
        raise _lib.GdmError("x must be 16-byte aligned")

    with pytest.raises(_lib.GdmError):
        with gb.guarded_calls(monkeypatch, skew=4, target=refuse, skew_params=gb.SKEW_REFUSE["gdm_affine_act_hip"]) as calls:
            ops.call("gdm_affine_act_hip", x, s, s, None, None, None, 6, 3, 4, 0, 0.0, y)
    assert seen["mod"] == ((x.data_ptr() + 4) % 16, s.data_ptr() % 16, (y.data_ptr() + 4) % 16)
    assert calls.refused == {"gdm_affine_act_hip": "GdmError: x must be 16-byte aligned"} and not calls.counts

    def refuse_late(name, x_g, scale, *rest):
        rest[-1].view(-1)[5] = 1.0000001          # "launched" something before refusing (0x3f800001: every byte but one changes)
        raise _lib.GdmError("x must be 16-byte aligned")

    with pytest.raises(gb.GuardViolation) as e:
        with gb.guarded_calls(monkeypatch, skew=4, target=refuse_late, skew_params=("x", "y")):
            ops.call("gdm_affine_act_hip", x, s, s, None, None, None, 6, 3, 4, 0, 0.0, y)
    assert (e.value.param, e.value.side, e.value.offset) == ("y", "interior", 20) and bool((y == 0).all())


def test_only_limits_the_guarded_entries(monkeypatch):
    feat, idx, out = _args()
    seen = []

    def target(name, *args):
        seen.append((name, args[0].data_ptr() == feat.data_ptr()))

    with gb.guarded_calls(monkeypatch, only=("gdm_gather_max_hip",), target=target) as calls:
        ops.call(ENTRY, feat, idx, B, C, N, M, K, out)
        ops.call("gdm_gather_max_hip", feat, idx, B, C, N, M, K, out, None)
    assert seen == [(ENTRY, True), ("gdm_gather_max_hip", False)] and calls.counts == {"gdm_gather_max_hip": 1}


def test_guard_and_guard_like_place_tensors_by_hand():
    t = torch.arange(12, dtype=torch.float32).view(3, 4)
    g = gb.guard(t, skew=4)
    assert torch.equal(g.t, t) and g.t.data_ptr() % 16 == (t.data_ptr() + 4) % 16
    g.check()
    o = gb.guard_like((2, 3), torch.float32, device="cpu")
    assert torch.isnan(o.t).all() and o.t.data_ptr() % 16 == 0
    i = gb.guard_like((5,), torch.int32, device="cpu")
    assert bool((i.t == -1).all())
    _flat_past(o.t, 2).fill_(0.0)
    with pytest.raises(gb.GuardViolation) as e:
        o.check("gdm_pointwise2_hip", "segs[0].x")
    assert (e.value.entry, e.value.param, e.value.side, e.value.offset) == ("gdm_pointwise2_hip", "segs[0].x", "after", 8)
    d = gb.guard(torch.zeros(3, dtype=torch.float64), skew=4)          # an 8-byte element cannot sit at 4 (mod 8): it moves by 8
    assert d.t.data_ptr() % 16 == 8


def test_the_constness_table_covers_every_pointer_parameter_of_every_hip_entry():
    entries = [n for n in _lib.SIGNATURES if n.endswith("_hip")]
    assert sorted(gb.CONST) == sorted(entries) and len(entries) > 100
    for name in entries:
        _res, argtypes = _lib.SIGNATURES[name]
        ptrs = {p for p, t in zip(_lib.PARAMS[name], argtypes)
                if p != "stream" and (t is ctypes.c_void_p or t is ctypes.c_char_p or hasattr(t, "contents"))}
        assert set(gb.CONST[name]) == ptrs, name
    # spot checks against the header's own text
    assert gb.CONST["gdm_group_gather_hip"] == {"feat": True, "idx": True, "out": False}
    assert gb.CONST["gdm_furthestsampling_hip"] == {"xyz": True, "temp": False, "idx": False}
    assert gb.CONST["gdm_knn_jobs_ws_hip"] == {"jobs": True, "workspace": False}


def test_the_skew_tables_name_only_entries_and_parameters_that_exist():
    for name in set(gb.SKEW_BRANCH) & set(gb.SKEW_REFUSE):
        assert not set(gb.SKEW_BRANCH[name]) & set(gb.SKEW_REFUSE[name]), name
    for table in (gb.SKEW_BRANCH, gb.SKEW_REFUSE):
        for name, params in table.items():
            assert name in gb.CONST, name
            assert params and set(params) <= set(gb.CONST[name]), (name, params)
    assert set(gb.MODULES) == {m for m in ("ops", "pose", "splinecnn", "pointops", "frontend", "targets", "matching", "pyramid", "loss")
                               if "call" in vars(__import__("geometric_aware_dense_matching_amd." + m, fromlist=["x"]))
                               and vars(__import__("geometric_aware_dense_matching_amd." + m, fromlist=["x"]))["call"] is _lib.call}
