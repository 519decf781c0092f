"""CPU: ops.train_plan -- the one place that decides which engine runs each of the three products of a 1x1 layer's training step -- gives,
from the shapes alone, every decision recorded on the GPU at the commit before it existed (tests/golden/train_products.json, written by
tools/record_train_products.py through the stubs of tests/train_products.py), and the 2 GiB answers recorded with it
(tests/golden/train_products_fits.json).  No exceptions, no skip list."""
import pytest
import torch

import train_products as tp


@pytest.fixture(scope="module")
def ops():
    from geometric_aware_dense_matching_amd import ops
    return ops


@pytest.fixture(scope="module")
def settings():
    from geometric_aware_dense_matching_amd import settings
    return settings


def planned(ops, shape, entry, bias, layout):
    """The four letters the plan predicts for a case.  Row layout is the one condition left to run time: wgrad_direct wants rows of n
    floats at stride n.  The _WxTrain route copies a gradient that is not contiguous; _Conv1x1Train reads it as it comes."""
    p = ops.train_plan(entry, *shape, cuda=True, bias_grad=bias)
    rows_ok = layout != "pixel_slice" or p.function == "_WxTrain"
    wgrad = next(e for e in p.wgrad if e != "wgrad_direct" or rows_ok)
    in_function = p.function == "_Conv1x1Train"
    bsrc = "-" if not bias else "D" if wgrad == "wgrad_direct" and in_function else "F" if in_function else "A"
    return tp.LETTER[p.fwd] + tp.LETTER[p.dgrad] + tp.LETTER[wgrad] + bsrc


def test_the_golden_grid_is_complete_and_holds_the_inherited_asymmetry():
    gold = tp.load("train_products.json")
    assert sorted(gold["rows"]) == sorted(("",) + tp.SWITCHES)
    keys = set(gold["rows"][""])
    assert all(set(rows) == keys for rows in gold["rows"].values())
    assert {tp.key(s) for s in tp.synthetic_grid() + tp.TEST_SHAPES} <= keys
    assert gold["replay_calls"] and {tp.key(c[1:5]) for c in gold["replay_calls"]} <= keys
    assert {c[0] for c in gold["replay_calls"]} == set(tp.ENTRIES)
    # members of the inherited class.  (2, 256, 72, 16384) has its shape but only 1.2 GFLOP, under the 2 GFLOP gate: it is in the grid as
    # the neighbour on which the two routes agree; (2, 256, 136, 16384), 2.3 GFLOP, is the smallest member
    assert {"2,256,72,16384", "2,256,136,16384", "24,256,72,4096"} <= keys
    assert not tp.in_asymmetry_class(2, 256, 72, 16384) and tp.in_asymmetry_class(2, 256, 136, 16384) and tp.in_asymmetry_class(24, 256, 72, 4096)
    assert sum(tp.in_asymmetry_class(*tp.shape_of(k)) for k in keys) >= 10
    cols = tp.columns()
    wx, conv = cols.index(("wx", False, "contiguous")), cols.index(("conv1x1_train", False, "contiguous"))
    for k in keys:                                             # the two routes disagree on exactly this class, at the defaults
        row = gold["rows"][""][k].split()
        assert (row[wx][2] == "W" and row[conv][2] != "W") == tp.in_asymmetry_class(*tp.shape_of(k)), (k, row)


@pytest.mark.parametrize("off", ("",) + tp.SWITCHES)
def test_the_plan_reproduces_every_recorded_decision(ops, settings, off):
    rows = tp.load("train_products.json")["rows"][off]
    cols = tp.columns(tp.LAYOUTS if not off else tp.LAYOUTS[:1])
    bad = []
    with tp.switched_off(settings, off):
        for k, row in rows.items():
            got = " ".join(planned(ops, tp.shape_of(k), *c) for c in cols)
            if got != row:
                bad.append((k, got, row))
    assert not bad, "%d of %d rows differ, first: %s" % (len(bad), len(rows), bad[:3])


def test_the_plan_needs_no_gpu_and_sends_cpu_operands_to_torch(ops):
    p = ops.train_plan("wx", 2, 256, 512, 4096, cuda=False)
    assert (p.fwd, p.dgrad, p.wgrad, p.fits) == ("torch.bmm", "torch.bmm", ("torch.bmm",), True)
    with pytest.raises(AttributeError):
        p.fwd = "pointwise"                                    # immutable


def test_fits_is_the_recorded_answer_on_both_sides_of_the_2_gib_line(ops, settings):
    gold = tp.load("train_products_fits.json")
    assert {tp.key(s) for s in tp.LIMIT_SHAPES} <= set(gold["fits"])
    for under, over in zip(tp.LIMIT_SHAPES[::2], tp.LIMIT_SHAPES[1::2]):          # each product's pair straddles the line
        assert gold["fits"][tp.key(under)] == "TT" and gold["fits"][tp.key(over)] == "FT", (under, over)
    for k, row in gold["fits"].items():
        for off, want in zip(("", "USE_MFMA_GEMM_TRAIN"), row):
            with tp.switched_off(settings, off):
                for entry in tp.ENTRIES:
                    assert ops.train_plan(entry, *tp.shape_of(k), cuda=True).fits == (want == "T"), (k, off, entry)


def test_conv1x1_train_supported_is_the_recorded_answer_past_the_limit(ops, settings):
    gold = tp.load("train_products_fits.json")["supported"]
    assert [tuple(c[:6]) for c in gold] == tp.supported_cases()
    assert any(c[6] for c in gold) and any(not c[6] and c[4] == 1 and c[5] for c in gold)
    for *case, want in gold:
        assert tp.supported(ops, settings, tuple(case)) == want, case
    # a tensor that is not on the GPU never takes the path, whatever its size (nothing is allocated: a meta tensor)
    conv = torch.nn.Conv1d(64, 128, 1, device="meta")
    assert not ops.conv1x1_train_supported(conv, torch.empty(33, 64, 43680, device="meta"))
