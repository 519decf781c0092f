"""The two pruning rules of the kNN kernels, restated in float32 numpy (tests/knn_prune_model.py), against brute force
(oracle.knn.knn_batch) on the adversarial cases of tests/knn_adversarial_cases.py.  No GPU: this is the argument "an fp32 lower
bound with a 0.1 % margin never skips a neighbour" made executable; tests/test_gpu_knn_adversarial.py holds the kernels themselves
to the same oracle on the same cases.

Three kinds of check: the model's (d2, index) keys equal the oracle's bit for bit; the cases REACH the rules (a search that walks
the whole grid proves nothing about the exit test); and the cases can SEE a rule that is off (a perturbed model must disagree with
the oracle on a named case)."""
import functools

import numpy as np
import pytest

import knn_adversarial_cases as kc
import knn_prune_model as pm

# the searches no rule prunes: below KC_MIN_S = 1024 points (knn_wave_kernel), and a 7-row grid (is_grid_job declines it)
EXHAUSTIVE = {n for n in kc.NAMES if n.startswith("sizes_1023_")} | {"grid_7x40"}
MODEL_KS = (16, 32)                                       # K = 1 has no pruned form (knn_kernel<1> is exhaustive)


@functools.lru_cache(maxsize=None)
def run_model(name, K, params=pm.KERNEL):
    """Per crop: (form, result dict) of the model on a case."""
    c = kc.make(name)
    return [pm.search(c.sup[b], c.qry[b], K, c.W, params) for b in range(kc.B)]


def mismatches(name, K, params=pm.KERNEL):
    """Queries of a case (all crops) whose model keys differ from the oracle's in any bit of any index or distance."""
    widx, wd2 = kc.want(name, K)
    n = 0
    for b, (form, res) in enumerate(run_model(name, K, params)):
        if form is None:
            continue
        idx, d2 = pm.keys_to_outputs(res["keys"])
        n += int(((idx != widx[b]).any(axis=1) | (d2.view(np.uint32) != wd2[b].view(np.uint32)).any(axis=1)).sum())
    return n


@pytest.mark.parametrize("K", MODEL_KS)
@pytest.mark.parametrize("name", kc.NAMES)
def test_model_equals_oracle_and_reaches_the_rule(name, K):
    """Correctness: the keys the restated rule ends with are the oracle's, indices and d2 bit for bit, in every crop.
    Coverage: in an unorganised case the exit test fires before the window is the whole grid for at least half of the queries; in
    an organised case the window is smaller than the grid for at least half (off_axis: a tenth).  Exempt are the degenerate axes
    (cell width 0: the edge distance is 0 and the walk always ends at the whole grid) and edge_race with K = 32 (its configurations
    hold 17 points a level: the 32nd neighbour is ten box sides away)."""
    c = kc.make(name)
    res = run_model(name, K)
    forms = {form for form, _ in res}
    assert forms == ({None} if name in EXHAUSTIVE else {"grid" if c.W else "cells"}), forms
    assert mismatches(name, K) == 0
    if name in EXHAUSTIVE:
        return
    if c.W:
        pruned = np.concatenate([r["pruned"] for _, r in res])
        print("%s K=%d: window below the grid for %.0f %% of %d queries" % (name, K, 100 * pruned.mean(), pruned.size))
        assert pruned.mean() >= c.min_pruned
    else:
        early = np.concatenate([r["early"] for _, r in res])
        print("%s K=%d: early exit for %.0f %% of %d queries" % (name, K, 100 * early.mean(), early.size))
        if not c.degenerate and not (name == "edge_race" and K != 16):
            assert early.mean() >= 0.5


def test_edge_race_has_both_outcomes_and_both_windows():
    """The outside point is among the oracle's K for some configurations and not for others, in every crop and for both windows;
    the 3 x 3 configurations do not exit on the first ring and the 5 x 5 ones walk three (15 points, no K-th distance; the race;
    the exit)."""
    c = kc.make("edge_race")
    widx, _ = kc.want("edge_race", 16)
    ring2 = c.info["ring2"]
    for b, (_, r) in enumerate(run_model("edge_race", 16)):
        among = (widx[b] == c.info["outside"][b][:, None]).any(axis=1)
        for part in (among[:ring2.start], among[ring2]):
            assert part.any() and not part.all()
        assert (r["rings"][ring2] == 3).all() and np.isinf(r["td"][0][ring2]).all()
        assert (r["rings"][:ring2.start] >= 1).all() and (r["rings"][:ring2.start] == 2).any()
        assert r["early"].all()


def test_hole_race_has_both_branches_and_both_outcomes():
    """Among the queries that race: the |q|^2 test fires for some and not for others, and the oracle has a hole among the K for
    some and not for others -- in every crop."""
    c = kc.make("hole_race")
    widx, _ = kc.want("hole_race", 16)
    race = c.info["race"]
    for b, (_, r) in enumerate(run_model("hole_race", 16)):
        hole = (c.sup[b] == 0).all(axis=1)
        among = hole[widx[b]].any(axis=1)[race]
        fired = r["holes_matter"][race]
        assert among.any() and not among.all()
        assert fired.any() and not fired.all()
        assert not (among & ~fired).any()                 # a hole among the K with the window not widened: only by luck right


def test_cases_are_what_their_names_say():
    """The constructions hit the code paths they are for: an overfull cell (a row of the window with more than 64 new points), cell
    width 0 on the degenerate axis, both grids at the switch-over size, ranges with lo == hi, empty ranges, unstructured queries,
    points whose cell coordinate is exactly 0, an integer, and G."""
    for b in range(kc.B):
        sup = kc.make("heavy_cell").sup[b]
        bx0, by0, cw, ch, icw, ich = pm.cells_box(sup, 16)
        cell = pm.cell_coord(sup[:, 1], by0, ich, 16) * 16 + pm.cell_coord(sup[:, 0], bx0, icw, 16)
        assert np.bincount(cell, minlength=256).max() >= 1024
        assert pm.cells_box(kc.make("line_x").sup[b], 16)[2] == 0 and pm.cells_box(kc.make("line_y").sup[b], 16)[3] == 0
        lo, hi, rlo, rhi, bad, hole = pm.grid_ranges(kc.make("dead_lines").sup[b], kc.make("dead_lines").W)
        assert not bad and hole and (lo > hi).sum() >= 3 and (rlo > rhi).sum() >= 2
        lo, hi, rlo, rhi, bad, hole = pm.grid_ranges(kc.make("flat_wall").sup[b], kc.make("flat_wall").W)
        assert np.array_equal(lo, hi) and not bad and not hole
        sup = kc.make("edge_points").sup[b]
        bx0, by0, cw, ch, icw, ich = pm.cells_box(sup, 16)
        f = (sup[:, 0] - bx0) * icw
        inner = (f > 0.5) & (f < 15.5)
        assert (f == 0).any() and (f >= 16).any()
        if b == 0:                                        # the unit box: n / 16 is exact
            assert ((f == np.trunc(f)) & inner).any()
        off = (f - np.round(f))[inner]                    # elsewhere the edges round: points a hair on either side of them
        assert ((off > 0) & (off < 1e-3)).any() and ((off < 0) & (off > -1e-3)).any()
    assert pm.kc_grid(8191) == 16 and pm.kc_grid(8192) == 32
    assert run_model("sizes_8191_sheet", 16)[0][1]["G"] == 16 and run_model("sizes_8192_sheet", 16)[0][1]["G"] == 32
    st = np.concatenate([r["structured"] for _, r in run_model("qz_nonpositive", 16)])
    assert 0.2 < (~st).mean() < 0.3


PERTURBATIONS = {
    "factor 1.02": (pm.PruneParams(factor=1.02), "edge_race"),
    "slack 0": (pm.PruneParams(slack=0.0), "ulp_wall"),
    "cell_coord rounds up": (pm.PruneParams(cell_round_up=True), "edge_points"),
    "hole test removed": (pm.PruneParams(hole_test=False), "hole_race"),
}


@pytest.mark.parametrize("what", sorted(PERTURBATIONS))
def test_a_perturbed_rule_is_caught(what):
    """Perturbations of the MODEL, not of the kernel: each must make a named case disagree with the oracle, else the cases could
    not tell a rule that is off by that much from one that is right.  Caught by (K = 16; queries that then differ, of the case's):
      * factor 1.02 instead of 0.999 -> edge_race (the exit fires with the outside point still unseen); also offset_sheet_2p20,
        edge_points, hole_race, dead_lines, grid_8x8, the scales and wide_fov.
      * slack 0 -> ulp_wall ONLY (pixel pitch of 1 to 3 ulps: a column's bound is off by more than the distance to the next
        column).  No map with an ordinary pitch sees it, which is why the case exists.
      * cell_coord rounding up -> edge_points (points on integer cell coordinates change cell, the edges do not move).
      * the hole test removed -> hole_race (dead border columns / rows hold the origin points the K come from); also dead_lines."""
    params, name = PERTURBATIONS[what]
    n = mismatches(name, 16, params)
    print("%s: %d queries of %s differ from the oracle" % (what, n, name))
    assert n > 0
