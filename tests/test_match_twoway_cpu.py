"""CPU: the two numpy restatements of include/gdm.h's TWO-WAY RULE and CYCLE RULE (matching.match_twoway_numpy,
pose.cycle_filter_numpy) on hand-written cases, the option checks of the Python surface that need no GPU, and the planted
inlier / outlier construction the GPU filter test relies on."""
import numpy as np
import pytest
import torch

import match_twoway_cases as mc
from geometric_aware_dense_matching_amd import matching, pose


# ---- the two-way rule ---------------------------------------------------------------------------------------------------------------------
def test_twoway_numpy_ties_take_the_lowest_row_and_the_first_column():
    sim = np.array([[0.5, 0.9, 0.9, 0.1],
                    [0.7, 0.9, 0.2, 0.1],
                    [0.7, 0.3, 0.2, 0.1],
                    [0.7, 0.9, 0.9, 0.1]], np.float32)
    r = matching.match_twoway_numpy(sim, None, np.ones(4))
    assert r["best_idx"].tolist() == [1, 1, 0, 1] and r["best_sim"].tolist() == [np.float32(0.9)] * 2 + [np.float32(0.7), np.float32(0.9)]
    assert r["col_idx"].tolist() == [1, 0, 0, 0] and r["col_sim"].dtype == np.float32
    assert r["col_sim"].tolist() == [np.float32(0.7), np.float32(0.9), np.float32(0.9), np.float32(0.1)]
    # the lower duplicate masked out: the next one wins; the rows' own arg-max does not look at the mask
    r2 = matching.match_twoway_numpy(sim, None, np.array([0, 0, 1, 1]))
    assert r2["col_idx"].tolist() == [2, 3, 3, 2] and r2["best_idx"].tolist() == r["best_idx"].tolist()


def test_twoway_numpy_empty_crop_and_nan():
    sim = np.array([[0.1, np.nan, np.nan], [0.3, np.nan, 0.2], [np.nan, np.nan, 0.2]], np.float64)
    r = matching.match_twoway_numpy(sim, None, np.zeros(3))
    assert r["col_idx"].tolist() == [-1, -1, -1] and np.all(np.isneginf(r["col_sim"]))
    r = matching.match_twoway_numpy(sim, None, np.array([1, 1, 1]))
    assert r["col_idx"].tolist() == [1, -1, 1]                      # a NaN never wins; an all-NaN column has no winner
    assert r["col_sim"][0] == 0.3 and np.isneginf(r["col_sim"][1]) and r["col_sim"][2] == 0.2
    assert r["best_idx"].tolist() == [0, 0, 2] and r["best_sim"].tolist() == [0.1, 0.3, 0.2]
    r = matching.match_twoway_numpy(sim, None, np.array([1, 0, 1]))
    assert r["col_idx"].tolist() == [0, -1, 2]


def test_twoway_numpy_from_descriptors_normalises_rows_and_columns():
    rs = mc.rng("twoway cpu descriptors")
    model = rs.randn(128, 7)
    scene = np.stack([3.0 * model[:, 4], 0.5 * model[:, 2], model[:, 4] + 1e-3 * rs.randn(128)])
    r = matching.match_twoway_numpy(scene, model, np.array([1, 1, 1]))
    assert r["best_idx"].tolist() == [4, 2, 4] and abs(r["best_sim"][0] - 1) < 1e-12
    assert r["col_idx"][4] == 0 and r["col_idx"][2] == 1
    assert matching.match_twoway_numpy(scene, model, np.array([0, 1, 1]))["col_idx"][4] == 2


# ---- the cycle rule -----------------------------------------------------------------------------------------------------------------------
def test_cycle_numpy_radius_zero_is_the_mutual_best_test():
    xyz = np.array([[0, 0, 0], [0.003, 0, 0], [0.1, 0, 0], [0.003, 0, 0]], np.float32)
    best_idx = np.array([0, 0, 1, 2])
    col_idx = np.array([0, 2, 1])                                  # vertex 0 picks point 0, vertex 1 point 2, vertex 2 point 1
    mask = np.ones(4, np.uint8)
    pm, n, d2 = pose.cycle_filter_numpy(xyz, best_idx, col_idx, mask, 0.0)
    # point 3 is no mutual best (vertex 2 picks point 1) but coincides with point 1: d2 = 0 keeps it, as the rule says
    assert pm.tolist() == [1, 0, 1, 1] and n == 3 and d2.dtype == np.float32
    assert d2[0] == 0 and d2[1] == np.float32(0.003) * np.float32(0.003) and d2[2] == 0 and d2[3] == 0
    pm, n, _ = pose.cycle_filter_numpy(xyz, best_idx, col_idx, mask, 0.005)
    assert pm.tolist() == [1, 1, 1, 1] and n == 4
    pm, n, d2 = pose.cycle_filter_numpy(xyz, best_idx, col_idx, np.array([1, 0, 1, 0]), 0.005)
    assert pm.tolist() == [1, 0, 1, 0] and n == 2 and np.isposinf(d2[1]) and np.isposinf(d2[3])


def test_cycle_numpy_drops_bad_indices_and_nan():
    xyz = np.array([[0, 0, 0], [0, np.nan, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32)
    best_idx = np.array([3, 0, -1, 1, 2])                          # 3 is out of range (M = 3), -1 too
    col_idx = np.array([1, -1, 9])                                 # vertex 1 was picked by nobody; vertex 2 names a point past N
    pm, n, d2 = pose.cycle_filter_numpy(xyz, best_idx, col_idx, np.ones(5), 1.0)
    assert pm.tolist() == [0, 0, 0, 0, 0] and n == 0
    assert np.isposinf(d2[0]) and np.isnan(d2[1]) and np.isposinf(d2[2]) and np.isposinf(d2[3]) and np.isposinf(d2[4])
    for bad in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="radius"):
            pose.cycle_filter_numpy(xyz, best_idx, col_idx, np.ones(5), bad)


def test_cycle_numpy_sums_in_the_written_order():
    """d2 = ((dx*dx) + dy*dy) + dz*dz in fp32: a case where another association or a fused multiply-add gives another float."""
    f = np.float32
    x, y, z = f(0.021), f(0.075), f(0.042)
    xyz = np.array([[x, y, z], [0, 0, 0]], f)
    pm, n, d2 = pose.cycle_filter_numpy(xyz, np.array([0, 0]), np.array([1]), np.array([1, 0]), 1.0)
    want = f(f(f(x * x) + f(y * y)) + f(z * z))
    assert d2[0] == want and d2[0].tobytes() == want.tobytes()
    assert want != f(f(x * x) + f(f(y * y) + f(z * z)))                                         # the other association differs here
    assert want != f(np.float64(f(f(x * x) + f(y * y))) + np.float64(z) * np.float64(z))        # and so does a fused last step


# ---- option checks ------------------------------------------------------------------------------------------------------------------------
def _res(col=True):
    res = dict(mask=torch.ones(1, 4, dtype=torch.uint8), best_idx=torch.zeros(1, 4, dtype=torch.int32))
    if col:
        res["col_idx"] = torch.zeros(1, 3, dtype=torch.int32)
    return res


def test_estimate_poses_refuses_unknown_or_inconsistent_pair_options():
    cld, xyz = torch.zeros(1, 9, 4), torch.zeros(3, 3)
    with pytest.raises(ValueError, match="pair_filter must be"):
        pose.estimate_poses(_res(), cld, xyz, pose_opts=dict(pair_filter="mutual"))
    with pytest.raises(ValueError, match="cycle_radius is for pair_filter='cycle'"):
        pose.estimate_poses(_res(), cld, xyz, pose_opts=dict(cycle_radius=0.01))
    with pytest.raises(ValueError, match="cycle_radius is for pair_filter='cycle'"):
        pose.estimate_poses(_res(), cld, xyz, pose_opts=dict(pair_filter="none", cycle_radius=0.01))
    for bad in (-0.001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cycle_radius"):
            pose.estimate_poses(_res(), cld, xyz, pose_opts=dict(pair_filter="cycle", cycle_radius=bad))
    with pytest.raises(ValueError, match="needs col_idx"):
        pose.estimate_poses(_res(col=False), cld, xyz, pose_opts=dict(pair_filter="cycle"))
    with pytest.raises(ValueError, match="needs col_idx"):
        pose.estimate_poses_verified(_res(col=False), cld, xyz, dict(), candidates=("kabsch",), pose_opts=dict(pair_filter="cycle"))
    with pytest.raises(ValueError, match="unknown pose_opts"):
        pose.estimate_poses(_res(), cld, xyz, pose_opts=dict(pair_radius=0.01))
    with pytest.raises(ValueError, match="no col_idx"):
        pose.cycle_filter(_res(col=False), cld, 0.005)
    assert pose.CYCLE_RADIUS == 0.005


def test_twoway_and_soft_exclude_each_other():
    ep = dict(seg=torch.zeros(1, 2, 4), rgbd=torch.zeros(1, 128, 4), mesh=torch.zeros(1, 128, 3))
    soft = dict(gamma=16.0, model_xyz=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="twoway and soft exclude each other"):
        matching.match_frames(ep, soft=soft, twoway=True)
    with pytest.raises(ValueError, match="twoway and soft exclude each other"):
        matching.match_tail(ep, 1, 4, 3, soft=soft, twoway=True)


def test_train_lm_flags_parse():
    from geometric_aware_dense_matching_amd import train_lm
    a = train_lm.build_parser().parse_args(["-state", "test", "--pair-filter", "cycle", "--cycle-radius", "0.01"])
    assert a.pair_filter == "cycle" and a.cycle_radius == 0.01
    a = train_lm.build_parser().parse_args(["-state", "test"])
    assert a.pair_filter == "none" and a.cycle_radius is None


# ---- the planted construction of the GPU filter test --------------------------------------------------------------------------------------
def test_planted_filter_case_separates_exactly_on_the_cpu():
    """tests/test_gpu_match_twoway.py test 9 rests on this: with the numpy restatements alone, the construction of
    match_twoway_cases.filter_case yields pair_mask == the inlier mask at radius 0.005, every outlier's vertex picks an inlier back,
    and without the filter a quarter of the pairs are wrong."""
    c = mc.filter_case()
    B, _, N = c["scene"].shape
    assert (B, N, c["model"].shape[1]) == (2, 256, 512) and int((c["inlier"] == 0).sum()) == B * (N // 4)
    for b in range(B):
        r = matching.match_twoway_numpy(c["scene"][b].T, c["model"], np.ones(N))
        pm, n, d2 = pose.cycle_filter_numpy(c["cld"][b, :3].T, r["best_idx"], r["col_idx"], np.ones(N), 0.005)
        assert np.array_equal(pm, c["inlier"][b]) and n == N - N // 4
        assert (d2[c["inlier"][b] == 1] == 0).all() and (d2[c["inlier"][b] == 0] > 0.05 ** 2).all()
        out = np.flatnonzero(c["inlier"][b] == 0)
        assert (c["inlier"][b][r["col_idx"][r["best_idx"][out]]] == 1).all()
        # margins that carry the construction over to the kernel's arithmetic (1e-4 per similarity): the inlier's own similarity is 1,
        # an outlier's claim stays below 0.97, and every other similarity of the scene stays below 0.6
        own = r["best_sim"]
        assert (own[c["inlier"][b] == 1] > 1 - 1e-6).all() and (own[out] < 0.97).all() and (own[out] > 0.9).all()
