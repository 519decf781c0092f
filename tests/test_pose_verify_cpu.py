"""CPU: the host restatement of pose verification (pose.verify_poses_numpy, verify_select_numpy; include/gdm.h THE VERIFICATION RULE;
DESIGN.md 6q) on scenes whose answer can be worked out by hand, the selection's rules, the ranking that fixes the inputs of the GPU
end-to-end test, boxes_to_windows, and the command line's refusal."""
import numpy as np
import pytest
import torch

import verify_cases as vc
from geometric_aware_dense_matching_amd import evaluation, pose, train_lm


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_rule_at_its_exact_edges(dtype):
    """A fronto-parallel triangle at z = 1 renders exactly 1.0f.  With delta = 2^-6: 1 + delta agrees with q = 256, the next float
    above is BEHIND, 1 - delta agrees with q = 256, the next float below is FRONT; 0, -1 and NaN are NODEPTH."""
    case = vc.edge_case(dtype)
    args, kw = vc.call_args(case)
    got = pose.verify_poses_numpy(*args, **kw)
    want = vc.edge_expected(case)
    assert got["counts"].dtype == np.int32 and got["counts"].shape == (1, 1, 6)
    assert got["counts"][0, 0].tolist() == want.tolist()
    n_model, n_agree, n_front, n_behind, n_nodepth, q = want.tolist()
    assert n_model == n_agree + n_front + n_behind + n_nodepth and min(n_agree, n_front, n_behind, n_nodepth) > 100
    assert got["score"][0, 0] == (n_agree - q / 512.0) / (n_agree + n_behind + 0.25 * n_front) and got["best"].tolist() == [0]
    # one pixel column at a time: each edge value on its own
    cov = evaluation.render_depth_numpy(case["verts"], case["faces"], case["RT"][0], case["K"], vc.H, vc.W, vc.NEAR)[0]
    x = 40
    col = int((cov[:, x] > 0).sum())
    assert col > 10
    for value, cls, q1 in zip(vc.EDGE_VALUES, (1, 1, 3, 1, 2, 4, 4, 4), (0, 256, 0, 256, 0, 0, 0, 0)):
        one = pose.verify_poses_numpy(case["verts"], case["faces"], case["RT"], np.full((vc.H, vc.W), value, dtype=np.float32), case["K"],
                                      window=np.array([[x, 0, x, vc.H - 1]]), delta=vc.DELTA_EDGE, near=vc.NEAR)["counts"][0, 0]
        expect = [col, 0, 0, 0, 0, q1 * col]
        expect[cls] = col
        assert one.tolist() == expect, value


@pytest.mark.parametrize("name", vc.MIXED)
def test_counts_add_up_and_windows_clamp(name):
    case = vc.mixed_case(name)
    args, kw = vc.call_args(case)
    got = pose.verify_poses_numpy(*args, **kw)
    c = got["counts"]
    assert np.array_equal(c[..., 0], c[..., 1:5].sum(axis=-1)) and (c >= 0).all() and (c[..., 5] <= 256 * c[..., 1]).all()
    score, best = pose.verify_select_numpy(c, 0.25, 16, case["cand_valid"])
    assert np.array_equal(score, got["score"]) and np.array_equal(best, got["best"])
    if name == "n3 C5 f32 K,depth per instance":
        assert (c[1, :, 0] > 4096).all()                                   # the large triangle: more than one 64 x 64 tile
        assert (c[2, :, 0] == 1).all() and got["best"][2] == -1            # the 1 x 1 window: below min_px
        assert got["best"][0] != 0 and got["score"][0, 0] == got["score"][0].max()          # cand_valid rules the best one out
    if name == "n3 C5 f64 K,depth shared":
        assert not c[1].any() and got["best"][1] == -1 and not got["score"][1].any()        # the window misses the frame
        inside = dict(kw, window=np.array([[0, 0, 50, 79], [5, 5, 4, 4], [60, 50, 95, 79]]))
        assert np.array_equal(pose.verify_poses_numpy(*args, **inside)["counts"], c)       # the clamped window, an empty window


def test_selection_ties_validity_and_min_px():
    counts = np.zeros((4, 3, 6), dtype=np.int32)
    counts[0] = [[100, 80, 0, 20, 0, 0], [100, 80, 0, 20, 0, 0], [100, 70, 0, 30, 0, 0]]            # a tie: the lower index
    counts[1] = [[100, 50, 0, 50, 0, 0], [100, 90, 0, 10, 0, 0], [15, 15, 0, 0, 0, 0]]              # candidate 2 is below min_px
    counts[2] = [[100, 50, 0, 50, 0, 0], [100, 90, 0, 10, 0, 0], [100, 60, 0, 40, 0, 0]]            # candidate 1 is not valid
    counts[3] = [[10, 10, 0, 0, 0, 0], [100, 100, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]]                  # nobody is eligible
    valid = np.array([[1, 1, 1], [1, 1, 1], [1, 0, 1], [1, 0, 1]], dtype=bool)
    score, best = pose.verify_select_numpy(counts, 0.25, 16, valid)
    assert best.dtype == np.int32 and best.tolist() == [0, 1, 2, -1]
    assert score[1].tolist() == [0.5, 0.9, 1.0] and score[3].tolist() == [1.0, 1.0, 0.0]             # written for every candidate
    assert pose.verify_select_numpy(counts, 0.25, 0, None)[1].tolist() == [0, 2, 1, 0]
    # the tolerance edge counts a half, an occluded pixel a quarter of the denominator
    k = np.array([[[40, 20, 20, 0, 0, 256 * 20]]])
    assert pose.verify_select_numpy(k, 0.25, 16)[0][0, 0] == (20 - 10) / 25.0


def test_ranking_true_over_shifted_over_flipped():
    """What the GPU end-to-end test repeats on the device: on the unoccluded frame and on the half-occluded one the true pose scores
    strictly above the pose 3 mm off along z, which scores strictly above the flipped one."""
    args, kw = vc.call_args(vc.ranking_case())
    got = pose.verify_poses_numpy(*args, **kw)
    s = got["score"]
    print("scores (true, shifted, flipped): unoccluded %s, occluded %s" % (s[0].tolist(), s[1].tolist()))
    assert (s[:, 0] > s[:, 1]).all() and (s[:, 1] > s[:, 2]).all() and got["best"].tolist() == [0, 0]
    assert s[0, 0] == 1.0 and got["counts"][1, 0, 2] > 200 and got["counts"][0, :2, 2].sum() == 0     # occlusion is FRONT, and neutral
    assert got["counts"][0, 2, 3] > 50                                                                   # the flip is seen through


def test_boxes_to_windows():
    boxes = torch.tensor([[10.0, 20.0, 30.0, 40.0],            # inside: 20 x 20 about (20, 30) -> 25 x 25
                          [-8.0, 70.0, 12.0, 90.0],             # across the left and bottom edges
                          [200.0, 10.0, 240.0, 30.0],           # right of the frame
                          [10.5, 10.5, 11.5, 11.5]])
    w = pose.boxes_to_windows(boxes, vc.H, vc.W)
    assert w.dtype == torch.int32 and w.device == boxes.device
    assert w.tolist() == [[7, 17, 33, 43], [0, 67, 15, 79], [96, 7, 95, 33], [10, 10, 12, 12]]
    assert pose.boxes_to_windows(boxes[:1], vc.H, vc.W, pad=1.0).tolist() == [[10, 20, 30, 40]]
    assert pose.boxes_to_windows(boxes[:1].double().numpy(), 30, 20).tolist() == [[7, 17, 19, 29]]
    with pytest.raises(ValueError):
        pose.boxes_to_windows(torch.zeros(3, 5), 4, 4)


def test_pose_verify_flag_needs_rendered_frames(capsys):
    args = train_lm.build_parser().parse_args("-state=test --pose-verify --verify-delta 0.004 --verify-candidates kabsch,ransac+icp".split())
    assert args.pose_verify and args.verify_delta == 0.004 and args.verify_candidates == "kabsch,ransac+icp"
    assert not train_lm.build_parser().parse_args(["-state=test"]).pose_verify
    with pytest.raises(SystemExit, match="depth frame"):
        train_lm.main(["-state=test", "--pose-verify"])
    with pytest.raises(SystemExit, match="candidates"):
        train_lm.main("-state=test -data rendered --pose-verify --verify-candidates kabsch,magic".split())
