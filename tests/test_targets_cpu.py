"""CPU: the documented arithmetic of the ground-truth targets (include/gdm.h gdm_hpr_visible_hip) against the golden vectors of the
real reference (tests/golden/make_golden_targets.py), and the host-side argument checks of the new entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch

from geometric_aware_dense_matching_amd import targets

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(G, "pose_targets.npz")))


@pytest.fixture(scope="module")
def lib():
    from geometric_aware_dense_matching_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.mark.parametrize("c", ["b", "e"])
def test_flip_formula_is_bit_equal_to_reference(gold, c):
    """(2 ((Rad - n) p)) / n + p in fp64 with fp32 p, n and Rad = fp64(max n) * 10^pi == the reference's sphericalFlip."""
    f = targets.spherical_flip(gold[c + "_model"], gold[c + "_inv_t"][0])
    assert f.dtype == np.float64 and np.array_equal(f, gold[c + "_flipped0"])
    assert targets.HPR_PARAM == 1385.4557313670107


def test_default_centre_formula(gold):
    """fp32(-R^T t) with fp64 sums in the documented order; within one fp32 ulp of the reference's LAPACK inverse."""
    for c in "abcdef":
        RT = gold[c + "_RT"]
        got = targets.default_cam_center(RT)
        for b in range(RT.shape[0]):
            R, t = RT[b, :, :3].astype(np.float64), RT[b, :, 3].astype(np.float64)
            want = np.array([-((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2]) for k in range(3)]).astype(np.float32)
            assert np.array_equal(got[b], want)
            ref = gold[c + "_inv_t"][b]
            assert (np.abs(got[b] - ref) <= np.spacing(np.abs(ref)) * 2).all(), (c, b, got[b], ref)


def test_workspace_query(lib):
    assert lib.gdm_targets_workspace_bytes(4, 2048, 4096) > 4 * 3 * 4096 * 4 + 4 * 2048 * 4
    assert lib.gdm_targets_workspace_bytes(4, 2048, 3) == 0
    assert lib.gdm_targets_workspace_bytes(0, 2048, 4096) == 0
    assert lib.gdm_targets_workspace_bytes(4, 0, 4096) == 0


def _buf():
    b = (ctypes.c_char * (1 << 20))()
    return b, (ctypes.addressof(b) + 255) & ~255


def test_hpr_argument_refusals(lib):
    keep, p = _buf()
    ws = 1 << 19
    assert lib.gdm_hpr_visible_hip(p, 0, p, None, 1, 3, p, ws, p, p, None) == -1
    assert b"M=3" in lib.gdm_last_error()
    assert lib.gdm_hpr_visible_hip(p, 0, p, None, 0, 64, p, ws, p, p, None) == -1
    assert b"B=0" in lib.gdm_last_error()
    assert lib.gdm_hpr_visible_hip(None, 0, p, None, 1, 64, p, ws, p, p, None) == -1
    assert b"NULL" in lib.gdm_last_error()
    assert lib.gdm_hpr_visible_hip(p, 0, p, None, 1, 64, p, 16, p, p, None) == -1
    assert b"workspace" in lib.gdm_last_error()
    assert lib.gdm_hpr_visible_hip(p, 5, p, None, 2, 64, p, ws, p, p, None) == -1
    assert b"model_bstride" in lib.gdm_last_error()


def test_pose_targets_argument_refusals(lib):
    keep, p = _buf()
    ws = 1 << 19

    def call(B=1, N=16, M=64, thresh=0.01, labels=p):
        return lib.gdm_pose_targets_hip(p, 48, 3, 1, labels, p, p, 0, p, B, N, M, thresh, p, ws, p, p, p, p, None)

    assert call(thresh=0.0) == -1 and b"dist_thresh" in lib.gdm_last_error()
    assert call(thresh=-0.01) == -1 and b"dist_thresh" in lib.gdm_last_error()
    assert call(M=3) == -1 and b"M=3" in lib.gdm_last_error()
    assert call(B=0) == -1 and b"B=0" in lib.gdm_last_error()
    assert call(B=-1) == -1 and b"B=-1" in lib.gdm_last_error()
    assert call(N=0) == -1 and b"N=0" in lib.gdm_last_error()
    assert call(labels=None) == -1 and b"NULL" in lib.gdm_last_error()


def test_python_api_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        targets.visible_vertices(torch.zeros(8, 3), torch.zeros(1, 3, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        targets.pose_gt_info(torch.zeros(1, 16, 3), torch.zeros(1, 16), torch.zeros(1, 3, 4), torch.zeros(8, 3))


def test_gt_targets_option_default_and_choices():
    from geometric_aware_dense_matching_amd import train_lm
    assert train_lm.build_parser().parse_args([]).gt_targets == "loader"
    assert train_lm.build_parser().parse_args(["--gt-targets", "device"]).gt_targets == "device"
    with pytest.raises(SystemExit):
        train_lm.build_parser().parse_args(["--gt-targets", "cpu"])


def test_synthetic_items_for_device_targets():
    """Default items are unchanged; device-mode items carry RT and origin_labels, no match_idx / visible_flag, and their labelled
    points lie on (or, for about 10 %, over a centimetre off) the posed model."""
    from geometric_aware_dense_matching_amd import synthetic, train_lm
    plain = train_lm.SyntheticCrops(2, 1024, 64)[1]
    assert set(plain) == {"rgb", "cld_rgb_nrm", "choose", "dpt_xyz", "labels", "origin_labels", "match_idx", "visible_flag", "RT",
                          "scene_id", "im_id"}
    xyz = (synthetic.make_model_points(1, 256)[:, :3] / 1000.0).astype(np.float32)
    it = train_lm.SyntheticCrops(2, 1024, 256, model_xyz=xyz)[1]
    assert "match_idx" not in it and "visible_flag" not in it and "labels" not in it
    assert it["RT"].shape == (3, 4) and it["origin_labels"].dtype == np.int32 and it["origin_labels"].sum() > 0
    posed = xyz @ it["RT"][:, :3].T + it["RT"][:, 3]
    pts = it["cld_rgb_nrm"][:3, it["origin_labels"] > 0].T
    d = np.sqrt(((pts[:, None] - posed[None]) ** 2).sum(-1)).min(1)
    assert 0.8 < (d < 0.0025).mean() < 0.97 and (d > 0.01).any()
