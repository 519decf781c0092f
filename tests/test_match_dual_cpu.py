"""CPU: the numpy restatement of include/gdm.h's THE DUAL RULE (matching.match_dual_numpy) on hand-written cases, the option checks of
the Python layers, the train_lm flags, the C entry's refusals before any HIP call, and the LDS / packed-fp32 hazard scan of the new
kernels."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from geometric_aware_dense_matching_amd import infer, matching, pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# gamma = 1 and sim = log of small integers: every weight exp(gamma sim) is that integer, so the sums are read off the matrix.
# Row 2 ties columns 2 and 3 (the first wins); column 1 ties rows 1 and 2, column 3 ties rows 1 and 2 (the lowest row wins).
W = np.array([[4.0, 1.0, 1.0, 2.0],
              [1.0, 2.0, 1.0, 4.0],
              [2.0, 2.0, 4.0, 4.0]])
XYZ = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [1.0, 1.0, 1.0]])


def _dual(mask):
    return matching.match_dual_numpy(np.log(W), None, XYZ, mask, 1.0)


def test_dual_numpy_full_mask_with_exact_ties():
    r = _dual([1, 1, 1])
    assert r["best_idx"].tolist() == [0, 3, 2] and r["col_idx"].tolist() == [0, 1, 2, 1]
    np.testing.assert_allclose(r["conf"], [4 / 8, 4 / 8, 4 / 12], rtol=1e-14)
    np.testing.assert_allclose(r["lse"], np.log([8, 8, 12]), rtol=1e-14)
    np.testing.assert_allclose(r["col_lse"], np.log([7, 5, 6, 10]), rtol=1e-14)
    np.testing.assert_allclose(r["col_sim"], np.log([4, 2, 4, 4]), rtol=1e-14)
    np.testing.assert_allclose(r["col_conf"], [4 / 7, 2 / 5, 4 / 6, 4 / 10], rtol=1e-14)
    np.testing.assert_allclose(r["dual"], [0.5 * 4 / 7, 0.5 * 4 / 10, (1 / 3) * 4 / 6], rtol=1e-14)
    np.testing.assert_allclose(r["soft_xyz"][0], (W[0] @ XYZ) / 8, rtol=1e-14)
    assert (r["dual"] <= r["conf"]).all() and (r["col_conf"] <= 1).all()


def test_dual_numpy_partial_mask_moves_the_columns_only():
    full, r = _dual([1, 1, 1]), _dual([1, 0, 1])
    for k in ("best_idx", "best_sim", "lse", "conf", "soft_xyz"):          # the rows do not know the mask
        assert np.array_equal(r[k], full[k]), k
    assert r["col_idx"].tolist() == [0, 2, 2, 2]
    np.testing.assert_allclose(r["col_lse"], np.log([6, 3, 5, 6]), rtol=1e-14)
    np.testing.assert_allclose(r["col_conf"], [4 / 6, 2 / 3, 4 / 5, 4 / 6], rtol=1e-14)
    np.testing.assert_allclose(r["dual"], [0.5 * 4 / 6, 0.0, (1 / 3) * 4 / 5], rtol=1e-14)
    assert r["dual"][1] == 0.0                                             # an unmasked point


def test_dual_numpy_single_masked_point():
    r = _dual([0, 1, 0])
    assert r["col_idx"].tolist() == [1, 1, 1, 1]
    assert (r["col_conf"] == 1.0).all()                                    # the only term of its column
    np.testing.assert_allclose(r["col_lse"], np.log(W[1]), rtol=1e-14, atol=1e-15)
    assert r["dual"].tolist() == [0.0, r["conf"][1], 0.0]                  # dual == conf exactly


def test_dual_numpy_crop_with_no_masked_point():
    r = _dual([0, 0, 0])
    assert r["col_idx"].tolist() == [-1] * 4 and np.isneginf(r["col_sim"]).all() and np.isneginf(r["col_lse"]).all()
    assert (r["col_conf"] == 0).all() and (r["dual"] == 0).all()
    assert r["best_idx"].tolist() == [0, 3, 2] and (r["conf"] > 0).all()   # the rows are as ever


def test_dual_numpy_from_descriptors_matches_its_parts():
    rs = np.random.RandomState(5)
    scene, model = rs.randn(6, 128).astype(np.float32) * 3, rs.randn(128, 9).astype(np.float32)
    xyz, mask = rs.rand(9, 3), np.array([1, 0, 1, 1, 0, 1])
    r = matching.match_dual_numpy(scene, model, xyz, mask, 16.0)
    soft, two = matching.match_soft_numpy(scene, model, xyz, 16.0), matching.match_twoway_numpy(scene, model, mask)
    for k in ("best_idx", "best_sim", "lse", "conf", "soft_xyz"):
        assert np.array_equal(r[k], soft[k]), k
    assert np.array_equal(r["col_idx"], two["col_idx"]) and np.array_equal(r["col_sim"], two["col_sim"])
    a = scene.astype(np.float64) / np.linalg.norm(scene.astype(np.float64), axis=1, keepdims=True)
    b = model.astype(np.float64) / np.linalg.norm(model.astype(np.float64), axis=0, keepdims=True)
    w = np.exp(16.0 * (a @ b))
    zc = w[mask != 0].sum(0)
    np.testing.assert_allclose(r["col_lse"], np.log(zc), rtol=1e-13)
    i = np.flatnonzero(mask)
    np.testing.assert_allclose(r["dual"][i], r["conf"][i] * w[i, r["best_idx"][i]] / zc[r["best_idx"][i]], rtol=1e-12)
    assert (r["dual"][mask == 0] == 0).all() and (r["dual"] <= r["conf"]).all()


# ---- option checks ------------------------------------------------------------------------------------------------------------------------
def _ep():
    return dict(seg=torch.zeros(1, 2, 4), rgbd=torch.zeros(1, 128, 4), mesh=torch.zeros(1, 128, 3))


def test_dual_needs_soft_and_excludes_twoway():
    soft = dict(gamma=16.0, model_xyz=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="dual=True needs soft"):
        matching.match_frames(_ep(), dual=True)
    with pytest.raises(ValueError, match="dual=True needs soft"):
        matching.match_tail(_ep(), 1, 4, 3, dual=True)
    with pytest.raises(ValueError, match="do not pass twoway=True"):
        matching.match_frames(_ep(), soft=soft, twoway=True, dual=True)
    with pytest.raises(ValueError, match="do not pass twoway=True"):
        matching.match_tail(_ep(), 1, 4, 3, soft=soft, twoway=True, dual=True)
    with pytest.raises(ValueError, match="twoway and soft exclude each other"):          # today's refusal stands
        matching.match_frames(_ep(), soft=soft, twoway=True)


def test_pipeline_options_refuse_before_anything_runs():
    with pytest.raises(ValueError, match="match_dual needs match_gamma"):
        infer.pipeline_step(None, {}, match_dual=True)
    with pytest.raises(ValueError, match="do not pass match_twoway"):
        infer.pipeline_step(None, {}, match_gamma=16.0, match_dual=True, match_twoway=True)
    with pytest.raises(ValueError, match="twoway and soft exclude each other"):          # without match_dual, as ever
        infer.pipeline_step(None, {}, match_gamma=16.0, pose_opts=dict(pair_filter="cycle"))
    with pytest.raises(ValueError, match="match_dual needs match_gamma"):
        infer.run_multi_object({}, {}, [1], match_dual=True)
    assert infer._twoway(False, dict(pair_filter="cycle"), 16.0, True) is False         # the dual kernel's col_idx serves the filter


def test_solve_poses_dual_weights_need_dual_in_res():
    with pytest.raises(ValueError, match=r"need the soft matching outputs \['dual'\]"):
        pose.solve_poses(dict(mask=None, best_idx=None, conf=None), None, None, weights="dual")
    with pytest.raises(ValueError, match="weights must be"):
        pose.solve_poses(dict(mask=None, best_idx=None), None, None, weights="sim")
    with pytest.raises(ValueError, match="RANSAC keeps the hard pairs"):
        pose.solve_poses(dict(mask=None, best_idx=None, dual=None), None, None, method="ransac", weights="dual")


def test_train_lm_flags_parse_and_check_one_another():
    from geometric_aware_dense_matching_amd import train_lm
    parse = train_lm.build_parser().parse_args
    a = parse(["-state", "test"])
    assert a.match_dual is False and a.match_score == "conf" and train_lm.check_dual_flags(a) is False
    a = parse("-state test --match-gamma 16 --match-dual --pose-weights dual --match-score dual --pair-filter cycle".split())
    assert a.match_dual and a.pose_weights == "dual" and a.match_score == "dual" and train_lm.check_dual_flags(a) is True
    for argv, msg in (("--match-dual", "--match-dual needs --match-gamma"),
                      ("--match-gamma 16 --pose-weights dual", "--pose-weights dual needs --match-dual"),
                      ("--match-gamma 16 --match-score dual", "--match-score dual needs --match-dual")):
        with pytest.raises(SystemExit, match=msg):
            train_lm.check_dual_flags(parse(["-state", "test"] + argv.split()))


# ---- the C entry ----------------------------------------------------------------------------------------------------------------------------
def test_dual_entry_refuses_before_any_hip_call():
    """Host pointers, no GPU: NULL, non-positive sizes, gamma outside (0, 40] and NaN, M beyond the 64 panels, a bad precision, B*N
    beyond the two-way entry's limit, rows or workspace off a 16-byte boundary, a short workspace -- each names itself."""
    from geometric_aware_dense_matching_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_char * 65536)()
    p = ctypes.addressof(buf)
    p += (-p) % 16

    def call(gamma=16.0, B=1, N=64, M=200, prec=0, nbytes=1 << 30, ptr=None):
        a = dict(scene_rows=p, model_rows=p, model_xyz=p, mask=p, partial=p)
        a.update(ptr or {})
        return lib.gdm_match_dual_packed_hip(a["scene_rows"], a["model_rows"], a["model_xyz"], a["mask"], B, N, M, prec, gamma,
                                             p, p, p, p, p, p, p, p, p, a.get("dual", p), a["partial"], nbytes, None)

    def err():
        return lib.gdm_last_error()

    for gamma in (0.0, -1.0, 40.5, float("nan"), float("inf")):
        assert call(gamma) == -1 and b"gdm_match_dual_packed_hip" in err() and b"gamma" in err(), gamma
    for name in ("scene_rows", "model_rows", "model_xyz", "mask", "partial", "dual"):
        assert call(ptr={name: None}) == -1 and b"gdm_match_dual_packed_hip: NULL" in err(), name
    for kw in (dict(B=0), dict(N=0), dict(M=0), dict(B=-1), dict(N=-5)):
        assert call(**kw) == -1 and b"bad shape" in err(), kw
    assert call(M=16385) == -1 and b"M=16385" in err()
    assert call(B=4096, N=1024) == -1 and b"B*N too large" in err()
    assert call(prec=2) == -1 and b"precision=2" in err()
    for name in ("scene_rows", "model_rows", "partial"):
        assert call(ptr={name: p + 4}) == -1 and b"16-byte aligned" in err(), name
    assert call(nbytes=1024) != 0 and b"gdm_match_dual_packed_hip: partial workspace" in err()
    B, N, M = 16, 2048, 8192
    assert lib.gdm_match_dual_partial_bytes(B, N, M) >= lib.gdm_match_soft_partial_bytes(B, N) + 8 * B * M + 4 * B * 8 * M + 4 * B * M
    assert lib.gdm_match_dual_partial_bytes(0, 5, 5) == 0 and lib.gdm_match_dual_partial_bytes(5, 5, 0) == 0
    assert _lib.PARAMS["gdm_match_dual_packed_hip"][-1] == "stream"


# ---- hazard scan ----------------------------------------------------------------------------------------------------------------------------
def test_dual_kernels_have_no_exposed_packed_fp32_consumer(tmp_path):
    """As tests/test_match_soft_cpu.py scans the soft kernels: hipcc -S of gdm_match.hip with the Makefile's flags, then
    tools/scan_lds_pk_hazard.py over the two dual panel instances, the column kernel and the row kernel."""
    csrc = os.path.join(ROOT, "geometric_aware_dense_matching_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", mk, flags=re.M))
    flags = var["CXXFLAGS"].replace("$(ARCH)", var["ARCH"]).split()
    hipcc = os.environ.get("HIPCC", var["HIPCC"])
    asm = str(tmp_path / "gdm_match.s")
    subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(csrc, "gdm_match.hip"), "-o", asm], check=True,
                   capture_output=True, timeout=900)
    spec = importlib.util.spec_from_file_location("scan_lds_pk_hazard", os.path.join(ROOT, "tools", "scan_lds_pk_hazard.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    text = open(asm).read()
    kernels = sorted(set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)))
    new = [k for k in kernels if "dual" in k]
    assert len(new) == 4, kernels
    assert not [k for k in tool.scan(asm) if "dual" in k]
    # the issue's register rule: no scratch in either instance of the panel kernel
    for k in new:
        body = text[text.index(".amdhsa_kernel " + k):]
        body = body[:body.index(".end_amdhsa_kernel")]
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", body), k
