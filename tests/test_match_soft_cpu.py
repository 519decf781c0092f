"""CPU: soft-assignment matching and the weighted pose fit without a device -- the fp64 restatements (matching.match_soft_numpy,
pose.kabsch_weighted_numpy) against direct evaluations and on the synthetic probe that motivated the feature, the shared fit fragment
with n = sum w, the host-side argument checks of the new entry points, and the LDS / packed-fp32 hazard scan of the new kernels."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from geometric_aware_dense_matching_amd import matching, pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatements ----------------------------------------------------------------------------------------------------------------
def test_match_soft_numpy_vs_scipy():
    """(1, 33, 50): lse / conf / soft_xyz against scipy's logsumexp and softmax on the fp64 cosines; ties take the first maximum."""
    from scipy.special import logsumexp, softmax
    rs = np.random.RandomState(50)
    scene = (rs.randn(33, 128) * rs.rand(33, 1) * 3).astype(np.float32)
    model = rs.randn(128, 50).astype(np.float32)
    model[:, 40] = model[:, 7]                                          # an exact duplicate: the first one must win
    scene[5] = model[:, 7]
    xyz = 0.05 * rs.uniform(-1, 1, (50, 3))
    for gamma in (16.0, 40.0):
        got = matching.match_soft_numpy(scene, model, xyz, gamma)
        a = scene.astype(np.float64) / np.linalg.norm(scene.astype(np.float64), axis=1, keepdims=True)
        b = model.astype(np.float64) / np.linalg.norm(model.astype(np.float64), axis=0, keepdims=True)
        sim = a @ b
        p = softmax(gamma * sim, axis=1)
        assert np.array_equal(got["best_idx"], sim.argmax(1)) and got["best_idx"][5] == 7
        assert np.abs(got["lse"] - logsumexp(gamma * sim, axis=1)).max() <= 1e-12
        assert np.abs(got["conf"] - p.max(1)).max() <= 1e-13
        assert np.abs(got["soft_xyz"] - p @ xyz).max() <= 1e-15
        assert got["conf"][5] <= 0.5
        again = matching.match_soft_numpy(sim, None, xyz, gamma)        # a similarity matrix in place of the descriptors
        for k in got:
            assert np.array_equal(got[k], again[k]), k


def _rotation(rs):
    q, r = np.linalg.qr(rs.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _ellipsoid(rs, n):
    v = rs.randn(n, 3)
    return v / np.linalg.norm(v, axis=1, keepdims=True) * np.array([0.05, 0.035, 0.025])   # 100 x 70 x 50 mm


def test_confidence_weighted_fit_on_the_synthetic_probe():
    """M = 4096 model vertices on a 100 x 70 x 50 mm ellipsoid, N = 1024 posed scene points on it with 0.5 mm noise, 128-d random
    Fourier features of position (length scale 6 mm) plus descriptor noise, 30 % of the scene points replaced by random descriptors
    at random positions near the object; gamma = 16.  Synthetic descriptors: no claim about a trained network.  The conf-weighted
    fit must reach a fifth of the unweighted fit's ADD (it reaches about a fifteenth) and the planted outliers' median confidence
    must stay under a tenth of the inliers' (0.007 against 0.22)."""
    rs = np.random.RandomState(1)
    M, N, gamma = 4096, 1024, 16.0
    mx, sx = _ellipsoid(rs, M), _ellipsoid(rs, N)
    W = rs.randn(3, 64) / 0.006

    def feat(x):
        return np.concatenate([np.cos(x @ W), np.sin(x @ W)], axis=1)

    R, t = _rotation(rs), np.array([0.01, -0.02, 0.6])
    scene = sx @ R.T + t + rs.randn(N, 3) * 0.0005
    fs = feat(sx) + rs.randn(N, 128) * 0.3
    out = rs.choice(N, int(0.3 * N), replace=False)
    fs[out] = rs.randn(len(out), 128)
    scene[out] = rs.uniform(-0.06, 0.06, (len(out), 3)) @ R.T + t
    r = matching.match_soft_numpy(fs.astype(np.float32), feat(mx).T.astype(np.float32), mx, gamma)
    A = mx[r["best_idx"]]

    def add(RT):
        return np.linalg.norm((mx @ RT[:, :3].T + RT[:, 3]) - (mx @ R.T + t), axis=1).mean()

    plain = add(pose.kabsch_weighted_numpy(A, scene, np.ones(N)))
    weighted = add(pose.kabsch_weighted_numpy(A, scene, r["conf"]))
    inl = np.ones(N, bool)
    inl[out] = False
    print("ADD plain %.3f mm, conf-weighted %.3f mm; median conf inliers %.3f, outliers %.4f"
          % (plain * 1e3, weighted * 1e3, np.median(r["conf"][inl]), np.median(r["conf"][out])))
    assert weighted <= plain / 5
    assert np.median(r["conf"][out]) < np.median(r["conf"][inl]) / 10


def test_kabsch_weighted_numpy_properties():
    """Exact data is recovered whatever the weights; scaling the weights changes nothing; a zero weight removes the pair."""
    rs = np.random.RandomState(3)
    A = rs.randn(40, 3)
    R, t = _rotation(rs), rs.randn(3)
    B = A @ R.T + t
    w = rs.rand(40) + 0.1
    RT = pose.kabsch_weighted_numpy(A, B, w)
    assert np.abs(RT[:, :3] - R).max() <= 1e-12 and np.abs(RT[:, 3] - t).max() <= 1e-12
    B2 = B + rs.randn(40, 3) * 0.05
    a, b = pose.kabsch_weighted_numpy(A, B2, w), pose.kabsch_weighted_numpy(A, B2, 1000 * w)
    assert np.abs(a - b).max() <= 1e-12
    w0 = w.copy()
    w0[::3] = 0
    assert np.abs(pose.kabsch_weighted_numpy(A, B2, w0) - pose.kabsch_weighted_numpy(A[w0 > 0], B2[w0 > 0], w0[w0 > 0])).max() <= 1e-12


# ---- the fit fragment with weights ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [1e-3, 1.0, 1e3])
def test_fit_fragment_with_weighted_statistics(total):
    """csrc/gdm_kabsch_fit.inc compiled for the host (oracle/kabsch_fit.py) on the 16 weighted statistics with n = sum w = total:
    the bounds of tests/test_pose_fit_cpu.py against kabsch_weighted_numpy (R to 1e-7, t to one fp32 ulp of max(1, |t|)) -- the
    fragment divides by n only, so the scale of the weights must not matter."""
    from oracle import kabsch_fit
    rs = np.random.RandomState(int(round(np.log10(total))) + 10)
    K, n = 200, 64
    stats, want = np.zeros((K, 16)), np.zeros((K, 3, 4))
    for k in range(K):
        A = (rs.rand(n, 3) - 0.5) * 0.2
        R, t = _rotation(rs), rs.randn(3) * 0.3 + np.array([0, 0, 0.8])
        B = (A @ R.T + t + rs.randn(n, 3) * 0.002).astype(np.float32).astype(np.float64)
        A = A.astype(np.float32).astype(np.float64)
        w = rs.rand(n).astype(np.float32).astype(np.float64)
        w *= total / w.sum()
        wA = w[:, None] * A
        stats[k] = np.concatenate([[w.sum()], wA.sum(0), (w[:, None] * B).sum(0), (wA.T @ B).reshape(9)])
        want[k] = pose.kabsch_weighted_numpy(A, B, w)
    got = kabsch_fit.fit(stats).astype(np.float64)
    assert np.isfinite(got).all()
    Rg = got[:, :, :3]
    assert np.abs(Rg @ Rg.transpose(0, 2, 1) - np.eye(3)).max() <= 2e-7
    assert np.abs(Rg - want[:, :, :3]).max() <= 1e-7, float(np.abs(Rg - want[:, :, :3]).max())
    tol = 2.0 ** -23 * np.maximum(1.0, np.abs(want[:, :, 3]).max(1))
    assert (np.abs(got[:, :, 3] - want[:, :, 3]).max(1) <= tol).all()


# ---- argument checks -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from geometric_aware_dense_matching_amd import _lib
    return _lib.lib()


def test_soft_entry_refuses_bad_gamma_and_uncovered_m_without_a_device(lib):
    """gamma in {0, -1, 40.5, NaN} and M = 16385 (beyond the 64 panels the kernel covers) come back as GDM_EINVAL with a message,
    before any HIP call: host pointers, no GPU."""
    buf = (ctypes.c_char * 65536)()
    p = ctypes.addressof(buf)

    def call(gamma, M=200, prec=0, nbytes=1 << 30):
        return lib.gdm_match_soft_packed_hip(p, p, p, 64, M, prec, gamma, p, p, p, p, p, p, nbytes, None)

    for gamma in (0.0, -1.0, 40.5, float("nan"), float("inf")):
        assert call(gamma) == -1, gamma
        assert b"gamma" in lib.gdm_last_error()
    assert call(16.0, M=16385) == -1 and b"M=16385" in lib.gdm_last_error()
    assert call(16.0, M=0) == -1
    assert call(16.0, prec=2) == -1 and b"precision" in lib.gdm_last_error()
    assert call(16.0, nbytes=1024) != 0 and b"partial workspace" in lib.gdm_last_error()
    assert lib.gdm_match_soft_partial_bytes(16, 2048) >= lib.gdm_match_partial_bytes(16, 2048) + 64 * 16 * 2048 * 16
    assert lib.gdm_match_soft_partial_bytes(0, 5) == 0
    assert lib.gdm_kabsch_stats_w_hip(p, 0, 1, 1, None, None, None, p, p, 1, 8, 8, p, p, None) == -1      # neither target nor vertices
    assert lib.gdm_kabsch_solve_w_hip(p, None, 1, 5, p, p, None) == -1


def test_python_layer_refuses_what_it_cannot_run():
    import torch
    from geometric_aware_dense_matching_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.match_soft(torch.zeros(1, 128, 32), torch.zeros(128, 64), torch.zeros(64, 3))
    with pytest.raises(ValueError, match="soft must be"):
        matching.match_frames(dict(seg=None, rgbd=None, mesh=None), soft=dict(gamma=16))
    with pytest.raises(ValueError, match="need the soft matching outputs"):
        pose.solve_poses(dict(mask=None, best_idx=None), None, None, weights="conf")
    with pytest.raises(ValueError, match="RANSAC keeps the hard pairs"):
        pose.solve_poses(dict(mask=None, best_idx=None), None, None, method="ransac", targets="soft")
    with pytest.raises(ValueError, match="weights must be"):
        pose.solve_poses(dict(mask=None, best_idx=None), None, None, method="ransac", weights="sim")
    with pytest.raises(ValueError, match=r"\['soft_xyz'\]"):
        pose.solve_poses(dict(mask=None, best_idx=None, conf=None), None, None, weights="conf", targets="soft")
    with pytest.raises(ValueError, match="unknown pose_opts"):
        pose.estimate_poses({}, None, None, pose_opts=dict(weight="conf"))


def test_bop_csv_writes_the_given_scores():
    from geometric_aware_dense_matching_amd import evaluation
    RT = np.tile(np.concatenate([np.eye(3), [[0.0], [0.0], [0.5]]], axis=1), (2, 1, 1))
    csv = evaluation.BopCsv()
    csv.add_batch(["000001/000007", "000001/000008"], 5, RT)
    csv.add_batch(["000002/000001", "000002/000002"], 5, RT, scores=np.array([0.25, 0.5]))
    assert [ln.split(",")[3] for ln in csv.lines[1:]] == ["-1", "-1", "0.25", "0.5"]
    with pytest.raises(ValueError):
        csv.add_batch(["000002/000001"], 5, RT, scores=np.array([0.25]))


# ---- hazard scan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit, marks, n_new", [("gdm_match.hip", ("soft",), 3), ("gdm_pose.hip", ("kabsch_stats_w", "kabsch_solve_w"), 2),
                                                ("gdm_match.hip", ("match_kernel", "match_panel_kernel"), 8),
                                                ("gdm_circle.hip", ("circle_mm",), 6)])
def test_new_kernels_have_no_exposed_packed_fp32_consumer(tmp_path, unit, marks, n_new):
    """hipcc -S of the translation units that hold the new kernels, with the Makefile's flags, then tools/scan_lds_pk_hazard.py: in
    no soft instance, in neither weighted pose kernel and in none of the kernels that share the tile helpers (match_kernel,
    match_panel_kernel, circle_mm_kernel: sharing re-orders their instructions) does a packed-fp32 instruction read a register fewer
    than two wait states after the wait that retires its LDS read."""
    csrc = os.path.join(ROOT, "geometric_aware_dense_matching_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", mk, flags=re.M))
    flags = var["CXXFLAGS"].replace("$(ARCH)", var["ARCH"]).split()
    hipcc = os.environ.get("HIPCC", var["HIPCC"])
    asm = str(tmp_path / (unit + ".s"))
    subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(csrc, unit), "-o", asm], check=True,
                   capture_output=True, timeout=900)
    spec = importlib.util.spec_from_file_location("scan_lds_pk_hazard", os.path.join(ROOT, "tools", "scan_lds_pk_hazard.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    text = open(asm).read()
    kernels = sorted(set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)))
    new = [k for k in kernels if any(m in k for m in marks)]
    assert len(new) == n_new, kernels
    assert "ds_read" in text or "ds_bpermute" in text                   # the scan had LDS reads to look at
    found = tool.scan(asm)
    assert not [k for k in found if any(m in k for m in marks)], found
