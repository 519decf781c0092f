"""CPU: the robust pose fits' host side -- the sample hash restated in Python against the golden's recorded draws, argument checking
of the new C entry points (no GPU needed: every check comes before any HIP call), the command-line defaults, and the numpy
restatements of the reference's RANSAC and ICP (oracle/pose_ref.py) against the golden the real reference made."""
import ctypes
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def lib():
    from geometric_aware_dense_matching_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_ransac_sample_indices_match_golden():
    from geometric_aware_dense_matching_amd import pose
    g = np.load(os.path.join(G, "pose_robust.npz"))
    n = g["r_mask"].sum(1)
    got = pose.ransac_sample_indices(n, int(g["H"]), int(g["seed"]))
    assert np.array_equal(got, g["r_samples"])
    assert (got[:, 0] == -1).all()
    live = got[:, 1:]
    assert (live >= 0).all() and (live < np.maximum(n, 1)[:, None, None]).all()


def test_ransac_sample_indices_known_values():
    """lowbias32 chain of include/gdm.h, by hand for crop 1, hypothesis 1, draw 0 (seed 7, n = 100)."""
    from geometric_aware_dense_matching_amd import pose

    def mix(x):
        x &= 0xffffffff
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xffffffff
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xffffffff
        return x ^ (x >> 16)

    r = mix(mix(mix(7 ^ 0x9e3779b9) ^ 1) ^ 4)
    assert pose.ransac_sample_indices([10, 100], 2, 7)[1, 1, 0] == (r * 100) >> 32


def _ransac(lib, p, **over):
    a = dict(scene=p, bstride=27, pts=1, chs=9, model=p, idx=p, mask=p, stats=p, B=1, N=3, M=4, H=20, err=0.015, fix=0.7, seed=0,
             minp=5, ws=p, wsb=1 << 16, RT=p, valid=p, counts=p, winner=p, stream=None)
    a.update(over)
    return lib.gdm_ransac_pose_hip(*a.values())


@pytest.mark.parametrize("over, msg", [
    (dict(H=0), b"H=0"), (dict(H=5000), b"H=5000"), (dict(err=0.0), b"match_err"), (dict(err=-0.01), b"match_err"),
    (dict(fix=0.0), b"fix_percent"), (dict(fix=1.5), b"fix_percent"), (dict(B=0), b"bad shape"), (dict(N=-1), b"bad shape"),
    (dict(scene=None), b"NULL"), (dict(counts=None), b"NULL"), (dict(wsb=16), b"workspace"), (dict(minp=0), b"min_points"),
])
def test_ransac_entry_rejects_bad_arguments(lib, over, msg):
    buf = (ctypes.c_char * 65536)()
    p = ctypes.addressof(buf)
    assert _ransac(lib, p, **over) == -1
    assert msg in lib.gdm_last_error()


def test_ransac_workspace_bytes(lib):
    assert lib.gdm_ransac_workspace_bytes(16, 2048, 1024) >= 16 * 2048 * 24 + 16 * 1024 * 48
    assert lib.gdm_ransac_workspace_bytes(16, 2048, 5000) == 0


def test_icp_entries_reject_bad_arguments(lib):
    buf = (ctypes.c_char * 65536)()
    p = ctypes.addressof(buf)
    assert lib.gdm_icp_update_hip(p, 27, 1, 9, p, p, p, p, 1, 3, 4, -1.0, -0.5, 5, p, p, p, p, None) == -1
    assert b"tolerance" in lib.gdm_last_error()
    assert lib.gdm_icp_update_hip(p, 27, 1, 9, p, p, p, p, 1, 3, 4, -1.0, 0.001, 0, p, p, p, p, None) == -1
    assert b"min_points" in lib.gdm_last_error()
    assert lib.gdm_icp_update_hip(p, 27, 1, 9, p, None, p, p, 1, 3, 4, -1.0, 0.001, 5, p, p, p, p, None) == -1
    assert b"NULL" in lib.gdm_last_error()
    assert lib.gdm_icp_transform_hip(p, 27, 0, 9, p, 1, 3, p, None) == -1
    assert b"strides" in lib.gdm_last_error()
    assert lib.gdm_icp_transform_hip(p, 27, 1, 9, p, 1, 0, p, None) == -1
    assert b"bad shape" in lib.gdm_last_error()


def test_shared_support_batch_stride_is_accepted_by_validation(lib):
    """The ICP searches one model cloud for every crop (support batch stride 0); a stride that is neither 0 nor >= S*3 stays an error."""
    from geometric_aware_dense_matching_amd import _lib
    buf = (ctypes.c_char * 65536)()
    p = ctypes.addressof(buf)
    job = (_lib.KnnJob * 1)()
    job[0].support, job[0].query, job[0].idx, job[0].d2 = p, p, p, p
    job[0].support_bstride, job[0].query_bstride, job[0].S, job[0].Q, job[0].K = 3, 12, 4, 4, 1
    assert lib.gdm_knn_jobs_ws_hip(job, 1, 2, None, 0, None) == -1
    assert b"support_bstride" in lib.gdm_last_error()


def test_parser_defaults_unchanged():
    from geometric_aware_dense_matching_amd import train_lm, train_ycb
    for mod in (train_lm, train_ycb):
        a = mod.build_parser().parse_args(["-state=test"])
        assert a.pose_fit == "kabsch" and a.icp_iters == 0
        assert a.ransac_iters == 20 and a.ransac_inlier_dist == 0.015 and a.icp_tolerance == 0.001
    a = train_lm.build_parser().parse_args("-state=test --pose-fit ransac --ransac-iters 64 --icp-iters 3".split())
    assert a.pose_fit == "ransac" and a.ransac_iters == 64 and a.icp_iters == 3
    with pytest.raises(SystemExit):
        train_lm.build_parser().parse_args("--pose-fit svd".split())


def test_pose_options_are_checked_on_the_host():
    from geometric_aware_dense_matching_amd import pose
    with pytest.raises(ValueError, match="method"):
        pose.solve_poses({"mask": None, "best_idx": None}, None, None, method="lmeds")
    with pytest.raises(ValueError, match="pose_opts"):
        pose.estimate_poses({}, None, None, pose_opts={"ransac_iter": 3})


def test_oracle_ransac_restatement_matches_reference_golden():
    """oracle/pose_ref.ransac (what the GPU tests at product shapes compare with) against the real reference's recorded run."""
    from oracle import pose_ref
    g = np.load(os.path.join(G, "pose_robust.npz"))
    H = int(g["H"])
    for b in range(g["r_mask"].shape[0]):
        sel = g["r_mask"][b] != 0
        if sel.sum() < 5:                                              # the evaluator's sentinel, before any fit
            assert g["r_winner"][b] == -1 and g["r_valid"][b] == 0
            continue
        A = g["r_model"][g["r_idx"][b][sel]].astype(np.float64)
        Bp = g["r_cld"][b, :3][:, sel].T.astype(np.float64)
        r = pose_ref.ransac(A, Bp, g["r_samples"][b], float(g["match_err"]), float(g["fix_percent"]))
        assert np.array_equal(r["counts"], g["r_counts"][b]) and np.array_equal(r["near"], g["r_near"][b])
        assert r["winner"] == g["r_winner"][b] and (r["winner"] >= 0) == bool(g["r_valid"][b])
        assert not r["degenerate"][1:].any()                           # the golden script rejected such data
        assert len(r["poses"]) == H
        if r["winner"] >= 0:
            assert np.abs(r["RT"] - g["r_RT"][b]).max() <= 1e-9
        else:
            assert r["RT"] is None


def test_oracle_icp_restatement_matches_reference_golden():
    from oracle import pose_ref
    g = np.load(os.path.join(G, "pose_robust.npz"))
    for b in range(g["i_RT0"].shape[0]):
        r = pose_ref.icp(g["i_cld"][b, :3].T, g["i_model"], g["i_RT0"][b], None, int(g["i_max_iters"]), float(g["i_tol"]))
        assert r["iters"] == g["i_iters"][b]
        assert np.abs(r["RT"] - g["i_RT"][b]).max() <= 1e-9
        assert abs(r["resid"][-1] - g["i_resid"][b]) <= 1e-9
        assert not r["starved"] and all(len(t) == 0 for t in r["ties"])


def test_oracle_ransac_rule_and_pinning():
    """The decision rule and the 'pinned' predicate the GPU test leans on, on hand-made count tables."""
    from oracle import pose_cases, pose_ref
    z = np.zeros(4, bool)
    assert pose_ref.ransac_decide([3, 8, 8, 2], 10, 0.7) == (1, True)
    assert pose_ref.ransac_decide([3, 7, 7, 2], 10, 0.7) == (1, False)          # 7 > 7.0 is false: best count, earliest on ties
    assert pose_ref.ransac_decide([0, 0, 0, 0], 10, 0.7) == (-1, False)
    assert pose_cases.decision_pinned([3, 8, 8, 2], [0, 0, 5, 5], z, 10, 0.7)
    assert not pose_cases.decision_pinned([3, 8, 8, 2], [0, 1, 0, 0], z, 10, 0.7)     # the winner could drop to 7
    assert not pose_cases.decision_pinned([6, 8, 8, 2], [2, 0, 0, 0], z, 10, 0.7)     # an earlier one could rise to 8
    assert pose_cases.decision_pinned([6, 8, 8, 2], [2, 0, 0, 0], np.array([1, 0, 0, 0], bool), 10, 0.7)
    assert pose_cases.decision_pinned([3, 7, 6, 2], [0, 0, 1, 0], z, 10, 0.7)          # a later tie still loses to the earlier h
    assert not pose_cases.decision_pinned([6, 7, 3, 2], [1, 0, 0, 0], z, 10, 0.7)     # an earlier tie would win
    assert not pose_cases.decision_pinned([0, 0, 0, 0], [0, 1, 0, 0], z, 10, 0.7)
