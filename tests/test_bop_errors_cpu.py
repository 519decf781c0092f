"""CPU: the BOP pose errors' host side -- the symmetry sets, the fp64 numpy restatements of MSSD / MSPD / VSD and of the depth
rasteriser's pixel rule, the PLY reader and the score table -- against tests/golden/bop_errors.npz (the REAL reference's
get_symmetry_transformations / mssd / mspd / vsd, tests/golden/make_golden_bop.py) and against properties of the written rule."""
import os
import sys

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, G)
import bop_inputs as bi  # noqa: E402

from geometric_aware_dense_matching_amd import evaluation as ev  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(G, "bop_errors.npz")))


@pytest.mark.parametrize("case", bi.SYM_CASES)
def test_symmetry_transformations_equal_the_reference(gold, case):
    R, t = ev.symmetry_transformations(bi.MODEL_INFOS[case], 0.01)
    assert R.dtype == np.float64 and t.dtype == np.float64
    assert R.shape == gold["sym_%s_R" % case].shape and t.shape == (R.shape[0], 3)
    assert R.shape[0] == {"none": 1, "discrete": 2, "continuous": 314, "both": 628}[case]
    assert np.abs(R - gold["sym_%s_R" % case]).max() <= 1e-12
    assert np.abs(t - gold["sym_%s_t" % case]).max() <= 1e-12
    _, t_m = ev.symmetry_transformations(bi.MODEL_INFOS[case], 0.01, scale=0.001)
    assert np.array_equal(t_m, t * 0.001)


def test_identity_comes_first_without_a_continuous_symmetry():
    for case in ("none", "discrete"):
        R, t = ev.symmetry_transformations(bi.MODEL_INFOS[case])
        assert np.array_equal(R[0], np.eye(3)) and not t[0].any()


def test_load_models_info(tmp_path):
    import json
    p = tmp_path / "models_info.json"
    p.write_text(json.dumps({"1": bi.MODEL_INFOS["continuous"], "12": bi.MODEL_INFOS["discrete"]}))
    info = ev.load_models_info(str(p))
    assert sorted(info) == [1, 12] and info[12]["symmetries_discrete"][0][3] == 3.0


@pytest.mark.parametrize("case", bi.SYM_CASES)
def test_mssd_mspd_numpy_equal_the_reference(gold, case):
    R, t = ev.symmetry_transformations(bi.MODEL_INFOS[case], 0.01, scale=0.001)
    mssd, mspd, b3, b2 = ev.mssd_mspd_numpy(gold["ms_RT_est"], gold["ms_RT_gt"], gold["ms_pts"], R, t, bi.LM_K)
    assert np.abs(mssd / gold["mssd_%s" % case] - 1).max() <= 1e-9
    assert np.abs(mspd / gold["mspd_%s" % case] - 1).max() <= 1e-9
    assert b3.dtype == np.int32 and ((0 <= b3) & (b3 < R.shape[0])).all() and ((0 <= b2) & (b2 < R.shape[0])).all()
    Kn = np.stack([bi.LM_K] * 5)                                     # K per instance gives the same
    again = ev.mssd_mspd_numpy(gold["ms_RT_est"], gold["ms_RT_gt"], gold["ms_pts"], R, t, Kn)
    assert np.array_equal(again[0], mssd) and np.array_equal(again[1], mspd)


def test_mssd_first_minimum_wins_a_tie():
    pts, RT_est, RT_gt = bi.mssd_inputs(M=50, n=2)
    R = np.stack([np.eye(3)] * 3)
    t = np.zeros((3, 3))
    _, _, b3, b2 = ev.mssd_mspd_numpy(RT_est, RT_gt, pts, R, t, bi.LM_K)
    assert b3.tolist() == [0, 0] and b2.tolist() == [0, 0]


def test_vsd_numpy_equals_the_reference_exactly(gold):
    err, union, inter, cost = ev.vsd_numpy(gold["vsd_depth_est"], gold["vsd_depth_gt"], gold["vsd_depth_test"], bi.K, bi.DELTA, bi.TAUS,
                                           diameter=float(gold["vsd_diameter"]), return_counts=True)
    assert np.array_equal(err, gold["vsd_errors"])
    assert (err[2] == 1.0).all() and union[2] > 0 and inter[2] == 0     # clipped: the two visible surfaces do not meet
    assert 0 < err[0, 0] < err[1, 0] < 1                                # near is better than far
    per_instance = np.stack([gold["vsd_depth_test"]] * 3)
    assert np.array_equal(ev.vsd_numpy(gold["vsd_depth_est"], gold["vsd_depth_gt"], per_instance, np.stack([bi.K] * 3), bi.DELTA, bi.TAUS,
                                       diameter=float(gold["vsd_diameter"])), err)


def test_vsd_numpy_empty_union_and_tlinear(gold):
    z = np.zeros((1, bi.H, bi.W), np.float32)
    assert (ev.vsd_numpy(z, z, gold["vsd_depth_test"], bi.K, bi.DELTA, bi.TAUS) == 1.0).all()
    d = float(gold["vsd_diameter"])
    step = ev.vsd_numpy(gold["vsd_depth_est"], gold["vsd_depth_gt"], gold["vsd_depth_test"], bi.K, bi.DELTA, bi.TAUS, diameter=d)
    tlin = ev.vsd_numpy(gold["vsd_depth_est"], gold["vsd_depth_gt"], gold["vsd_depth_test"], bi.K, bi.DELTA, bi.TAUS, diameter=d,
                        cost_type="tlinear")
    assert (tlin >= step - 1e-12).all() and (tlin <= 1.0).all()         # min(d / tau, 1) >= [d >= tau]
    with pytest.raises(ValueError):
        ev.vsd_numpy(z, z, gold["vsd_depth_test"], bi.K, bi.DELTA, bi.TAUS, cost_type="other")


def test_stored_depth_images_are_the_restatement_of_today(gold):
    """The fixture's depth images are render_depth_numpy's: a change of the written rule shows here first."""
    verts, faces = bi.mesh()
    est, gt = bi.poses()
    assert np.array_equal(ev.render_depth_numpy(verts, faces, est, bi.K, bi.H, bi.W, bi.NEAR), gold["vsd_depth_est"])
    d_gt = ev.render_depth_numpy(verts, faces, gt[:1], bi.K, bi.H, bi.W, bi.NEAR)
    assert np.array_equal(d_gt[0], gold["vsd_depth_gt"][0])
    assert np.array_equal(bi.make_test_depth(d_gt[0]), gold["vsd_depth_test"])
    assert abs(float(gold["vsd_diameter"]) - bi.diameter(verts)) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# properties of the pixel rule

def test_full_image_quad_fills_every_pixel_once_at_its_depth():
    verts, faces = bi.full_quad(z=0.5)
    d = ev.render_depth_numpy(verts, faces, bi.identity_pose(), bi.K, bi.H, bi.W, bi.NEAR)
    assert d.shape == (1, bi.H, bi.W) and d.dtype == np.float32
    assert (d == np.float32(0.5)).all()
    count = sum((ev.render_depth_numpy(verts, faces[i:i + 1], bi.identity_pose(), bi.K, bi.H, bi.W, bi.NEAR) > 0).astype(int) for i in (0, 1))
    assert (count == 1).all()                                           # the diagonal's pixels belong to exactly one triangle


def _coverage(verts, faces):
    return sum((ev.render_depth_numpy(verts, f[None], bi.identity_pose(), bi.K, bi.H, bi.W, bi.NEAR)[0] > 0).astype(int) for f in faces)


def test_shared_edge_pixels_are_covered_exactly_once():
    z = 0.4

    def back(u, v):
        return [(u - bi.K[0, 2]) / bi.K[0, 0] * z, (v - bi.K[1, 2]) / bi.K[1, 1] * z, z]
    # integer pixel corners: the shared diagonal and the outer edges pass exactly through pixel centres
    verts = np.array([back(5, 4), back(45, 4), back(45, 34), back(5, 34)])
    tri = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    both = _coverage(verts, tri)
    assert both.max() == 1
    on_diagonal = [(4 + 3 * k, 5 + 4 * k) for k in range(1, 10)]       # (row, col) of pixel centres on the edge 0-2
    assert all(both[r, c] == 1 for r, c in on_diagonal)
    other_diagonal = np.array([[0, 1, 3], [1, 2, 3]], dtype=np.int32)  # the same quad split the other way
    assert np.array_equal(_coverage(verts, other_diagonal), both)
    # top-left rule on the quad's outline: the top row and the left column are in, the bottom row and the right column are out
    assert both[4, 5:45].all() and both[4:34, 5].all() and not both[34].any() and not both[:, 45].any()
    assert both.sum() == 40 * 30


def test_flipped_windings_draw_the_same_image():
    verts, faces = bi.mesh()
    _, gt = bi.poses()
    a = ev.render_depth_numpy(verts, faces, gt[:1], bi.K, bi.H, bi.W, bi.NEAR)
    b = ev.render_depth_numpy(verts, faces[:, ::-1].copy(), gt[:1], bi.K, bi.H, bi.W, bi.NEAR)
    assert (a > 0).sum() > 300 and np.array_equal(a, b)


def test_triangle_with_a_vertex_behind_near_draws_nothing():
    verts = np.array([[-0.05, -0.05, 0.3], [0.05, -0.05, 0.3], [0.0, 0.05, 0.3]])
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    assert (ev.render_depth_numpy(verts, tri, bi.identity_pose(), bi.K, bi.H, bi.W, 0.01) > 0).sum() > 50
    verts[2, 2] = 0.005
    assert not ev.render_depth_numpy(verts, tri, bi.identity_pose(), bi.K, bi.H, bi.W, 0.01).any()
    verts[2, 2] = -0.3                                                   # behind the camera
    assert not ev.render_depth_numpy(verts, tri, bi.identity_pose(), bi.K, bi.H, bi.W, 0.0).any()


def test_z_test_keeps_the_nearer_surface():
    verts, faces = bi.mesh()
    _, gt = bi.poses()
    d = ev.render_depth_numpy(verts, faces, gt[:1], bi.K, bi.H, bi.W, bi.NEAR)[0]
    layers = np.stack([ev.render_depth_numpy(verts, f[None], gt[:1], bi.K, bi.H, bi.W, bi.NEAR)[0] for f in faces])
    assert ((layers > 0).sum(0) >= 2).sum() > 300                       # front and back faces overlap
    nearest = np.where(layers > 0, layers, np.inf).min(0)
    assert np.array_equal(d, np.where(np.isinf(nearest), 0, nearest).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------------
# mesh file and scores

def _write_ply(path, verts, faces, binary):
    extra = np.arange(len(verts), dtype=np.float32)
    with open(path, "wb") as f:
        head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment made by a test",
                "element vertex %d" % len(verts), "property float x", "property float y", "property float z", "property float nx",
                "property uchar red", "element face %d" % len(faces), "property list uchar int vertex_indices", "end_header"]
        f.write(("\n".join(head) + "\n").encode())
        if binary:
            rec = np.zeros(len(verts), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("red", "u1")])
            rec["x"], rec["y"], rec["z"], rec["nx"], rec["red"] = verts[:, 0], verts[:, 1], verts[:, 2], extra, 7
            f.write(rec.tobytes())
            fr = np.zeros(len(faces), dtype=[("n", "u1"), ("v", "<i4", (3,))])
            fr["n"], fr["v"] = 3, faces
            f.write(fr.tobytes())
        else:
            for v, e in zip(verts, extra):
                f.write(("%r %r %r %r 7\n" % (float(v[0]), float(v[1]), float(v[2]), float(e))).encode())
            for t in faces:
                f.write(("3 %d %d %d\n" % tuple(t)).encode())


@pytest.mark.parametrize("binary", [False, True])
def test_load_ply_round_trip(tmp_path, binary):
    verts = np.array([[0, 0, 0], [1.5, 0, 0], [0, -2.25, 0], [0, 0, 3.125], [4, 5, 6]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [1, 4, 3]], dtype=np.int32)
    p = str(tmp_path / "m.ply")
    _write_ply(p, verts, faces, binary)
    v, f = ev.load_ply(p)
    assert v.dtype == np.float64 and f.dtype == np.int32
    assert np.array_equal(v, verts.astype(np.float64)) and np.array_equal(f, faces)


def test_load_ply_refuses_what_it_does_not_read(tmp_path):
    p = tmp_path / "bad.ply"
    p.write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nend_header\n")
    with pytest.raises(ValueError, match="not supported"):
        ev.load_ply(str(p))
    p.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                  b"element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n4 0 0 0 0\n")
    with pytest.raises(ValueError, match="triangles"):
        ev.load_ply(str(p))


def test_bop_scores_hand_computed():
    s = ev.BopScores()
    # diameter 0.2: MSSD thresholds 0.01, 0.02, ..., 0.1.  width 1280: MSPD thresholds 10, 20, ..., 100 px.
    s.update("cup", mssd=[0.005, 0.045, 0.2], mspd=[9.0, 55.0, 1000.0], diameter=0.2, width=1280)
    r = s.recalls("cup")
    # instance 0 passes all ten, instance 1 passes theta x 0.2 > 0.045 (0.05 ... 0.1: six; 0.045 < 0.05), instance 2 none
    assert np.allclose(r["mssd"], [1 / 3] * 4 + [2 / 3] * 6)
    assert np.allclose(r["mspd"], [1 / 3] * 5 + [2 / 3] * 5)             # 55 < 60, 70, ..., 100: five
    assert r["vsd"] is None and r["AR_vsd"] is None
    assert abs(r["AR_mssd"] - (10 + 6 + 0) / 30) < 1e-12 and abs(r["AR_mspd"] - (10 + 5 + 0) / 30) < 1e-12
    assert abs(r["AR"] - 0.5 * (16 / 30 + 15 / 30)) < 1e-12              # the mean of the two without VSD
    # an error exactly on a threshold is NOT correct (strict <)
    t = ev.BopScores()
    t.update("o", mssd=[0.05], mspd=[5.0], diameter=1.0, width=640)
    assert t.recalls("o")["mssd"][0] == 0 and t.recalls("o")["mssd"][1] == 1 and t.recalls("o")["mspd"][0] == 0
    # VSD: [n, T] errors at T tolerances; correct when e < theta for each of the ten theta
    v = ev.BopScores()
    vsd = np.array([[0.0] * 10, [0.3] * 5 + [0.12] * 5])
    v.update("o", mssd=[0.0, 0.0], mspd=[0.0, 0.0], vsd=vsd, diameter=1.0, width=640)
    v.missing("o", 2)
    r = v.recalls("o")
    # instance 1: 0.3 < theta for theta = 0.35 ... 0.5 (four) at five taus, 0.12 < theta for 0.15 ... 0.5 (eight) at five taus
    assert abs(r["AR_vsd"] - (100 + 4 * 5 + 8 * 5) / 400) < 1e-12
    assert abs(r["AR_mssd"] - 0.5) < 1e-12 and abs(r["AR"] - (0.5 + 0.5 + 0.4) / 3) < 1e-12
    assert np.allclose(r["vsd"][[0, 2, 6, 9]], [0.25, (10 + 5) / 40, (10 + 5 + 5) / 40, 0.5])


def test_bop_scores_table_and_dump(tmp_path):
    s = ev.BopScores()
    s.update("ape", mssd=[0.001], mspd=[1.0], diameter=0.1, width=640)
    s.update("cat", mssd=[1.0], mspd=[1e3], diameter=0.1, width=640)
    tab = s.table()
    assert tab[0] == ["objects", "ape", "cat", "Avg(2)"]
    names = [row[0] for row in tab[1:]]
    assert names[:2] == ["mssd_0.05", "mssd_0.1"] and names[10] == "AR_mssd" and names[11] == "mspd_5" and names[-1] == "AR"
    assert "AR_vsd" not in names
    assert tab[-1][1:] == ["100.00", "0.00", "50.00"]
    paths = s.dump(str(tmp_path), "lm_test", method_name="ffb6d")
    assert all(os.path.exists(p) for p in paths) and paths[1].endswith("ffb6d_lm_test_bop_tab.txt")
    assert open(paths[1]).read().strip() == s.format()


def test_bop_ops_refuse_cpu_tensors_and_wrong_dtypes():
    import torch
    from geometric_aware_dense_matching_amd import ops
    rt, pts, R, t, K = torch.zeros(2, 3, 4).double(), torch.zeros(8, 3).double(), torch.eye(3).double()[None], torch.zeros(1, 3).double(), \
        torch.eye(3).double()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mssd_mspd(rt, rt, pts, R, t, K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_depth(pts, torch.zeros(1, 3, dtype=torch.int32), rt, K, 4, 4, 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_depth(pts.numpy(), torch.zeros(1, 3, dtype=torch.int32), rt, K, 4, 4, 0.0)
    d = torch.zeros(2, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.vsd_counts(d, d, d, K, 0.015, [0.1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.vsd(d, d, d, K, 0.015, [0.1])


@pytest.mark.gpu
def test_bop_ops_refuse_wrong_dtypes_and_shapes():
    import torch
    from geometric_aware_dense_matching_amd import ops
    c = "cuda:0"
    rt, pts, R, t, K = (a.to(c) for a in (torch.zeros(2, 3, 4).double(), torch.ones(8, 3).double(), torch.eye(3).double()[None],
                                          torch.zeros(1, 3).double(), torch.eye(3).double()))
    with pytest.raises(TypeError):
        ops.mssd_mspd(rt.float(), rt, pts, R, t, K)
    with pytest.raises(TypeError):
        ops.mssd_mspd(rt, rt, pts.float(), R, t, K)
    with pytest.raises(ValueError):
        ops.mssd_mspd(rt, rt[:1], pts, R, t, K)
    with pytest.raises(ValueError):
        ops.mssd_mspd(rt, rt, pts, R, t, K[None])                    # [1,3,3] is neither [3,3] nor [n,3,3]
    f = torch.zeros(1, 3, dtype=torch.int32, device=c)
    with pytest.raises(TypeError):
        ops.render_depth(pts.half(), f, rt, K, 4, 4, 0.0)
    with pytest.raises(TypeError):
        ops.render_depth(pts, f.long(), rt, K, 4, 4, 0.0)
    with pytest.raises(TypeError):
        ops.render_depth(pts, f, rt.float(), K, 4, 4, 0.0)
    d = torch.zeros(2, 4, 4, device=c)
    with pytest.raises(TypeError):
        ops.vsd_counts(d.double(), d, d, K, 0.015, [0.1])
    with pytest.raises(ValueError):
        ops.vsd_counts(d, d, d[:, :2], K, 0.015, [0.1])
    with pytest.raises(ValueError):
        ops.vsd_counts(d, d, d, K, 0.015, [0.1] * 17)
    from geometric_aware_dense_matching_amd._lib import GdmError
    with pytest.raises(GdmError, match="near"):
        ops.render_depth(pts, f, rt, K, 4, 4, -1.0)
