"""CPU: the model-preparation module without a GPU -- the PLY reader with attributes, the three rules of include/gdm.h as their numpy
restatements state them (fill and stay inside, attribute rules, farthest-point order with ties, the first farthest pair), and the
contract of build_model_points with the restatements standing in for the kernels through model_prep._impl, the module's one hook."""
import argparse
import json
import os
import warnings

import numpy as np
import pytest

import model_prep_cases as C
from geometric_aware_dense_matching_amd import evaluation, model_prep as mp

EPS = float(np.finfo(np.float32).eps)


@pytest.fixture
def numpy_ops(monkeypatch):
    monkeypatch.setattr(mp, "_impl", mp._NumpyOps)


# ---- reader ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("with_normals, with_colors", [(True, True), (False, False), (True, False), (False, True)])
def test_reader_returns_the_attributes_the_file_has(tmp_path, binary, with_normals, with_colors):
    verts, faces = C.icosphere(1)
    normals, colors = C.sphere_attributes(verts)
    path = C.write_ply(tmp_path / "m.ply", verts, faces, normals if with_normals else None, colors if with_colors else None, binary)
    v, f, n, c = mp.load_ply(path)
    assert v.dtype == np.float64 and f.dtype == np.int32
    assert np.array_equal(v.astype(np.float32), verts.astype(np.float32)) and np.array_equal(f, faces)      # (ascii: 9 digits)
    if binary:
        assert np.array_equal(v, verts.astype(np.float32).astype(np.float64))
    if with_normals:
        assert n.dtype == np.float32 and np.array_equal(n, normals)
    else:
        assert n is None
    if with_colors:
        assert c.dtype == np.uint8 and np.array_equal(c, colors)
    else:
        assert c is None
    # today's callers: the same two arrays, and only those
    old = evaluation.load_ply(path)
    assert isinstance(old, tuple) and len(old) == 2 and np.array_equal(old[0], v) and np.array_equal(old[1], f)
    assert old[0].dtype == np.float64 and old[1].dtype == np.int32
    two = mp.load_ply(path, attributes=False)
    assert len(two) == 2 and np.array_equal(two[0], v)


def test_vertex_normals_of_a_sphere_point_outwards():
    verts, faces = C.icosphere(2)
    n = mp.vertex_normals_numpy(verts, faces)
    assert n.dtype == np.float64 and np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-12)
    assert (np.sum(n * verts / 50.0, axis=1) > 0.99).all()
    lone = mp.vertex_normals_numpy(np.concatenate([verts, [[0, 0, 0]]]), faces)          # a vertex of no face
    assert np.array_equal(lone[-1], [0, 0, 0]) and np.array_equal(lone[:-1], n)


# ---- the sample rule ---------------------------------------------------------------------------------------------------------
def _barycentric(p, tri):
    """fp64 weights of points p[S,3] with respect to triangle tri[3,3] (least squares in its plane) and the plane residual."""
    e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
    A = np.stack([e1, e2], axis=1)
    uv = np.linalg.lstsq(A, (p - tri[0]).T, rcond=None)[0].T
    nrm = np.cross(e1, e2)
    resid = np.abs((p - tri[0]) @ (nrm / np.linalg.norm(nrm)))
    return np.stack([1 - uv[:, 0] - uv[:, 1], uv[:, 0], uv[:, 1]], axis=1), resid


def _strip_inputs():
    verts, faces = C.strip()
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], dtype=np.float32), (4, 1))
    rgb = np.array([[0, 0, 0], [255, 0, 0], [0, 255, 0], [255, 255, 255]], dtype=np.float32)
    return verts, faces, nrm, rgb


def test_samples_fill_the_triangles_by_area_and_stay_inside():
    verts, faces, nrm, rgb = _strip_inputs()
    cdf = mp.face_cdf(verts, faces)
    assert cdf.dtype == np.int64 and cdf.tolist() == [1 << 24, (1 << 24) + 5592405]          # rint(2^24 / 3)
    S = 65536
    out = mp.surface_sample_numpy(verts, faces, nrm, rgb, cdf, S, seed=C.seed_of("fill"))
    assert out.shape == (S, 9) and out.dtype == np.float32
    p = out[:, :3].astype(np.float64)
    tol = 1e-6
    (w_big, r_big), (w_small, r_small) = (_barycentric(p, verts[f]) for f in faces)
    in_big, in_small = (w_big >= -tol).all(axis=1), (w_small >= -tol).all(axis=1)
    assert (in_big | in_small).all()
    share = float((in_small & ~in_big).mean())
    print("share on the small triangle: %.5f" % share)
    assert abs(share - 0.25) < 0.01                                        # sigma of a Bernoulli share here: 0.0017
    # the plane: five roundings of at most half an ulp of the largest coordinate per component
    assert max(r_big.max(), r_small.max()) <= 8 * EPS * np.abs(verts).max()


def test_a_face_of_weight_zero_is_never_drawn():
    verts, faces, nrm, rgb = _strip_inputs()
    # a degenerate face at a far vertex between the two, through the area rule
    verts3 = np.concatenate([verts, [[100.0, 100.0, 100.0]]])
    faces3 = np.array([faces[0], [4, 4, 4], faces[1]], dtype=np.int32)
    cdf = mp.face_cdf(verts3, faces3)
    assert cdf[1] == cdf[0]
    out = mp.surface_sample_numpy(verts3, faces3, np.concatenate([nrm, nrm[:1]]), np.concatenate([rgb, rgb[:1]]), cdf, 20000,
                                  seed=C.seed_of("degenerate"))
    assert out[:, 0].max() <= 3.0
    # and through a hand-made cdf: weight 0 on the first face, on the last face
    for weights, keep in (([0, 5], 1), ([7, 0], 0)):
        out = mp.surface_sample_numpy(verts, faces, nrm, rgb, np.cumsum(weights).astype(np.int64), 20000, seed=C.seed_of("zero weight"))
        w, _ = _barycentric(out[:, :3].astype(np.float64), verts[faces[keep]])
        assert (w >= -1e-6).all()
    with pytest.raises(ValueError):
        mp.surface_sample_numpy(verts, faces, nrm, rgb, np.zeros(2, dtype=np.int64), 16)
    with pytest.raises(ValueError):
        mp.surface_sample_numpy(verts, faces, nrm, rgb, cdf[:2], 1 << 31)


def test_attribute_rules():
    verts, faces = C.icosphere(2)
    normals, colors = C.sphere_attributes(verts)
    assert colors.min() == 0 and colors.max() == 255
    cdf = mp.face_cdf(verts, faces)
    out = mp.surface_sample_numpy(verts, faces, normals, colors, cdf, 30000, seed=C.seed_of("attributes"))
    length = np.linalg.norm(out[:, 6:9].astype(np.float64), axis=1)
    assert np.abs(length - 1).max() <= 2 * EPS
    rgb = out[:, 3:6]
    assert np.array_equal(rgb, np.floor(rgb)) and rgb.min() >= 0 and rgb.max() <= 255
    # a zero normal stays zero (and is no NaN)
    zero = mp.surface_sample_numpy(verts, faces, np.zeros_like(normals), colors, cdf, 1000, seed=1)
    assert np.array_equal(zero[:, 6:9], np.zeros((1000, 3), dtype=np.float32))
    assert np.array_equal(zero[:, :6], mp.surface_sample_numpy(verts, faces, normals, colors, cdf, 1000, seed=1)[:, :6])
    # the draw is a function of (seed, s) alone: a longer run starts with the shorter one, another seed differs
    assert np.array_equal(out[:500], mp.surface_sample_numpy(verts, faces, normals, colors, cdf, 500, seed=C.seed_of("attributes")))
    assert not np.array_equal(out[:500, :3], mp.surface_sample_numpy(verts, faces, normals, colors, cdf, 500, seed=2)[:, :3])


# ---- farthest-point order --------------------------------------------------------------------------------------------------
def _fps_by_definition(xyz, m):
    """The definition, scalar by scalar in fp32."""
    xyz = xyz.astype(np.float32)
    dist = [np.float32(1e10)] * len(xyz)
    picks = [0]
    for _ in range(1, m):
        last = xyz[picks[-1]]
        best, at = np.float32(-1), -1
        for k in range(len(xyz)):
            dx, dy, dz = xyz[k, 0] - last[0], xyz[k, 1] - last[1], xyz[k, 2] - last[2]
            d2 = np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz)
            dist[k] = min(dist[k], d2)
            if dist[k] > best:
                best, at = dist[k], k
        picks.append(at)
    return np.array(picks, dtype=np.int32)


def lattice():
    g = np.arange(6, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def test_fps_on_a_lattice_takes_the_lowest_index_among_equals():
    xyz = lattice()
    idx = mp.fps_numpy(xyz, 40)
    assert idx.dtype == np.int32 and idx[0] == 0 and idx[1] == 215           # the opposite corner is the only farthest point
    assert np.array_equal(idx, _fps_by_definition(xyz, 40))
    assert len(set(idx.tolist())) == 40
    # the third pick is tied by symmetry (the lattice maps onto itself when the two picked corners swap): the lowest index wins
    d = np.minimum(((xyz - xyz[0]) ** 2).sum(1), ((xyz - xyz[215]) ** 2).sum(1))
    assert (d == d.max()).sum() > 1 and idx[2] == np.flatnonzero(d == d.max())[0]


def test_fps_with_duplicated_points_and_m_equal_n():
    rng = np.random.default_rng(C.seed_of("duplicates"))
    base = rng.standard_normal((30, 3)).astype(np.float32)
    xyz = base[rng.integers(0, 30, 60)]
    idx = mp.fps_numpy(xyz, 60)
    assert np.array_equal(idx, _fps_by_definition(xyz, 60))
    distinct = len(np.unique(xyz, axis=0))
    assert len(set(idx[:distinct].tolist())) == distinct                   # every distinct point once ...
    assert (idx[distinct:] == 0).all()                                     # ... then every distance is 0 and index 0 is the lowest
    with pytest.raises(ValueError):
        mp.fps_numpy(xyz, 61)


# ---- diameter ----------------------------------------------------------------------------------------------------------------
def test_point_diameter_on_the_cube_is_the_first_body_diagonal():
    verts, _ = C.cube()
    pair, d2 = mp.point_diameter_numpy(verts)
    assert pair.dtype == np.int32 and pair.tolist() == [0, 7] and d2 == np.float32(3)
    pair, d2 = mp.point_diameter_numpy(verts[::-1])
    assert pair.tolist() == [0, 7]
    pair, d2 = mp.point_diameter_numpy(np.array([[0, 0, 0], [0, 0, 0]], dtype=np.float32))
    assert pair.tolist() == [0, 1] and d2 == 0


def test_model_diameter_is_the_fp64_pairwise_maximum(numpy_ops):
    rng = np.random.default_rng(C.seed_of("diameter"))
    verts = (rng.standard_normal((500, 3)) * 40).astype(np.float32).astype(np.float64)
    want = max(float(np.linalg.norm(verts[i + 1:] - verts[i], axis=1).max()) for i in range(499))
    got = mp.model_diameter(verts)
    assert isinstance(got, float) and abs(got - want) <= 1e-12 * want


# ---- the pipeline on the restatements ------------------------------------------------------------------------------------------
def _sphere_mesh():
    verts, faces = C.icosphere(3)
    normals, colors = C.sphere_attributes(verts)
    return {"verts": verts, "faces": faces, "normals": normals, "colors": colors}


def test_build_model_points_contract(numpy_ops):
    mesh = _sphere_mesh()
    assert mesh["verts"].shape == (642, 3) and mesh["faces"].shape == (1280, 3)
    table = mp.build_model_points(mesh, 1024, candidates=4096, seed=C.seed_of("contract"))
    assert table.shape == (1024, 9) and table.dtype == np.float32 and table.flags["C_CONTIGUOUS"]
    r = np.linalg.norm(table[:, :3].astype(np.float64), axis=1)
    assert r.max() <= 50.0 * (1 + 4 * EPS) and r.min() > 49.0            # on the facets of a 50 mm sphere: the mesh's unit
    assert np.array_equal(table[:, 3:6], np.floor(table[:, 3:6])) and table[:, 3:6].min() >= 0 and table[:, 3:6].max() <= 255
    assert np.abs(np.linalg.norm(table[:, 6:9].astype(np.float64), axis=1) - 1).max() <= 2 * EPS
    assert (np.sum(table[:, 6:9] * table[:, :3], axis=1) > 0).all()       # outward normals travel with their points
    # nested prefixes, for the same candidates
    small = mp.build_model_points(mesh, 256, candidates=4096, seed=C.seed_of("contract"))
    assert np.array_equal(table[:256], small)
    # a farthest-point order: the spacing of the first k rows shrinks as k grows
    d = np.linalg.norm(table[:64, None, :3] - table[None, :64, :3], axis=-1) + np.eye(64) * 1e9
    assert d[:16, :16].min() > d.min()


def test_build_model_points_from_vertices_and_its_refusals(numpy_ops, tmp_path):
    mesh = _sphere_mesh()
    table = mp.build_model_points(mesh, 128, source="vertices")
    rows = np.concatenate([mesh["verts"].astype(np.float32), mesh["colors"].astype(np.float32), mesh["normals"]], axis=1)
    order = mp.fps_numpy(rows[:, :3], 128)
    assert order[0] == 0 and np.array_equal(table, rows[order])
    with pytest.raises(ValueError, match="vertices"):
        mp.build_model_points(mesh, 643, source="vertices")
    with pytest.raises(ValueError, match="candidates"):
        mp.build_model_points(mesh, 64, candidates=63)
    with pytest.raises(ValueError, match="source"):
        mp.build_model_points(mesh, 64, source="faces")
    with pytest.raises(ValueError, match="outside"):
        mp.build_model_points({"verts": mesh["verts"][:10], "faces": mesh["faces"]}, 4)
    # a file without colours or normals: 128 with a warning, normals from the faces
    path = C.write_ply(tmp_path / "bare.ply", mesh["verts"], mesh["faces"], binary=True)
    with pytest.warns(UserWarning, match="128"):
        bare = mp.build_model_points(path, 64, candidates=512)
    assert (bare[:, 3:6] == 128).all()
    assert (np.sum(bare[:, 6:9] * bare[:, :3], axis=1) > 49.0).all()


def test_command_line_writes_one_file_per_object(numpy_ops, tmp_path, capsys):
    mesh = _sphere_mesh()
    models = tmp_path / "models"
    models.mkdir()
    C.write_ply(models / "obj_000001.ply", mesh["verts"], mesh["faces"], mesh["normals"], mesh["colors"], binary=True)
    C.write_ply(models / "obj_000005.ply", mesh["verts"] * 0.5, mesh["faces"], mesh["normals"], mesh["colors"], binary=False)
    (models / "models_info.json").write_text(json.dumps({"1": {"diameter": 100.0}, "5": {"diameter": 50.0}}))
    out = tmp_path / "kps"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert mp.main(["--models-dir", str(models), "--out-dir", str(out), "--n-points", "64", "--candidates", "256"]) == 0
    text = capsys.readouterr().out
    for obj, scale in ((1, 1.0), (5, 0.5)):
        table = np.load(out / ("obj_%06d_fps.npy" % obj))
        v, f, n, c = mp.load_ply(str(models / ("obj_%06d.ply" % obj)))
        want = mp.build_model_points({"verts": v, "faces": f, "normals": n, "colors": c}, 64, candidates=256)
        assert table.dtype == np.float32 and np.array_equal(table, want)
        assert np.linalg.norm(table[:, :3], axis=1).max() <= 50.0 * scale * (1 + 1e-6)
    assert text.count("relative difference") == 2 and "obj 1:" in text and "obj 5:" in text
    # the icosphere's antipodal vertices are 100 mm apart up to the fp32 the file stores
    assert abs(mp.model_diameter(mp.load_ply(str(models / "obj_000001.ply"))[0]) - 100.0) < 1e-4


def test_models_dir_builds_the_table_when_the_file_is_missing(numpy_ops, tmp_path):
    from geometric_aware_dense_matching_amd import synthetic, train_lm
    mesh = _sphere_mesh()
    models = tmp_path / "models"
    models.mkdir()
    path = C.write_ply(models / "obj_000001.ply", mesh["verts"], mesh["faces"], mesh["normals"], mesh["colors"], binary=True)
    ds = {"model_pth": str(tmp_path / "kps"), "diameters": {1: 100.0, 2: 80.0}}
    args = train_lm.build_parser().parse_args(["--n-mesh", "16", "--models-dir", str(models)])
    assert args.models_dir == str(models)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = train_lm._model_points(args, ds, 1)
        assert np.array_equal(got, mp.build_model_points(path, 16))
    # no mesh for object 2, and no flag at all: what it returned before
    assert np.array_equal(train_lm._model_points(args, ds, 2), synthetic.make_model_points(2, 16, 80.0))
    plain = train_lm.build_parser().parse_args(["--n-mesh", "16"])
    assert plain.models_dir is None
    assert np.array_equal(train_lm._model_points(plain, ds, 1), synthetic.make_model_points(1, 16, 100.0))
    assert np.array_equal(train_lm._model_points(argparse.Namespace(n_mesh=16), ds, 1), synthetic.make_model_points(1, 16, 100.0))
    # a model file still wins over the mesh
    os.makedirs(ds["model_pth"])
    np.save(os.path.join(ds["model_pth"], "obj_000001_fps.npy"), np.ones((16, 9), dtype=np.float32))
    assert np.array_equal(train_lm._model_points(args, ds, 1), np.ones((16, 9), dtype=np.float32))
