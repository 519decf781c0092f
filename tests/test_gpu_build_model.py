"""GPU: the three model-preparation entries against their numpy restatements, bit for bit (surface_sample, furthestsampling_wide --
also against ops.furthestsampling --, point_diameter), the pipeline from a PLY file to a table the constructors load, the command
line in a child process, train_lm's --models-dir, and one guarded run of each entry (tests/guard_bands.py)."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import guard_bands as gb
import model_prep_cases as C
from geometric_aware_dense_matching_amd import model_prep as mp, ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- surface_sample ------------------------------------------------------------------------------------------------------------
def _sample_mesh(name):
    """(verts f32, faces, normals f32, colours f32, cdf)"""
    if name == "icosphere":
        verts, faces = C.icosphere(3)
        normals, colors = C.sphere_attributes(verts)
        assert verts.shape == (642, 3) and faces.shape == (1280, 3)
        return verts.astype(np.float32), faces, normals, colors.astype(np.float32), mp.face_cdf(verts, faces)
    verts, faces = C.strip()
    normals = mp.vertex_normals_numpy(verts, faces).astype(np.float32)
    normals[3] = 0                                                         # one zero normal: interpolated, not divided by zero
    colors = np.array([[0, 0, 0], [255, 0, 0], [0, 255, 0], [255, 255, 255]], dtype=np.float32)
    if name == "strip":
        return verts.astype(np.float32), faces, normals, colors, mp.face_cdf(verts, faces)
    assert name == "zero weight"                                           # a degenerate face between the two, and a face of weight 0
    verts = np.concatenate([verts, [[100.0, 100.0, 100.0]]])
    faces = np.array([faces[0], [4, 4, 4], faces[1], faces[0]], dtype=np.int32)
    cdf = np.cumsum([1 << 24, 0, 5592405, 0]).astype(np.int64)
    assert np.array_equal(cdf[:3], mp.face_cdf(verts, faces[:3]))
    return verts.astype(np.float32), faces, np.concatenate([normals, normals[:1]]), np.concatenate([colors, colors[:1]]), cdf


@pytest.mark.parametrize("mesh", ["icosphere", "strip", "zero weight"])
def test_surface_sample_equals_its_restatement_bit_for_bit(mesh):
    verts, faces, normals, colors, cdf = _sample_mesh(mesh)
    dev = [_t(a) for a in (verts, faces, normals, colors, cdf)]
    for S in (1, 63, 4097):
        for seed in (C.seed_of(mesh), 0):
            want = mp.surface_sample_numpy(verts, faces, normals, colors, cdf, S, seed)
            got = ops.surface_sample(*dev, S, seed)
            assert got.shape == (S, 9) and got.dtype == torch.float32
            got = got.cpu().numpy()
            for ch in range(9):
                assert np.array_equal(_bits(got[:, ch]), _bits(want[:, ch])), (S, seed, ch)
            again = ops.surface_sample(*dev, S, seed).cpu().numpy()
            assert np.array_equal(_bits(again), _bits(got))
    if mesh == "zero weight":
        assert got[:, 0].max() <= 3.0                                      # S = 4097: nothing at the far vertex
    # colours may come as uint8
    u8 = ops.surface_sample(dev[0], dev[1], dev[2], _t(colors.astype(np.uint8)), dev[4], 63, 5).cpu().numpy()
    assert np.array_equal(_bits(u8), _bits(mp.surface_sample_numpy(verts, faces, normals, colors, cdf, 63, 5)))


def test_surface_sample_refuses_before_any_launch():
    verts, faces, normals, colors, cdf = _sample_mesh("strip")
    dev = [_t(a) for a in (verts, faces, normals, colors, cdf)]
    with pytest.raises(ValueError, match="cdf"):
        ops.surface_sample(dev[0], dev[1], dev[2], dev[3], torch.zeros_like(dev[4]), 16)
    with pytest.raises(ValueError, match="S="):
        ops.surface_sample(*dev, 1 << 31)
    with pytest.raises(ValueError, match="outside"):
        ops.surface_sample(dev[0], dev[1] + 2, dev[2], dev[3], dev[4], 16)
    with pytest.raises(ops._lib.GdmError, match="S="):
        ops.call("gdm_surface_sample_hip", dev[0], dev[1], dev[2], dev[3], dev[4], 4, 2, 1 << 31, 0, torch.empty(9, device="cuda"))
    torch.cuda.synchronize()


# ---- furthestsampling_wide ---------------------------------------------------------------------------------------------------
def _cloud(name, n):
    return np.random.default_rng(C.seed_of(name)).standard_normal((n, 3)).astype(np.float32)


def _check_fps(xyz, m, groups):
    """xyz f32[B,n,3]"""
    dev = _t(xyz)
    wide = ops.furthestsampling_wide(dev, m, groups)
    assert wide.shape == (xyz.shape[0], m) and wide.dtype == torch.int32
    one = ops.furthestsampling(dev, m)
    assert torch.equal(wide, one), (xyz.shape, m, groups)
    wide = wide.cpu().numpy()
    for b in range(xyz.shape[0]):
        assert np.array_equal(wide[b], mp.fps_numpy(xyz[b], m)), (xyz.shape, m, groups, b)
    return wide


@pytest.mark.parametrize("n, m, groups", [(1, 1, 1), (300, 300, 1), (300, 17, 3), (5000, 64, 64), (5001, 64, 7), (20000, 64, 0)])
def test_fps_wide_equals_the_single_workgroup_form_and_the_restatement(n, m, groups):
    _check_fps(_cloud("fps %d" % n, n)[None], m, groups)


@pytest.mark.parametrize("groups", [1, 5])
def test_fps_wide_on_a_lattice_with_ties_everywhere(groups):
    g = np.arange(6, dtype=np.float32)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    idx = _check_fps(xyz[None], 216, groups)                               # slices of 44: ties straddle their boundaries
    assert idx[0, 0] == 0 and idx[0, 1] == 215 and sorted(idx[0].tolist()) == list(range(216))


def test_fps_wide_with_duplicated_points_and_more_groups_than_points():
    rng = np.random.default_rng(C.seed_of("fps duplicates"))
    xyz = _cloud("fps base", 70)[rng.integers(0, 70, 200)]
    idx = _check_fps(xyz[None], 200, 4)
    distinct = len(np.unique(xyz, axis=0))
    assert (idx[0, distinct:] == 0).all()
    _check_fps(xyz[None, :9], 9, 16)                                       # seven workgroups with an empty slice


def test_fps_wide_batch_of_two_clouds():
    xyz = np.stack([_cloud("fps batch 0", 1500), _cloud("fps batch 1", 1500) * 3 + 1])
    idx = _check_fps(xyz, 33, 6)
    assert not np.array_equal(idx[0], idx[1])
    _check_fps(xyz, 32, 0)


def test_fps_wide_refusals():
    xyz = _t(_cloud("fps refusals", 10)[None])
    for m, groups in ((11, 1), (0, 1), (4, 1025), (4, -1)):
        with pytest.raises(ops._lib.GdmError, match="gdm_fps_wide_hip"):
            ops.furthestsampling_wide(xyz, m, groups)
    assert ops.call("gdm_fps_wide_groups", 1) == 1 and ops.call("gdm_fps_wide_groups", 262144) == 256
    assert ops.call("gdm_fps_wide_groups", 1 << 30) == 1024 and ops.call("gdm_fps_wide_groups", 0) == 0
    torch.cuda.synchronize()


# ---- point_diameter ------------------------------------------------------------------------------------------------------------
def _check_diameter(xyz):
    pair, d2 = ops.point_diameter(_t(xyz))
    assert pair.dtype == torch.int32 and pair.shape == (2,) and d2.dtype == torch.float32 and d2.shape == (1,)
    want_pair, want_d2 = mp.point_diameter_numpy(xyz)
    assert pair.cpu().numpy().tolist() == want_pair.tolist(), len(xyz)
    assert _bits(d2.cpu().numpy())[0] == _bits(np.array([want_d2], dtype=np.float32))[0]
    again = ops.point_diameter(_t(xyz))
    assert torch.equal(again[0], pair) and torch.equal(again[1], d2)
    return want_pair.tolist()


@pytest.mark.parametrize("V", [2, 257, 1000])
def test_point_diameter_equals_its_restatement(V):
    _check_diameter(_cloud("diameter %d" % V, V))


def test_point_diameter_cube_ties_and_the_last_tile():
    verts, _ = C.cube()
    assert _check_diameter(verts.astype(np.float32)) == [0, 7]
    assert _check_diameter(np.tile(verts.astype(np.float32), (40, 1))) == [0, 7]          # 320 points: the tie repeats in every tile pair
    xyz = _cloud("diameter last tile", 600)
    xyz[598], xyz[599] = (-50, 0, 0), (50, 1, 0)
    assert _check_diameter(xyz) == [598, 599]                              # both ends in the last, ragged tile
    xyz[598], xyz[3] = (0, 0, 0), (-50, 0, 0)
    assert _check_diameter(xyz) == [3, 599]
    assert _check_diameter(np.zeros((300, 3), dtype=np.float32)) == [0, 1]
    with pytest.raises(ops._lib.GdmError, match="V=1"):
        ops.point_diameter(_t(xyz[:1]))
    torch.cuda.synchronize()


# ---- end to end --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_ply(tmp_path_factory):
    verts, faces = C.icosphere(3)
    normals, colors = C.sphere_attributes(verts)
    return C.write_ply(tmp_path_factory.mktemp("mesh") / "obj_000001.ply", verts, faces, normals, colors, binary=True)


def test_ply_to_model_table_end_to_end(sphere_ply, monkeypatch):
    from geometric_aware_dense_matching_amd import splinecnn
    table = mp.build_model_points(sphere_ply, 512, candidates=8192)
    assert table.shape == (512, 9) and table.dtype == np.float32
    with monkeypatch.context() as m:
        m.setattr(mp, "_impl", mp._NumpyOps)
        want = mp.build_model_points(sphere_ply, 512, candidates=8192)
    assert np.array_equal(_bits(table), _bits(want))
    assert np.array_equal(table[:128], mp.build_model_points(sphere_ply, 128, candidates=8192))
    # both forms of the farthest-point order serve the pipeline with the same rows
    monkeypatch.setattr(mp, "FPS_WIDE_MIN_N", 8193 if mp.FPS_WIDE_MIN_N <= 8192 else 1)
    assert np.array_equal(table, mp.build_model_points(sphere_ply, 512, candidates=8192))
    monkeypatch.undo()
    verts = mp.load_ply(sphere_ply)[0]
    assert abs(mp.model_diameter(verts) - 100.0) < 1e-4
    mesh = splinecnn.SplineCNN_Mesh({"n_mesh_node": 512}, 1, model_points=table).cuda()
    assert mesh.xyz.shape == (512, 3) and torch.equal(mesh.xyz.cpu(), torch.from_numpy(table[:, :3] / np.float32(1000.0)))
    ei, ea = splinecnn.build_mesh_graph(mesh.xyz, k=4)
    assert ei.shape == (2, 4 * 512) and ea.shape == (4 * 512, 3) and bool(torch.isfinite(ea).all())


def test_command_line_in_a_child_process(sphere_ply, tmp_path):
    models = tmp_path / "models"
    models.mkdir()
    verts, faces, normals, colors = mp.load_ply(sphere_ply)
    C.write_ply(models / "obj_000001.ply", verts, faces, normals, colors, binary=True)
    C.write_ply(models / "obj_000002.ply", verts * 0.5, faces, normals, colors, binary=False)
    (models / "models_info.json").write_text('{"1": {"diameter": 100.0}, "2": {"diameter": 50.0}}')
    out = tmp_path / "kps"
    run = subprocess.run([sys.executable, "-m", "geometric_aware_dense_matching_amd.model_prep", "--models-dir", str(models), "--out-dir",
                          str(out), "--n-points", "256", "--candidates", "4096", "--seed", "3"], cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.count("relative difference") == 2
    for obj in (1, 2):
        table = np.load(out / ("obj_%06d_fps.npy" % obj))
        want = mp.build_model_points(str(models / ("obj_%06d.ply" % obj)), 256, candidates=4096, seed=3)
        assert table.dtype == np.float32 and np.array_equal(_bits(table), _bits(want))


def test_train_lm_models_dir(sphere_ply, tmp_path):
    from geometric_aware_dense_matching_amd import synthetic, train_lm
    ds = {"model_pth": str(tmp_path / "none"), "diameters": {1: 100.0}}
    args = train_lm.build_parser().parse_args(["--n-mesh", "64", "--models-dir", os.path.dirname(sphere_ply)])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = train_lm._model_points(args, ds, 1)
    assert got.shape == (64, 9) and np.array_equal(got, mp.build_model_points(sphere_ply, 64))
    plain = train_lm.build_parser().parse_args(["--n-mesh", "64"])
    assert np.array_equal(train_lm._model_points(plain, ds, 1), synthetic.make_model_points(1, 64, 100.0))


# ---- guard bands -------------------------------------------------------------------------------------------------------------
def test_the_three_entries_stay_inside_their_tensors(monkeypatch):
    verts, faces, normals, colors, cdf = _sample_mesh("icosphere")
    xyz = _cloud("guarded", 3001)
    with gb.filled_empties(), gb.guarded_calls(monkeypatch) as st:
        out = ops.surface_sample(*[_t(a) for a in (verts, faces, normals, colors, cdf)], 1000, 7)
        idx = ops.furthestsampling_wide(_t(xyz[None]), 40, 7)
        idx0 = ops.furthestsampling_wide(_t(xyz[None]), 41, 0)
        pair, d2 = ops.point_diameter(_t(xyz))
    assert st.counts["gdm_surface_sample_hip"] == 1 and st.counts["gdm_fps_wide_hip"] == 2 and st.counts["gdm_point_diameter_hip"] == 1
    # the bands and the const inputs were checked by the wrapper; here: no output element kept the allocator's fill
    assert bool(torch.isfinite(out).all())
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(mp.surface_sample_numpy(verts, faces, normals, colors, cdf, 1000, 7)))
    assert np.array_equal(idx[0].cpu().numpy(), mp.fps_numpy(xyz, 40)) and np.array_equal(idx0[0].cpu().numpy(), mp.fps_numpy(xyz, 41))
    want_pair, want_d2 = mp.point_diameter_numpy(xyz)
    assert pair.cpu().numpy().tolist() == want_pair.tolist() and float(d2[0]) == float(want_d2)
