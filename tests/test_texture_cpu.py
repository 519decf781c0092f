"""CPU: textured meshes on the host -- the PLY reader's texture coordinates, THE TEXTURE RULE of include/gdm.h as
texture.py restates it (mips, fetch, level choice), render.render_frames_numpy and model_prep.surface_sample_tex_numpy with a
texture, and the refusals of the new entries, which come before any HIP call."""
import ctypes
import warnings

import numpy as np
import pytest

import texture_cases as tc
from geometric_aware_dense_matching_amd import evaluation as ev
from geometric_aware_dense_matching_amd import model_prep as mp
from geometric_aware_dense_matching_amd import render, texture


# ---- the PLY reader ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("names", [("texture_u", "texture_v"), ("u", "v"), ("s", "t")])
def test_load_ply_gathers_vertex_uv_through_the_faces(tmp_path, binary, names):
    verts, faces = tc.tetrahedron()
    vuv = np.random.RandomState(1).rand(len(verts), 2).astype(np.float32)
    p = str(tmp_path / "m.ply")
    tc.write_ply(p, verts, faces, binary, vertex_uv=vuv, uv_names=names, texture_file="obj_000001.png")
    v, f, nr, c, uv, name = ev.load_ply(p, attributes=True, texcoords=True)
    assert np.array_equal(v, verts.astype(np.float64)) and np.array_equal(f, faces) and nr is None and c is None
    assert uv.dtype == np.float32 and uv.shape == (3, 3, 2) and np.array_equal(uv, vuv[faces])
    assert name == "obj_000001.png"
    v2, f2, uv2, name2 = ev.load_ply(p, texcoords=True)                    # without the vertex attributes: (verts, faces, uv, name)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and np.array_equal(uv2, uv) and name2 == name
    assert len(ev.load_ply(p)) == 2 and len(ev.load_ply(p, attributes=True)) == 4          # today's tuples stay as they are


@pytest.mark.parametrize("binary", [False, True])
def test_load_ply_reads_a_face_texcoord_list_and_keeps_its_seam(tmp_path, binary):
    verts, faces = tc.tetrahedron()
    fuv = np.random.RandomState(2).rand(len(faces), 6).astype(np.float32)          # vertex 0 gets another (u, v) in every face: a seam
    p = str(tmp_path / "m.ply")
    tc.write_ply(p, verts, faces, binary, face_uv=list(fuv))
    v, f, uv, name = ev.load_ply(p, texcoords=True)
    assert np.array_equal(f, faces) and np.array_equal(uv, fuv.reshape(-1, 3, 2)) and name is None
    assert not np.array_equal(uv[0, 0], uv[1, 0])
    v0, f0 = ev.load_ply(p)                                                # the extra face properties do not disturb the plain read
    assert np.array_equal(v0, v) and np.array_equal(f0, f)


@pytest.mark.parametrize("binary", [False, True])
def test_load_ply_without_texture_coordinates_gives_none(tmp_path, binary):
    verts, faces = tc.tetrahedron()
    p = str(tmp_path / "m.ply")
    tc.write_ply(p, verts, faces, binary)
    assert ev.load_ply(p, attributes=True, texcoords=True)[4:] == (None, None)


def test_load_ply_refuses_a_ragged_texcoord_list(tmp_path):
    verts, faces = tc.tetrahedron()
    p = str(tmp_path / "m.ply")
    tc.write_ply(p, verts, faces, False, face_uv=[[0.1] * 6, [0.2] * 4, [0.3] * 6])
    with pytest.raises(ValueError, match="texcoord.*6 coordinates"):
        ev.load_ply(p, texcoords=True)
    tc.write_ply(p, verts, faces, True, face_uv=[[0.1] * 6, [0.2] * 4, [0.3] * 6])
    with pytest.raises(ValueError):
        ev.load_ply(p, texcoords=True)


def test_load_mesh_reads_the_named_image_beside_the_file(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    verts, faces = tc.tetrahedron()
    img = tc.image(5, 7, 3)
    Image.fromarray(img).save(str(tmp_path / "obj_000001.png"))
    p = str(tmp_path / "obj_000001.ply")
    tc.write_ply(p, verts, faces, True, vertex_uv=np.zeros((len(verts), 2), np.float32), texture_file="obj_000001.png")
    m = mp.load_mesh(p)
    assert np.array_equal(m["texture"], img) and m["uv"].shape == (3, 3, 2) and m["texture_file"].endswith("obj_000001.png")
    tc.write_ply(p, verts, faces, True, vertex_uv=np.zeros((len(verts), 2), np.float32), texture_file="missing.png")
    with pytest.warns(UserWarning, match="missing.png"):
        assert "texture" not in mp.load_mesh(p)


# ---- mips ---------------------------------------------------------------------------------------------------------------------------
def test_mips_of_a_constant_image_stay_constant():
    img = np.tile(np.array([7, 130, 255], dtype=np.uint8), (9, 21, 1))
    pyr = texture.build_mips_numpy(img)
    assert pyr.shape == (texture.pyramid_texels(9, 21), 4) and pyr.dtype == np.uint8
    assert (pyr == np.array([7, 130, 255, 0], dtype=np.uint8)).all()


@pytest.mark.parametrize("h,w,want", [(1, 1, [(1, 1)]), (3, 5, [(3, 5), (1, 2), (1, 1)]), (7, 1, [(7, 1), (3, 1), (1, 1)]),
                                      (130, 67, [(130, 67), (65, 33), (32, 16), (16, 8), (8, 4), (4, 2), (2, 1), (1, 1)])])
def test_level_shapes(h, w, want):
    """5 x 3, 1 x 7 and 67 x 130 are width x height."""
    assert texture.level_shapes(h, w) == want and texture.full_levels(h, w) == len(want)
    pyr = texture.build_mips_numpy(tc.image(h, w, 5))
    assert len(pyr) == sum(a * b for a, b in want) == texture.pyramid_texels(h, w)
    assert np.array_equal(texture.level_view(pyr, h, w, 0)[..., :3], tc.image(h, w, 5))
    with pytest.raises(ValueError):
        texture.level_shapes(h, w, len(want) + 1)


def test_mip_of_a_2_by_2_image_by_hand():
    img = np.array([[[0, 1, 255], [1, 2, 255]], [[1, 3, 254], [0, 4, 255]]], dtype=np.uint8)
    # r: (0 + 1 + 1 + 0 + 2) >> 2 = 1;  g: (1 + 2 + 3 + 4 + 2) >> 2 = 3;  b: (255 + 255 + 254 + 255 + 2) >> 2 = 255
    pyr = texture.build_mips_numpy(img)
    assert pyr.shape == (5, 4) and pyr[4].tolist() == [1, 3, 255, 0]
    # 3 x 1 (width 3): the second source index of texel 0 is 1, and the level is 1 x 1: texel 2 is not read
    row = np.array([[[10, 0, 0], [13, 0, 0], [200, 0, 0]]], dtype=np.uint8)
    assert texture.build_mips_numpy(row)[3].tolist() == [(10 + 13 + 10 + 13 + 2) >> 2, 0, 0, 0]


# ---- fetch and level ------------------------------------------------------------------------------------------------------------------
def test_fetch_at_a_texel_centre_returns_the_texel_and_flip_v_turns_the_rows():
    img = tc.image(8, 16, 6)
    pyr = texture.build_mips_numpy(img)
    ys, xs = np.meshgrid(np.arange(8), np.arange(16), indexing="ij")
    u, v = (xs + 0.5) / 16.0, (ys + 0.5) / 8.0
    assert np.array_equal(texture.fetch_numpy(pyr, 8, 16, 0, u, v, flip_v=False), img)
    assert np.array_equal(texture.fetch_numpy(pyr, 8, 16, 0, u, v, flip_v=True), img[::-1])
    assert np.array_equal(texture.fetch_numpy(pyr, 8, 16, 0, u, 1.0 - v), img)                          # the default flips
    lv1 = texture.level_view(pyr, 8, 16, 1)[..., :3]
    assert np.array_equal(texture.fetch_numpy(pyr, 8, 16, 1, (xs[:4, :8] + 0.5) / 8.0, (ys[:4, :8] + 0.5) / 4.0, flip_v=False), lv1)
    # half way between two texel centres: fx = 128, the integer blend by hand
    a, b = img[2, 3].astype(np.int64), img[2, 4].astype(np.int64)
    want = ((a * 128 + b * 128) * 256 + 32768) >> 16
    assert np.array_equal(texture.fetch_numpy(pyr, 8, 16, 0, 4.0 / 16.0, 2.5 / 8.0, flip_v=False), want)


def test_fetch_clamps_to_the_edge_and_sends_a_non_finite_coordinate_to_texel_0():
    img = tc.image(4, 4, 7)
    pyr = texture.build_mips_numpy(img)
    f = lambda u, v: texture.fetch_numpy(pyr, 4, 4, 0, u, v, flip_v=False)
    assert np.array_equal(f(-3.0, -0.1), img[0, 0]) and np.array_equal(f(1.0, 1.0), img[3, 3]) and np.array_equal(f(7.5, 0.125), img[0, 3])
    assert np.array_equal(f(-1e300, 1e300), img[3, 0]) and np.array_equal(f(0.0, 0.0), img[0, 0])
    for bad in (np.nan, np.inf, -np.inf):
        assert np.array_equal(f(bad, 0.9), img[0, 0]) and np.array_equal(f(0.9, bad), img[0, 0])
    assert np.array_equal(texture.fetch_numpy(pyr, 4, 4, 1, np.nan, 0.9), texture.level_view(pyr, 4, 4, 1)[0, 0, :3])


def test_level_boundaries_at_rho2_exactly_1_4_and_16():
    lv = lambda d, L=6, **kw: int(texture.mip_level_numpy(0.0, 0.0, d, 0.0, 0.0, 0.0, L, **kw))
    up = lambda x: float(np.nextafter(x, np.inf))
    assert [lv(1.0), lv(2.0), lv(4.0)] == [0, 1, 2]                        # rho2 = 1, 4, 16: the boundary belongs to the finer level
    assert [lv(up(1.0)), lv(up(2.0)), lv(up(4.0))] == [1, 2, 3]
    assert lv(0.0) == 0 and lv(1e9) == 5 and lv(1e9, L=1) == 0 and lv(np.nan) == 5 and lv(np.inf) == 5
    assert lv(0.5, fine=False) == 5                                        # a neighbour with Q <= 0
    # the larger of the two directions decides, each direction's square sum on its own
    assert int(texture.mip_level_numpy(1.0, 1.0, 1.5, 1.5, 1.0, 3.0, 6)) == 1
    assert int(texture.mip_level_numpy(1.0, 1.0, 2.2, 2.2, 1.0, 1.1, 6)) == 1          # 1.2^2 + 1.2^2 = 2.88


# ---- the frame restatement ----------------------------------------------------------------------------------------------------------
def test_untextured_scene_goes_through_the_untextured_path_with_the_same_output():
    case = tc.textured_scene(*tc.SIZES[0], k_per_instance=True)
    args, kw = tc.render_args(case)
    plain = [m[:4] for m in case["meshes"]]
    a = render.render_frames_numpy(render.SceneMeshes(plain, device=None), *args, **kw)
    assert "tex_level" not in a
    # the same scene with a texture that no slot shows: every drawn pixel takes the vertex-colour branch of the textured path
    spare = case["meshes"][0][:2] + (None, None) + case["meshes"][0][4:]
    b = render.render_frames_numpy(render.SceneMeshes(plain + [spare], device=None), *args, **kw)
    assert (b.pop("tex_level") == -1).all()
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_fronto_parallel_quad_reproduces_its_texture_texel_for_pixel():
    """K = (64, 64, 0, 0), a quad at z = 1 whose corners project to x = 3.5, 11.5 and y = 2.5, 10.5, an 8 x 8 texture: pixel
    (4 + i, 3 + j) samples u = (i + 0.5) / 8, 1 - v = (j + 0.5) / 8 exactly (every weight is an integer over 2^22), the footprint is
    one texel (rho2 = 1: level 0) and ambient = 1 leaves the fetched level as it is."""
    img = tc.image(8, 8, 8)
    x0, x1, y0, y1 = 3.5 / 64, 11.5 / 64, 2.5 / 64, 10.5 / 64
    verts = np.array([[x0, y0, 1], [x1, y0, 1], [x1, y1, 1], [x0, y1, 1]], dtype=np.float64)
    faces = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    corner = np.array([[0, 1], [1, 1], [1, 0], [0, 0]], dtype=np.float32)  # per vertex: gathered by SceneMeshes
    nrm = np.tile(np.array([0, 0, -1], dtype=np.float32), (4, 1))
    scene = render.SceneMeshes([(verts, faces, None, nrm, corner, img)], device=None)
    K = np.array([[64.0, 0, 0], [0, 64.0, 0], [0, 0, 1]])
    out = render.render_frames_numpy(scene, [[0]], tc.pose(np.eye(3), (0, 0, 0))[None, None], K, 16, 16, ambient=1.0, near=tc.NEAR)
    assert (out["inst"][0, 3:11, 4:12] == 1).all() and out["inst"].sum() == 64
    assert (out["tex_level"][0, 3:11, 4:12] == 0).all()
    assert np.array_equal(out["rgb"][0, 3:11, 4:12], img)
    flipped = render.SceneMeshes([(verts, faces, None, nrm, corner, img)], device=None, flip_v=False)
    out = render.render_frames_numpy(flipped, [[0]], tc.pose(np.eye(3), (0, 0, 0))[None, None], K, 16, 16, ambient=1.0, near=tc.NEAR)
    assert np.array_equal(out["rgb"][0, 3:11, 4:12], img[::-1])


def test_textured_restatement_uses_the_levels_the_scene_was_posed_for():
    for frame, tex in tc.SIZES:
        case = tc.textured_scene(frame, tex, k_per_instance=False)
        args, kw = tc.render_args(case)
        out = render.render_frames_numpy(render.SceneMeshes(case["meshes"], device=None), *args, **kw)
        far, near = out["tex_level"][0], out["tex_level"][1]
        assert not out["ambiguous"].any()
        assert (far >= 0).sum() >= 4 and far[far >= 0].min() >= 2                              # far: minified
        assert (near == 0).sum() > 0.2 * near.size and near.max() >= 2                         # near: magnified; its limb grazes
        assert ((out["inst"][1] == 2) & (near >= 0)).sum() > 20 and (out["tex_level"][out["inst"] == 3] == -1).all()
        assert (out["tex_level"][0][out["inst"][0] == 2] == -1).all()                          # the vertex-coloured object


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------
def test_surface_sample_tex_numpy_keeps_the_draws_and_fetches_the_colour():
    m = render.demo_mesh(level=1, seed=5, textured=True, tex_size=8)
    verts, faces, nrm = m["verts"].astype(np.float32), m["faces"], m["normals"]
    rgb = np.zeros((len(verts), 3), dtype=np.float32)
    cdf = mp.face_cdf(m["verts"], faces)
    pyr = texture.build_mips_numpy(m["texture"])
    row = (0, 16, 8, 5)
    S = 1000
    plain = mp.surface_sample_numpy(verts, faces, nrm, rgb, cdf, S, seed=9)
    tex = mp.surface_sample_tex_numpy(verts, faces, nrm, rgb, cdf, m["uv"], pyr, row, S, seed=9)
    assert np.array_equal(plain[:, :3].view(np.uint32), tex[:, :3].view(np.uint32))
    assert np.array_equal(plain[:, 6:].view(np.uint32), tex[:, 6:].view(np.uint32))
    _, (f, w0, u, v) = mp.surface_sample_numpy(verts, faces, nrm, rgb, cdf, S, seed=9, _draws=True)
    t = ((w0 * m["uv"][f, 0]) + (u * m["uv"][f, 1])) + (v * m["uv"][f, 2])
    assert t.dtype == np.float32
    want = texture.fetch_numpy(pyr, 8, 16, 0, t[:, 0].astype(np.float64), t[:, 1].astype(np.float64))
    assert np.array_equal(tex[:, 3:6], want.astype(np.float32)) and len(np.unique(tex[:, 3])) > 20
    # W0 = 0: no texture, the vertex colours
    assert np.array_equal(mp.surface_sample_tex_numpy(verts, faces, nrm, rgb, cdf, m["uv"], pyr, (0, 0, 0, 0), S, seed=9), plain)


def test_build_model_points_colours_a_textured_mesh_without_a_warning(monkeypatch):
    monkeypatch.setattr(mp, "_impl", mp._NumpyOps)
    m = render.demo_mesh(level=1, seed=5, textured=True, tex_size=8)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        table = mp.build_model_points(m, 64, candidates=512)
    assert table.shape == (64, 9) and len(np.unique(table[:, 3:6], axis=0)) > 16
    with pytest.raises(ValueError, match="vertices"):
        mp.build_model_points(m, 8, source="vertices")
    with pytest.warns(UserWarning, match="no vertex colours"):            # without the texture the mesh is what it was: grey, said aloud
        grey = mp.build_model_points({k: m[k] for k in ("verts", "faces", "normals")}, 64, candidates=512)
    assert (grey[:, 3:6] == 128).all() and np.array_equal(grey[:, :3], table[:, :3])


# ---- refusals, before any HIP call -------------------------------------------------------------------------------------------------
def test_new_entries_refuse_on_the_host():
    from geometric_aware_dense_matching_amd import _lib
    L = _lib.lib()
    assert L.gdm_texture_pyramid_texels(130, 67, 8) == texture.pyramid_texels(130, 67)
    assert L.gdm_texture_pyramid_texels(3, 5, 2) == 17 and L.gdm_texture_pyramid_texels(16384, 16384, 15) == texture.pyramid_texels(16384, 16384)
    for bad in ((0, 4, 1), (4, 0, 1), (16385, 4, 1), (4, 4, 0), (4, 4, 4), (1, 1, 2)):
        assert L.gdm_texture_pyramid_texels(*bad) == 0
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    err = lambda: L.gdm_last_error().decode()
    assert L.gdm_texture_mips_hip(p, 4, 4, 4, p, 100, None) != 0 and "L=4" in err()
    assert L.gdm_texture_mips_hip(p, 4, 4, 3, p, 20, None) != 0 and "21 needed" in err()
    assert L.gdm_texture_mips_hip(p, 4, 4, 3, p + 2, 21, None) != 0 and "aligned" in err()
    assert L.gdm_texture_mips_hip(p, 4, 4, 3, p, 1 << 31, None) != 0 and "2^31" in err()
    sample = lambda tex, row, texels, flip=1: L.gdm_surface_sample_tex_hip(p, p, p, p, p, p, tex, *row, texels, flip, 4, 2, 16, 0, p, None)
    assert sample(p + 1, (0, 4, 4, 3), 21) != 0 and "aligned" in err()
    assert sample(p, (0, 4, 4, 3), 1 << 31) != 0 and "2^31" in err()
    assert sample(p, (0, 4, 4, 3), 21, flip=2) != 0 and "flip_v" in err()
    for row in ((-1, 4, 4, 3), (1, 4, 4, 3), (0, 4, 4, 4), (0, 16385, 4, 3), (0, 4, -4, 1), (0, 4, 4, 0)):
        assert sample(p, row, 21) != 0 and "does not lie inside" in err(), row
    one = (ctypes.c_int32 * 2)(0, 1)
    frames = lambda tex, tab, texels, flip=1: L.gdm_render_frames_tex_hip(p, 0, p, p, p, one, p, p, p, 0, p, 0.5, 0.01, 1, 1, 1, 4, 1, 4, 4, p,
                                                                        4096, p, p, p, p, p, p, tex, tab, texels, flip, None)
    assert frames(p + 2, p, 21) != 0 and "tex must be 4-byte aligned" in err()
    assert frames(p, p + 4, 21) != 0 and "tex_tab" in err()
    assert frames(p, p, 0) != 0 and "tex_texels" in err()
    assert frames(p, p, 1 << 31) != 0 and "2^31" in err()
    assert frames(p, p, 21, flip=-1) != 0 and "flip_v" in err()
    assert frames(None, p, 21) != 0 and "NULL" in err()
    with pytest.raises(ValueError, match="needs uv"):
        render.SceneMeshes([tc.tetrahedron() + (None, None, None, tc.image(4, 4, 1))], device=None)
    with pytest.raises(ValueError, match="uv must be"):
        render.SceneMeshes([tc.tetrahedron() + (None, None, np.zeros((7, 2), np.float32), tc.image(4, 4, 1))], device=None)
