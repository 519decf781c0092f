"""GPU: textured meshes -- gdm_texture_mips_hip, gdm_render_frames_tex_hip and gdm_surface_sample_tex_hip against
their numpy restatements (texture.py, render.render_frames_numpy, model_prep.surface_sample_tex_numpy), bit for bit; the table rows
a kernel must not trust; hipGraph capture; the model table of a textured mesh.  (This file sorts before
tests/test_gpu_guard_bands.py, whose coverage test wants every entry to have run under guards by then.)"""
import warnings

import numpy as np
import pytest
import torch

import guard_bands as gb
import texture_cases as tc
from geometric_aware_dense_matching_amd import model_prep as mp
from geometric_aware_dense_matching_amd import ops, render, texture

pytestmark = pytest.mark.gpu
OUTPUTS = ("rgb", "depth", "inst", "face", "px_all", "px_vis", "bbox_vis", "visib_fract")


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(a, b):
    return all(torch.equal(a[k].contiguous().view(-1).view(torch.uint8), b[k].contiguous().view(-1).view(torch.uint8)) for k in a)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- mips -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 5), (7, 1), (64, 64), (130, 67)])
def test_mips_kernel_equals_the_restatement_bit_for_bit(monkeypatch, h, w):
    img = tc.image(h, w, 100 + h)
    want = texture.build_mips_numpy(img)
    with gb.guarded_calls(monkeypatch) as calls:
        got = texture.build_mips(_t(img))
    assert calls.counts["gdm_texture_mips_hip"] == 1
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want)
    if texture.full_levels(h, w) > 1:                                      # fewer levels: a prefix of the same pyramid
        part = texture.build_mips(_t(img), L=texture.full_levels(h, w) - 1).cpu().numpy()
        assert np.array_equal(part, want[:len(part)]) and len(part) == texture.pyramid_texels(h, w, texture.full_levels(h, w) - 1)
    with pytest.raises(ValueError):
        texture.build_mips(_t(img), L=texture.full_levels(h, w) + 1)


# ---- the textured frames ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wanted():
    """The restatement's frames, computed once per (sizes, vertex type, K per instance)."""
    cache = {}

    def get(sizes, dtype, kpi):
        key = (sizes, np.dtype(dtype).name, kpi)
        if key not in cache:
            case = tc.textured_scene(*sizes, k_per_instance=kpi)
            args, kw = tc.render_args(case)
            want = render.render_frames_numpy(render.SceneMeshes(case["meshes"], device=None, verts_dtype=dtype), *args, **kw)
            assert not want["ambiguous"].any()
            cache[key] = (case, want)
        return cache[key]
    return get


@pytest.mark.parametrize("kpi", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("sizes", tc.SIZES, ids=["48x64-tex16x16", "37x53-tex33x20"])
def test_textured_frames_equal_the_restatement_bit_for_bit(wanted, monkeypatch, sizes, dtype, kpi):
    case, want = wanted(sizes, dtype, kpi)
    args, kw = tc.render_args(case)
    scene = render.SceneMeshes(case["meshes"], verts_dtype=dtype)
    assert scene.has_texture and np.array_equal(scene.tex.cpu().numpy(), scene.tex_np)
    with gb.guarded_calls(monkeypatch) as calls:
        got = render.render_frames(scene, *args, **kw)
    assert calls.counts["gdm_render_frames_tex_hip"] == 1 and "gdm_render_frames_hip" not in calls.counts
    host = _host(got)
    lv = want["tex_level"]
    print("%s %s kpi=%d: %d textured pixels, levels %s" % (sizes, np.dtype(dtype).name, kpi, (lv >= 0).sum(),
                                                           dict(zip(*np.unique(lv[lv >= 0], return_counts=True)))))
    for k in OUTPUTS:
        assert host[k].dtype == want[k].dtype and host[k].shape == want[k].shape, k
        print("  %s: %d values differ" % (k, (host[k] != want[k]).sum()))
    for k in OUTPUTS:
        assert np.array_equal(_bits(host[k]), _bits(want[k])), "%s differs at %d places" % (k, (host[k] != want[k]).sum())
    assert (lv[0][lv[0] >= 0] >= 2).all() and (lv[1] == 0).any() and lv[1].max() >= 2          # far, near, grazing
    assert _same(got, render.render_frames(scene, *args, **kw))                                  # and again, plain: the same bytes


def _entry_args(scene, case):
    """The textured scene as the arguments of ops.render_frames up to `textures`."""
    (slot_obj, RT, K, H, W), kw = tc.render_args(case)
    return (scene.verts, scene.vcol, scene.vnrm, scene.faces, scene.obj_face0, _t(slot_obj), _t(RT), _t(K), _t(case["light"]), H, W,
            kw["ambient"], kw["near"])


def test_a_table_without_textures_gives_the_untextured_entrys_bytes(monkeypatch):
    case = tc.textured_scene(*tc.SIZES[1], k_per_instance=False)
    scene = render.SceneMeshes(case["meshes"])
    head = _entry_args(scene, case)
    plain = ops.render_frames(*head)
    with gb.guarded_calls(monkeypatch) as calls:
        tex = ops.render_frames(*head, textures=(scene.fuv, scene.tex, torch.zeros_like(scene.tex_tab), True))
    assert calls.counts["gdm_render_frames_tex_hip"] == 1
    assert all(torch.equal(a, b) for a, b in zip(plain, tex))
    # and the untextured objects of a textured call are coloured as the untextured entry colours them
    mixed = ops.render_frames(*head, textures=(scene.fuv, scene.tex, scene.tex_tab, True))
    textured = mixed[2] == 1                                               # slot 0 holds object 0 in both frames ...
    textured[1] |= mixed[2][1] == 2                                        # ... and so does slot 1 of frame 1
    assert torch.equal(mixed[0][~textured], plain[0][~textured]) and not torch.equal(mixed[0][textured], plain[0][textured])
    assert all(torch.equal(a, b) for a, b in zip(plain[1:], mixed[1:]))


@pytest.mark.parametrize("row", [(-1, 20, 33, 6), (1 << 40, 20, 33, 6), (2, 20, 33, 6), (0, 20, 33, 7), (0, 20, 33, 0), (0, 16385, 33, 6),
                                 (0, 20, -33, 6), (0, 1 << 33, 1 << 33, 1 << 33)],
                         ids=["negative-offset", "offset-past-the-end", "pyramid-past-the-end", "L-too-large", "L-zero", "W0-too-large",
                              "H0-negative", "all-huge"])
def test_an_invalid_table_row_is_no_texture_and_nothing_outside_is_touched(monkeypatch, row):
    """The row of the textured object replaced by one the rule calls invalid: under guard bands (every tensor between 1 MiB of 0xFF,
    so a read outside `tex` would bring 0xFF texels in and a write would be seen) the call gives the vertex-colour image."""
    case = tc.textured_scene(*tc.SIZES[1], k_per_instance=False)
    scene = render.SceneMeshes(case["meshes"])
    assert scene.tex_tab_np[0].tolist() == [0, 20, 33, 6] and len(scene.tex_np) == texture.pyramid_texels(33, 20)
    head = _entry_args(scene, case)
    plain = ops.render_frames(*head)
    tab = scene.tex_tab.clone()
    tab[0] = torch.tensor(row, dtype=torch.int64)
    with gb.guarded_calls(monkeypatch) as calls:
        got = ops.render_frames(*head, textures=(scene.fuv, scene.tex, tab, True))
    assert calls.counts["gdm_render_frames_tex_hip"] == 1
    assert all(torch.equal(a, b) for a, b in zip(plain, got))


def test_textured_frames_capture_in_a_graph_and_replay_bit_identically():
    case = tc.textured_scene(*tc.SIZES[0], k_per_instance=True)
    args, kw = tc.render_args(case)
    scene = render.SceneMeshes(case["meshes"])
    so, RT, K = _t(args[0]), _t(args[1]), _t(args[2])
    light = _t(case["light"])

    def run():
        return render.render_frames(scene, so, RT, K, case["H"], case["W"], light=light, ambient=tc.AMBIENT, near=tc.NEAR)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = {k: v.clone() for k, v in run().items()}
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for _ in range(2):
        for v in out.values():
            v.fill_(0) if v.dtype != torch.float32 else v.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(eager, out)


# ---- the textured sampler -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 257, 4096])
def test_surface_sample_tex_equals_its_restatement(monkeypatch, S):
    m = render.demo_mesh(level=2, seed=6, textured=True, tex_size=16)
    verts, faces, nrm = m["verts"].astype(np.float32), m["faces"], m["normals"]
    rgb = np.random.RandomState(2).randint(0, 256, size=verts.shape).astype(np.float32)
    cdf = mp.face_cdf(m["verts"], faces)
    img2 = tc.image(33, 20, 12)                                            # a second pyramid in front: the row's offset is not 0
    pyr = np.concatenate([texture.build_mips_numpy(img2), texture.build_mips_numpy(m["texture"])])
    row = (texture.pyramid_texels(33, 20), 32, 16, 6)
    want = mp.surface_sample_tex_numpy(verts, faces, nrm, rgb, cdf, m["uv"], pyr, row, S, seed=21)
    dev = [_t(a) for a in (verts, faces, nrm, rgb, cdf)]
    with gb.guarded_calls(monkeypatch) as calls:
        got = ops.surface_sample_tex(*dev, _t(m["uv"]), _t(pyr), row, S, seed=21).cpu().numpy()
    assert calls.counts["gdm_surface_sample_tex_hip"] == 1
    assert np.array_equal(_bits(got), _bits(want))
    plain = ops.surface_sample(*dev, S, seed=21).cpu().numpy()
    assert np.array_equal(_bits(got[:, :3]), _bits(plain[:, :3])) and np.array_equal(_bits(got[:, 6:]), _bits(plain[:, 6:]))
    assert S == 1 or not np.array_equal(got[:, 3:6], plain[:, 3:6])
    # W0 = 0: the vertex colours; a row outside the buffer is refused (it is host data here)
    assert np.array_equal(_bits(ops.surface_sample_tex(*dev, _t(m["uv"]), _t(pyr), (0, 0, 0, 0), S, seed=21).cpu().numpy()), _bits(plain))
    from geometric_aware_dense_matching_amd import _lib
    with pytest.raises(_lib.GdmError, match="does not lie inside"):
        ops.surface_sample_tex(*dev, _t(m["uv"]), _t(pyr), (row[0] + 1, 32, 16, 6), S, seed=21)


def test_build_model_points_of_the_textured_demo_mesh():
    m = render.demo_mesh(level=3, seed=1, textured=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        table = mp.build_model_points(m, 256, candidates=4096, seed=3)
    assert table.shape == (256, 9) and table.dtype == np.float32
    assert len(np.unique(table[:, 3:6], axis=0)) > 64 and table[:, 3:6].min() >= 0 and table[:, 3:6].max() <= 255
    prev = mp._impl
    mp._impl = mp._NumpyOps
    try:
        want = mp.build_model_points(m, 256, candidates=4096, seed=3)
    finally:
        mp._impl = prev
    assert np.array_equal(_bits(table), _bits(want))
