"""GPU: the frame renderer (gdm_render_frames_hip, render.py) against its host restatement on the fixture scenes of
tests/render_cases.py, its ties, reproducibility, hipGraph capture and guard bands; the chain from rendered frames through the front
end and the device targets to a pose fit; two training iterations of `train_lm -data rendered`.  (This file sorts before
tests/test_gpu_guard_bands.py, whose coverage test wants every entry to have run under guards by then.)"""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import guard_bands as gb
import render_cases as rc
from render_cases import bi
from geometric_aware_dense_matching_amd import model_prep, ops, pose, render

pytestmark = pytest.mark.gpu
H, W = rc.H, rc.W
EXACT = ("inst", "face", "rgb", "px_all", "px_vis", "bbox_vis", "visib_fract")


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ulp(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _check(got, want, what):
    """inst, face, rgb and the statistics equal; depth within 1 ulp (the bound check_image of test_gpu_bop_errors.py uses)."""
    got = _host(got)
    for k in EXACT:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), "%s: %s differs at %d places" % (what, k, (got[k] != want[k]).sum())
    assert got["depth"].dtype == np.float32 and np.array_equal(got["depth"] > 0, want["depth"] > 0)
    m = want["depth"] > 0
    worst = int(_ulp(got["depth"][m], want["depth"][m]).max()) if m.any() else 0
    print("%s: %d covered pixels, largest depth difference %d ulp" % (what, m.sum(), worst))
    assert worst <= 1 and not got["depth"][~m].any()
    return got


def _same(a, b):
    return all(torch.equal(a[k].contiguous().view(-1).view(torch.uint8), b[k].contiguous().view(-1).view(torch.uint8)) for k in a)


@pytest.fixture(scope="module")
def wanted():
    """The restatement's frames of every fixture scene, for f64 and f32 vertices, computed once."""
    out = {}
    for name, make in rc.SCENES.items():
        case = make()
        args, kw = rc.render_args(case)
        for dtype in (np.float64, np.float32):
            want = render.render_frames_numpy(render.SceneMeshes(case["meshes"], device=None, verts_dtype=dtype), *args, **kw)
            assert not want["ambiguous"].any()
            out[name, dtype] = want
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_kernel_equals_the_restatement_and_is_reproducible(wanted, dtype):
    case = rc.two_objects()
    args, kw = rc.render_args(case)
    scene = render.SceneMeshes(case["meshes"], verts_dtype=dtype)
    assert scene.verts.dtype == (torch.float32 if dtype == np.float32 else torch.float64)
    got = render.render_frames(scene, *args, **kw)
    host = _check(got, wanted["two objects", dtype], "two objects, %s vertices" % np.dtype(dtype).name)
    assert host["px_all"][1, 1] == 0 and host["bbox_vis"][1, 1].tolist() == [W, H, -1, -1]            # the empty slot of frame 1
    assert (host["px_vis"][:, 0] < host["px_all"][:, 0])[[0, 2]].all()                                 # occlusion happened
    assert _same(got, render.render_frames(scene, *args, **kw))                                        # bit-identical again
    # an object index outside the table, given as device data, is an empty slot
    so = torch.as_tensor(case["slot_obj"]).cuda()
    so[1, 1] = 77
    assert _same(got, render.render_frames(scene, so, *args[1:], **kw))


def test_large_triangles_take_the_cooperative_path(wanted):
    case = rc.tilted_quad()
    args, kw = rc.render_args(case)
    for dtype in (np.float64, np.float32):
        got = _check(render.render_frames(render.SceneMeshes(case["meshes"], verts_dtype=dtype), *args, **kw), wanted["tilted quad", dtype],
                     "tilted quad, %s" % np.dtype(dtype).name)
    assert got["px_vis"][0, 0] > 500 and len(np.unique(got["depth"])) > 100      # two triangles, each far above the per-thread limit
    # the quad in two slots: the wave draws large triangles of both, so slot and face travel with the source lane
    case = rc.tilted_quad_twice()
    args, kw = rc.render_args(case)
    for dtype in (np.float64, np.float32):
        got = _check(render.render_frames(render.SceneMeshes(case["meshes"], verts_dtype=dtype), *args, **kw),
                     wanted["tilted quad twice", dtype], "tilted quad twice, %s" % np.dtype(dtype).name)
        assert got["px_all"][0].tolist() == [744, 748] and got["px_vis"][0].tolist() == [744, 8]


def test_equal_depths_go_to_the_lower_face_id():
    verts = np.array([[-0.1, -0.08, 0.4], [0.12, -0.05, 0.45], [0.0, 0.1, 0.35]])
    faces = np.array([[0, 1, 2], [0, 1, 2]], dtype=np.int32)
    for order in (faces, faces[:, [1, 0, 2]]):                             # both windings; the two copies name the vertices in one order
        scene = render.SceneMeshes([(verts, order, rc.colours(3, 5), None)])
        out = _host(render.render_frames(scene, [[0]], bi.identity_pose()[:, None], bi.K, H, W, near=bi.NEAR))
        assert (out["inst"] == 1).sum() > 300 and (out["face"][out["inst"] == 1] == 0).all() and (out["face"][out["inst"] == 0] == -1).all()


def test_equal_depths_go_to_the_lower_slot():
    case = rc.two_objects()
    scene = render.SceneMeshes(case["meshes"][:1])
    RT = np.repeat(case["RT"][:, :1], 2, axis=1)
    out = _host(render.render_frames(scene, np.zeros((3, 2), dtype=np.int32), RT, case["K"], H, W, near=bi.NEAR))
    assert set(np.unique(out["inst"]).tolist()) == {0, 1}
    assert (out["px_vis"][:, 1] == 0).all() and np.array_equal(out["px_all"][:, 1], out["px_all"][:, 0]) and (out["px_all"][:, 0] > 100).all()
    assert np.array_equal(out["px_vis"][:, 0], out["px_all"][:, 0]) and (out["bbox_vis"][:, 1] == [W, H, -1, -1]).all()


def test_refusals():
    case = rc.two_objects()
    args, kw = rc.render_args(case)
    scene = render.SceneMeshes(case["meshes"])
    with pytest.raises(ValueError, match="S=9"):
        render.render_frames(scene, np.zeros((1, 9), dtype=np.int32), np.zeros((1, 9, 3, 4)), bi.K, H, W)
    with pytest.raises(ValueError, match="slot_obj"):
        render.render_frames(scene, np.full((3, 3), 3), *args[1:], **kw)
    dev = [scene.verts, scene.vcol, scene.vnrm, scene.faces]
    rest = [torch.as_tensor(a).cuda() for a in (case["slot_obj"], case["RT"], case["K"], case["light"])]
    with pytest.raises(ops._lib.GdmError, match="not ascending"):
        ops.render_frames(*dev, [0, 400, 320, 642], *rest, H, W, 0.3, bi.NEAR)
    with pytest.raises(ops._lib.GdmError, match="exceeds Ft"):
        ops.render_frames(*dev, [0, 320, 640, 643], *rest, H, W, 0.3, bi.NEAR)
    with pytest.raises(ops._lib.GdmError, match="ambient"):
        ops.render_frames(*dev, scene.obj_face0, *rest, H, W, 1.5, bi.NEAR)
    assert ops.call("gdm_render_frames_workspace_bytes", 3, 3, H, W) == 3 * 3 * H * W * 8
    assert ops.call("gdm_render_frames_workspace_bytes", 3, 9, H, W) == 0
    torch.cuda.synchronize()


def test_graph_capture_and_replay_with_new_poses():
    case = rc.two_objects()
    scene = render.SceneMeshes(case["meshes"])
    so, K, light = (torch.as_tensor(case[k]).cuda() for k in ("slot_obj", "K", "light"))
    so = so.to(torch.int32)
    static_RT = torch.as_tensor(case["RT"]).cuda()

    def frames():
        return render.render_frames(scene, so, static_RT, K, H, W, light=light, ambient=rc.AMBIENT, near=rc.NEAR)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = {k: v.clone() for k, v in frames().items()}
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = frames()
    graph.replay()
    assert _same(first, out)
    moved = case["RT"].copy()
    moved[:, 0, 0, 3] -= 0.02                                              # object 0 two centimetres to the left, object 1 turned
    moved[:, 1, :, :3] = moved[:, 1, :, :3] @ bi.rot(0.4, (0, 0, 1))
    static_RT.copy_(torch.as_tensor(moved).cuda())
    graph.replay()
    replayed = {k: v.clone() for k, v in out.items()}
    eager = frames()
    assert _same(eager, replayed) and not _same(first, replayed)


def test_the_entry_stays_inside_its_tensors(wanted, monkeypatch):
    case = rc.two_objects()
    args, kw = rc.render_args(case)
    scene = render.SceneMeshes(case["meshes"])
    with gb.filled_empties(), gb.guarded_calls(monkeypatch) as st:
        got = render.render_frames(scene, *args, **kw)
    assert st.counts["gdm_render_frames_hip"] == 1
    # the bands and the const inputs were checked by the wrapper; equality with the restatement in every element of every output
    # says that none of them kept the allocator's fill
    _check(got, wanted["two objects", np.float32], "guarded")


# ---- the chain: rendered frames -> front end -> device targets -> pose fit -------------------------------------------------------
def test_rendered_frames_through_the_front_end_and_the_targets_to_a_pose():
    """ADD(fit, true RT) < dist_thresh = 0.01 m for every valid item.  The bound is derived: every accepted correspondence lies within
    dist_thresh of its vertex under the true pose, so the true pose's RMS residual is at most that and the least-squares fit's is
    no larger; 0.01 m is also 0.1 d of the demo object."""
    from geometric_aware_dense_matching_amd import train_lm
    mesh = render.demo_mesh(level=3)
    M, n, S_crop, N = 1024, 4, 64, 512
    Hc, Wc = 120, 160
    K = np.array([[143.1, 0.0, 81.3], [0.0, 143.4, 60.5], [0.0, 0.0, 1.0]])
    model_xyz = torch.from_numpy(np.ascontiguousarray(model_prep.build_model_points(mesh, M)[:, :3])).cuda()
    other = render.demo_mesh(level=2, seed=9)
    scene = render.SceneMeshes([render._as_mesh(mesh), render._as_mesh(other), render._as_mesh(render.backdrop_mesh(K, Hc, Wc, z=1.5))])
    frames = render.RenderedFrames(scene, 0, model_xyz, n, N, S_crop=S_crop, seed=3, n_batches=2, K=K, H=Hc, W=Wc, S=4,
                                   z_range=(0.3, 0.6), backdrop_obj=2, build_pyramid=False)          # 512 points: below the pyramid's 1024
    assert len(frames) == 2
    _, RT_true, fr = frames.frames(0)
    assert (fr["depth"] > 0).all() and (fr["px_vis"][:, 0] > 64).all()      # the backdrop fills the frame; the target shows
    assert bool((fr["visib_fract"][:, 0] <= 1).all()) and bool((fr["px_all"][:, 0] >= fr["px_vis"][:, 0]).all())
    batches = list(frames)
    assert len(batches) == 2 and not torch.equal(batches[0]["RT"], batches[1]["RT"])
    worst = 0.0
    for item in batches:
        assert item["cld_rgb_nrm"].shape == (n, 9, N) and item["RT"].shape == (n, 3, 4) and item["origin_labels"].shape == (n, N)
        counter = torch.zeros(2, dtype=torch.int64, device="cuda")
        cu = train_lm.device_targets(SimpleNamespace(model_emb=SimpleNamespace(xyz=model_xyz)), dict(item), counter)
        match = cu["match_idx"]
        res = dict(mask=(match < M).to(torch.uint8), best_idx=match.clamp(max=M - 1).to(torch.int32).contiguous())
        RT, valid = pose.solve_poses(res, cu["cld_rgb_nrm"], model_xyz)
        add = pose.add_metric(RT, cu["RT"], model_xyz)
        pairs = res["mask"].sum(dim=1)
        print("matched points per item %s, ADD of the fit (m) %s, items replaced / unreplaced %s" %
              (pairs.tolist(), ["%.5f" % a for a in add.tolist()], counter.tolist()))
        assert int(counter[1]) == 0 and bool(valid.any())
        assert bool((add[valid] < 0.01).all())
        assert int(pairs[valid].min()) >= 20
        worst = max(worst, float(add[valid].max()))
    print("largest ADD of a fit on ground-truth correspondences: %.5f m" % worst)


def test_train_lm_on_rendered_frames(tmp_path, capsys):
    from geometric_aware_dense_matching_amd import train_lm
    common = "-data rendered -cls_id=1 --batch-size 2 --n-points 1024 --n-mesh 256 --synthetic-items 4"
    argv = ("-state=train --deterministic --epochs 1 --save-every 1 --log-every 1 --log-dir %s %s" % (tmp_path, common)).split()
    assert train_lm.build_parser().parse_args(argv).gt_targets == "loader"          # -data rendered switches it to "device" itself
    train_lm.main(argv)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("avg_loss")]
    assert len(lines) == 2
    for ln in lines:
        m = re.match(r"avg_loss:(\S+) seg: (\S+) match: (\S+)  invalid items replaced: (\d+) unreplaced: (\d+)", ln)
        assert m, ln
        assert all(np.isfinite(float(v)) for v in m.groups()[:3]) and int(m.group(5)) == 0
    # -state=test on held-out rendered frames (another seed) with the checkpoint the epoch left, through the existing evaluator
    res = train_lm.test(train_lm.build_parser().parse_args(("-state=test -checkpoint %s %s" % (tmp_path, common)).split()))
    assert len(res) == 2 and all(r["RT"].shape == (2, 3, 4) and r["cls_id"] == [1, 1] for r in res)
    (name, rec), = train_lm.test.last_table.recalls.items()
    assert len(rec["ad_10"]) == 4 and np.isfinite(train_lm.test.last_table.errors[name]["ad"]).all()
    with pytest.raises(SystemExit):
        train_lm.build_parser().parse_args(["-data", "frames"])
