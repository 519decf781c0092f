"""GPU: the depth sensor kernel (gdm_depth_sensor_hip, sensor.simulate_depth_sensor) against the restatement
sensor.simulate_depth_sensor_numpy, bit for bit and under guard bands: every stage alone and together, both baseline signs, K per
frame, the widest and the narrowest shadow window, every case of tests/sensor_cases.py; hipGraph capture with a device seed; the
refusals; RenderedFrames(depth_sensor=...) and the sensed batch through the YCB-V fill and pose verification.  (This file sorts
before tests/test_gpu_guard_bands.py, whose coverage test wants every entry to have run under guards by then.)"""
import numpy as np
import pytest
import torch

import guard_bands as gb
import sensor_cases as sc
from geometric_aware_dense_matching_amd import _lib, frontend, model_prep, ops, pose, render, sensor
from geometric_aware_dense_matching_amd.sensor import DepthSensor

pytestmark = pytest.mark.gpu
TW, TH = sensor.tile_shape()
# the smallest frame in which a tile has neighbours on both sides, the last tile of a row and of a column is partial and a shadow
# window reaches into the next tile; one narrower than a tile and than the window; one pixel
H0, W0 = TH + 3, 2 * TW + 5
STAGE_SETS = [("range",), ("shadow",), ("grazing",), ("jitter",), ("noise",), "all"]


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _K2(H, W):
    """Two cameras, one per frame: other focal lengths, the second with an off-centre principal point."""
    return np.stack([sc.make_K(300.0, 310.0, H=H, W=W), sc.make_K(261.5, 255.0, 0.37 * W, 0.61 * H)])


def _check(monkeypatch, depth, K, s, seed, what):
    want = sensor.simulate_depth_sensor_numpy(depth, K, s, seed=seed)
    with gb.guarded_calls(monkeypatch) as calls:
        got = sensor.simulate_depth_sensor(torch.from_numpy(depth).cuda(), K, s, seed=seed)
    assert calls.counts["gdm_depth_sensor_hip"] == 1
    gd, gc = got["depth"].cpu().numpy(), got["cause"].cpu().numpy()
    assert gd.dtype == np.float32 and gc.dtype == np.uint8 and gd.shape == depth.shape and gc.shape == depth.shape
    hist = np.bincount(want["cause"].ravel(), minlength=6).tolist()
    nd, nc = int((_bits(gd).reshape(-1, 4) != _bits(want["depth"]).reshape(-1, 4)).any(1).sum()), int((gc != want["cause"]).sum())
    print("%s: causes %s, %d depth words and %d causes differ" % (what, hist, nd, nc))
    assert nc == 0 and nd == 0, what
    return want, hist


@pytest.mark.parametrize("baseline", [0.075, -0.075], ids=["right", "left"])
@pytest.mark.parametrize("stages", STAGE_SETS, ids=[s if isinstance(s, str) else s[0] for s in STAGE_SETS])
def test_each_stage_and_all_equal_the_restatement(monkeypatch, stages, baseline):
    depth = sc.mixed(H0, W0, 3)
    depth[:, :, TW - 20:TW + 30] = sc.shadow_across_tiles(H0, W0, TW, TH)[:, :, TW - 20:TW + 30]
    _, hist = _check(monkeypatch, depth, _K2(H0, W0), DepthSensor(baseline=baseline, stages=stages), 7, "%s %+g" % (stages, baseline))
    if stages == "all":
        assert all(h > 0 for h in hist)                                    # every cause occurs
    elif stages != ("noise",):
        assert hist[sensor.STAGES[stages[0]].bit_length() + 1] > 0         # range -> 2, shadow -> 3, grazing -> 4, jitter -> 5


@pytest.mark.parametrize("baseline", [0.075, -0.075], ids=["right", "left"])
@pytest.mark.parametrize("fx,wd", [(1357.0, 255), (5.0, 1)])
def test_the_widest_and_the_narrowest_window(monkeypatch, fx, wd, baseline):
    K = sc.make_K(fx, H=H0, W=W0)
    s = DepthSensor(baseline=baseline)
    assert sensor.frame_constants(K, s)[5] == wd
    depth = sc.shadow_across_tiles(H0, W0, TW, TH)
    depth[:, :, :40] = sc.shadow_leaves_frame(H0, W0)[:, :, :40]
    depth[1] = np.where(depth[1] == sc.FRONT, np.float32(0.41), depth[1])  # frame 1: a disparity of just under the window
    _, hist = _check(monkeypatch, depth, K, s, 21, "Wd=%d %+g" % (wd, baseline))
    assert wd == 1 or hist[3] > 200


@pytest.fixture(scope="module")
def cases():
    return sc.all_cases(H0, W0, sc.make_K(300.0, H=H0, W=W0), TW, TH)


@pytest.mark.parametrize("baseline", [0.075, -0.075], ids=["right", "left"])
@pytest.mark.parametrize("name", ["box", "tilted-30", "tilted-80", "tilted-89.5", "invalid", "shadow-across-tiles", "shadow-leaves-frame",
                                  "mixed"])
def test_every_case_under_guard_bands(monkeypatch, cases, name, baseline):
    assert sorted(cases) == sorted(sc.all_cases(2, 2, sc.make_K(1.0), 1, 1))          # the parametrisation above names them all
    _check(monkeypatch, cases[name], sc.make_K(300.0, H=H0, W=W0), DepthSensor(baseline=baseline), 5, name)


@pytest.mark.parametrize("n,H,W", [(2, 5, 17), (1, 1, 1), (2, 3 * TH, TW)], ids=["17x5", "1x1", "tile-aligned"])
def test_small_and_aligned_frames(monkeypatch, n, H, W):
    depth = sc.mixed(H, W, 9)[:n]
    for baseline in (0.075, -0.075):
        _check(monkeypatch, depth, _K2(H, W)[:n], DepthSensor(baseline=baseline), 2, "%dx%d %+g" % (W, H, baseline))
    if (H, W) == (1, 1):                                                   # one valid pixel, nothing to difference against: grazing
        depth[:] = 1.0
        want, _ = _check(monkeypatch, depth, sc.make_K(300.0), DepthSensor(stages=("range", "shadow", "grazing", "noise")), 2, "1x1 valid")
        assert want["cause"].tolist() == [[[4]]]


def test_graph_capture_redraws_from_the_device_seed():
    depth = sc.mixed(H0, W0, 3)
    K, s = sc.make_K(300.0, H=H0, W=W0), DepthSensor()
    dev = torch.from_numpy(depth).cuda()
    word = torch.tensor([41], dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = {k: v.clone() for k, v in sensor.simulate_depth_sensor(dev, K, s, seed=word).items()}
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sensor.simulate_depth_sensor(dev, K, s, seed=word)
    for seed in (41, 977):
        word.fill_(seed)
        out["depth"].fill_(float("nan"))
        out["cause"].fill_(99)
        graph.replay()
        torch.cuda.synchronize()
        want = sensor.simulate_depth_sensor_numpy(depth, K, s, seed=seed)
        assert np.array_equal(_bits(out["depth"].cpu().numpy()), _bits(want["depth"])) and np.array_equal(out["cause"].cpu().numpy(), want["cause"])
        if seed == 41:
            assert all(gb.same_bits(eager[k], out[k]) for k in eager)
    plain = sensor.simulate_depth_sensor(dev, K, s, seed=977)              # and an int seed draws what the word drew
    assert all(gb.same_bits(plain[k], out[k]) for k in plain)


def test_refusals_come_before_any_launch(monkeypatch):
    depth = torch.ones(2, 6, 9, device="cuda")
    K = torch.from_numpy(sc.make_K(300.0, H=6, W=9))
    good = DepthSensor()

    def refused(match, s=good, K=K, **kw):
        with gb.guarded_calls(monkeypatch) as calls:                       # a refused call has touched nothing, interior included
            with pytest.raises(_lib.GdmError, match=match):
                ops.depth_sensor(depth, K, *s.scalars(), s.stages, **kw)
        assert "gdm_depth_sensor_hip" in calls.refused and not calls.counts

    s = DepthSensor()
    for field, value, match in (("z_min", 0.0, "z_min"), ("z_min", -1.0, "z_min"), ("z_max", 0.4, "z_max"), ("subpixel", 0.99, "subpixel"),
                                ("cos_soft", 0.05, "cos_min"), ("p_shift", 1.01, "p_shift"), ("p_shift", -0.01, "p_shift"),
                                ("cos_soft", 1.5, "cos_soft"), ("sigma_d", -0.1, "sigma_d"), ("baseline", 0.0, "baseline"),
                                ("z_min", 0.05, "shadow window")):
        setattr(s, field, value)
        refused(match, s)
        s = DepthSensor()
    refused("shadow window", K=torch.from_numpy(sc.make_K(1400.0)))       # ceil(105 / 0.4) = 263 > 255
    refused("fx", K=torch.zeros(3, 3))
    s.stages = 32
    refused("stages", s)
    out_d, out_c = torch.empty_like(depth), torch.empty(2, 6, 9, dtype=torch.uint8, device="cuda")
    refused("alias", out=(depth, out_c))
    refused("alias", out=(out_d, depth.view(torch.uint8).view(-1)[4:4 + 108].view(2, 6, 9)))
    refused("alias", out=(out_d, out_d.view(torch.uint8).view(-1)[-108:].view(2, 6, 9)))
    many = torch.ones(sensor.MAX_K + 1, 2, 2, device="cuda")
    with pytest.raises(_lib.GdmError, match="at most"):
        ops.depth_sensor(many, torch.from_numpy(np.stack([sc.make_K(300.0 + i) for i in range(sensor.MAX_K + 1)])), *good.scalars(), 31)
    assert sensor.simulate_depth_sensor(many, np.stack([sc.make_K(300.0)] * (sensor.MAX_K + 1)))["cause"].shape == many.shape   # one camera: any n
    with pytest.raises(TypeError):
        ops.depth_sensor(depth, K.cuda(), *good.scalars(), 31)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_sensor(depth.cpu(), K, *good.scalars(), 31)
    ops.depth_sensor(depth, K, *good.scalars(), 31)                        # and the same call with nothing wrong runs


# ---- batches --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rendered():
    mesh = render.demo_mesh(level=3)
    B, N, Hc, Wc = 2, 1024, 120, 160
    K = np.array([[143.1, 0.0, 81.3], [0.0, 143.4, 60.5], [0.0, 0.0, 1.0]])
    model_xyz = torch.from_numpy(np.ascontiguousarray(model_prep.build_model_points(mesh, 1024)[:, :3])).cuda()
    scene = render.SceneMeshes([render._as_mesh(mesh), render._as_mesh(render.demo_mesh(level=2, seed=9)),
                                render._as_mesh(render.backdrop_mesh(K, Hc, Wc, z=1.5))])
    kw = dict(S_crop=64, seed=3, n_batches=1, K=K, H=Hc, W=Wc, S=4, z_range=(0.45, 0.8), backdrop_obj=2, build_pyramid=False, train=False)
    return dict(mesh=mesh, scene=scene, model_xyz=model_xyz, K=K, B=B, N=N, H=Hc, W=Wc, kw=kw)


def test_rendered_batches_carry_the_sensed_frame(rendered):
    r = rendered
    args = (r["scene"], 0, r["model_xyz"], r["B"], r["N"])
    frames = render.RenderedFrames(*args, keep_frames=True, depth_sensor=DepthSensor(), **r["kw"])
    item = frames.batch_at(0)
    clean = render.RenderedFrames(*args, keep_frames=True, **r["kw"]).batch_at(0)
    none = render.RenderedFrames(*args, keep_frames=True, depth_sensor=None, **r["kw"]).batch_at(0)
    assert set(none) == set(clean) and all(gb.same_bits(clean[k], none[k]) for k in clean if torch.is_tensor(clean[k]))
    assert set(item) - set(clean) == {"frame_depth_clean", "depth_cause"}
    assert gb.same_bits(item["frame_depth_clean"], clean["frame_depth"])
    again = sensor.simulate_depth_sensor(item["frame_depth_clean"], r["K"], DepthSensor(), seed=frames.sensor_seed(0))
    assert gb.same_bits(item["frame_depth"], again["depth"]) and gb.same_bits(item["depth_cause"], again["cause"])
    hist = torch.bincount(item["depth_cause"].flatten().long(), minlength=6).tolist()
    print("causes of the sensed batch: %s" % hist)
    assert hist[0] > 0.5 * sum(hist) and hist[3] > 0 and hist[4] > 0
    assert not gb.same_bits(item["cld_rgb_nrm"], clean["cld_rgb_nrm"]) and not gb.same_bits(item["frame_depth"], clean["frame_depth"])
    for k in ("RT", "K", "bbox", "px_vis", "visib_fract", "rgb", "center", "scale"):          # the renderer's, and the crop's colour
        assert gb.same_bits(item[k], clean[k]), k
    assert frames.sensor_seed(0) != frames.sensor_seed(1) and frames.sensor_seed(0) != frames.item_seed(0)


def test_a_sensed_frame_goes_through_the_fill_and_the_verification(rendered):
    r = rendered
    frames = render.RenderedFrames(r["scene"], 0, r["model_xyz"], r["B"], r["N"], keep_frames=True, depth_sensor=DepthSensor(), **r["kw"])
    _, RT, fr = frames.frames(0)
    item = frames.batch_at(0)
    mask = (fr["inst"] == 1).to(torch.uint8) * 255
    K32 = torch.from_numpy(r["K"].astype(np.float32)).cuda().expand(r["B"], 3, 3).contiguous()
    filled = frontend.make_inputs_from_boxes(fr["rgb"], item["frame_depth"], K32, item["bbox"], 64, r["N"], mask=mask, depth_fill="fast",
                                             sampler="hash", seed=4, build_pyramid=False)
    assert all(bool(torch.isfinite(filled[k]).all()) for k in ("cld_rgb_nrm", "depth_filled", "rgb"))
    crop_holes = int((filled["depth_filled"] > 1e-6).sum()) - int((filled["dpt_xyz"][..., 2] > 1e-6).sum())
    print("the fill closed %d crop pixels the sensor had dropped" % crop_holes)
    assert crop_holes > 0
    nv = len(r["mesh"]["verts"])
    got = pose.verify_poses(r["scene"].verts[:nv], r["scene"].faces[:len(r["mesh"]["faces"])],
                            torch.from_numpy(RT[:, :1].copy()).cuda(), item["frame_depth"], torch.from_numpy(r["K"]).cuda(),
                            window=pose.boxes_to_windows(item["bbox"], r["H"], r["W"]), delta=0.01)
    print("verification of the true pose against the sensed frame: score %s, counts %s" % (got["score"].tolist(), got["counts"].tolist()))
    assert bool(torch.isfinite(got["score"]).all()) and bool((got["counts"] >= 0).all()) and all(b in (-1, 0) for b in got["best"].tolist())
