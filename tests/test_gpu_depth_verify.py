"""GPU: pose verification against the observed depth (gdm_pose_verify_hip, pose.verify_poses) -- the fused kernel against
its host restatement and against the existing rasteriser, bit for bit; selection and the end-to-end chain from rendered frames;
reproducibility, hipGraph capture, the memory condition, guard bands, and verify=None leaving the pipeline as it was.  (This file
sorts before tests/test_gpu_guard_bands.py, whose coverage test wants every entry to have run under guards by then.)"""
import collections
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import guard_bands as gb
import verify_cases as vc
from geometric_aware_dense_matching_amd import infer, model_prep, pose, render, synthetic
from geometric_aware_dense_matching_amd.config import make_model_cfg

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _case(name):
    if name in vc.MIXED:
        return vc.mixed_case(name)
    if name == "ranking":
        return vc.ranking_case()
    return vc.edge_case(np.float32 if name == "edges f32" else np.float64)


CASES = vc.MIXED + ("edges f32", "edges f64", "ranking")


@pytest.fixture(scope="module")
def wanted():
    """The restatement's answer for every case, computed once."""
    out = {}
    for name in CASES:
        args, kw = vc.call_args(_case(name))
        out[name] = pose.verify_poses_numpy(*args, **kw)
    return out


def _device_args(case):
    """The case on the device: verts in the case's dtype, RT f64, depth f32, K f64, window i32, cand_valid bool."""
    args, kw = vc.call_args(case)
    args = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args)
    kw = {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    return args, kw


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _equal(got, want, what):
    got = _host(got)
    for k, dtype in (("counts", np.int32), ("score", np.float64), ("best", np.int32)):
        assert got[k].dtype == dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), "%s: %s differs\n%s\n%s" % (what, k, got[k], want[k])


@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_the_restatement_and_is_reproducible(wanted, name):
    case = _case(name)
    args, kw = _device_args(case)
    assert args[0].dtype == (torch.float32 if case["verts"].dtype == np.float32 else torch.float64)
    got = pose.verify_poses(*args, **kw)
    _equal(got, wanted[name], name)
    again = pose.verify_poses(*args, **kw)
    assert all(gb.same_bits(got[k], again[k]) for k in got)
    if name.startswith("edges"):
        assert got["counts"][0, 0].tolist() == vc.edge_expected(case).tolist()
    if name == "n3 C5 f32 K,depth per instance":
        assert int(got["counts"][1, :, 0].min()) > 4096                   # the large triangle fills more than one tile


@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_the_existing_rasteriser(name):
    """The same counts from evaluation.render_depth(keep_inf=True) into an [n C, H, W] buffer plus torch comparisons: the LDS path and
    the raster_kernel path agree with zero tolerance."""
    args, kw = _device_args(_case(name))
    got = pose.verify_poses(*args, **kw)["counts"]
    composed = pose.verify_counts_composed(*args, window=kw["window"], delta=kw["delta"], near=kw["near"])
    assert composed.dtype == torch.int32 and torch.equal(got, composed), "%s\n%s\n%s" % (name, got.cpu(), composed.cpu())


def test_selection_ranks_true_over_shifted_over_flipped():
    case = vc.ranking_case()
    RT = torch.from_numpy(case["RT"].astype(np.float32)).cuda()
    valid = torch.ones(2, dtype=torch.bool, device="cuda")
    cands = collections.OrderedDict((name, (RT[:, c].contiguous(), valid)) for c, name in enumerate(vc.RANK_NAMES))
    verify = dict(verts=torch.from_numpy(case["verts"]).cuda(), faces=torch.from_numpy(case["faces"]).cuda(),
                  depth=torch.from_numpy(case["depth"]).cuda(), K=torch.from_numpy(case["K"]).cuda(), delta=case["delta"], near=case["near"])
    sel = pose.select_verified(cands, verify)
    s = sel["scores"].cpu().numpy()
    print("scores (true, shifted, flipped): unoccluded %s, occluded %s" % (s[0].tolist(), s[1].tolist()))
    assert sel["names"] == vc.RANK_NAMES and sel["which"].dtype == torch.int32 and sel["which"].tolist() == [0, 0]
    assert (s[:, 0] > s[:, 1]).all() and (s[:, 1] > s[:, 2]).all() and sel["valid"].tolist() == [True, True]
    assert gb.same_bits(sel["RT"], RT[:, 0].contiguous()) and torch.equal(sel["score"], sel["scores"][:, 0])
    # the true pose ruled out in item 0, everything ruled out in item 1: the next best; candidate 0's pose with valid = False
    cands["true"] = (RT[:, 0].contiguous(), torch.tensor([False, False], device="cuda"))
    cands["shifted"] = (RT[:, 1].contiguous(), torch.tensor([True, False], device="cuda"))
    cands["flipped"] = (RT[:, 2].contiguous(), torch.tensor([True, False], device="cuda"))
    sel = pose.select_verified(cands, verify)
    assert sel["which"].tolist() == [1, -1] and sel["valid"].tolist() == [True, False]
    assert gb.same_bits(sel["RT"], torch.stack([RT[0, 1], RT[1, 0]]))
    with pytest.raises(ValueError, match="unknown keys"):
        pose.select_verified(cands, dict(verify, tolerance=1.0))


def test_rendered_frames_to_a_verified_pose():
    """RenderedFrames(keep_frames=True) -> device targets -> every candidate fit -> verification against the batch's own depth frame:
    `which` names a candidate and RT is that candidate's, bit for bit."""
    from geometric_aware_dense_matching_amd import train_lm
    mesh = render.demo_mesh(level=3)
    M, B, N, Hc, Wc = 1024, 2, 1024, 120, 160
    K = np.array([[143.1, 0.0, 81.3], [0.0, 143.4, 60.5], [0.0, 0.0, 1.0]])
    model_xyz = torch.from_numpy(np.ascontiguousarray(model_prep.build_model_points(mesh, M)[:, :3])).cuda()
    scene = render.SceneMeshes([render._as_mesh(mesh), render._as_mesh(render.demo_mesh(level=2, seed=9)),
                                render._as_mesh(render.backdrop_mesh(K, Hc, Wc, z=1.5))])
    kw = dict(S_crop=64, seed=3, n_batches=1, K=K, H=Hc, W=Wc, S=4, z_range=(0.3, 0.6), backdrop_obj=2, build_pyramid=False, train=False)
    plain = render.RenderedFrames(scene, 0, model_xyz, B, N, **kw).batch_at(0)
    item = render.RenderedFrames(scene, 0, model_xyz, B, N, keep_frames=True, **kw).batch_at(0)
    assert set(item) - set(plain) == {"frame_depth", "bbox"} and all(gb.same_bits(plain[k], item[k]) for k in plain if torch.is_tensor(plain[k]))
    assert item["frame_depth"].shape == (B, Hc, Wc) and item["frame_depth"].dtype == torch.float32 and item["bbox"].shape == (B, 4)
    cu = train_lm.device_targets(SimpleNamespace(model_emb=SimpleNamespace(xyz=model_xyz)), train_lm.to_device(item, torch.device("cuda")),
                                 torch.zeros(2, dtype=torch.int64, device="cuda"))          # (the held-out batch's ids are host tensors)
    match = cu["match_idx"]
    res = dict(mask=(match < M).to(torch.uint8), best_idx=match.clamp(max=M - 1).to(torch.int32).contiguous())
    verify = dict(verts=scene.verts[:len(mesh["verts"])], faces=scene.faces[:len(mesh["faces"])], depth=cu["frame_depth"], K=cu["K"],
                  window=pose.boxes_to_windows(cu["bbox"], Hc, Wc), delta=0.01)          # device_targets gathers these with the items
    sel = pose.estimate_poses_verified(res, cu["cld_rgb_nrm"], model_xyz, verify, icp_iters=4)
    C = len(pose.VERIFY_CANDIDATES)
    assert sel["names"] == pose.VERIFY_CANDIDATES and sel["cand_RT"].shape == (B, C, 3, 4) and sel["counts"].shape == (B, C, 6)
    which = sel["which"].tolist()
    print("winner per item %s, scores %s" % ([sel["names"][w] if w >= 0 else None for w in which], sel["scores"].cpu().numpy().round(4).tolist()))
    assert all(-1 <= w < C for w in which) and sel["valid"].tolist() == [w >= 0 for w in which]
    # the candidates are what estimate_poses gives for each name; the winner is one of them, bit for bit
    for c, name in enumerate(sel["names"]):
        fit, _, icp = name.partition("+")
        one = pose.estimate_poses(res, cu["cld_rgb_nrm"], model_xyz, fit, 4 if icp else 0)
        assert gb.same_bits(one["RT"], sel["cand_RT"][:, c].contiguous()), name
    for i, w in enumerate(which):
        assert gb.same_bits(sel["RT"][i], sel["cand_RT"][i, max(w, 0)].contiguous())
    # an item is valid exactly when one of its valid candidates draws min_px pixels into the window; fits on ground-truth
    # correspondences do
    eligible = (sel["cand_valid"] & (sel["counts"][:, :, 0] >= 16)).any(dim=1)
    assert sel["valid"].tolist() == eligible.tolist() and bool(sel["cand_valid"][:, 0].any()) and bool(eligible.any())


def test_graph_capture_and_replay_on_changed_inputs():
    args, kw = _device_args(vc.mixed_case("n3 C5 f32 K,depth per instance"))
    other, _ = _device_args(vc.mixed_case("n3 C5 f64 K,depth shared"))
    verts, faces, RT, depth, K = args
    static_RT, static_depth = RT.clone(), depth.clone()

    def run():
        return pose.verify_poses(verts, faces, static_RT, static_depth, K, **kw)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = {k: v.clone() for k, v in run().items()}
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    assert all(gb.same_bits(first[k], out[k]) for k in first)
    static_RT.copy_(other[2])                                              # other poses, and the depth turned upside down
    static_depth.copy_(depth.flip(1))
    replays = []
    for _ in range(2):
        graph.replay()
        replays.append({k: v.clone() for k, v in out.items()})
    eager = run()
    for r in replays:
        assert all(gb.same_bits(eager[k], r[k]) for k in eager)
    assert not torch.equal(eager["counts"], first["counts"])


def test_no_image_per_candidate_is_allocated():
    """n = 4, C = 8 at 480 x 640: beyond its outputs the call allocates less than ONE [H,W] float image -- a condition (there is no
    [n C, H, W] buffer), not a measurement."""
    n, C, Hf, Wf = 4, 8, 480, 640
    m = render.demo_mesh(level=2, seed=2)
    verts, faces = torch.from_numpy(m["verts"].astype(np.float32)).cuda(), torch.from_numpy(m["faces"]).cuda()
    RT = torch.from_numpy(np.tile(vc.pose(vc.rot(0.7, (0.3, 1.0, 0.2)), (0.0, 0.0, 0.5)), (n, C, 1, 1))).cuda()
    K = torch.tensor([[572.4, 0.0, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]], dtype=torch.float64, device="cuda")
    depth = torch.full((n, Hf, Wf), 0.5, dtype=torch.float32, device="cuda")
    window = torch.tensor([[250, 170, 400, 320]] * n, dtype=torch.int32, device="cuda")
    pose.verify_poses(verts, faces, RT, depth, K, window=window)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = pose.verify_poses(verts, faces, RT, depth, K, window=window)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    outputs = sum(max(512, v.numel() * v.element_size()) for v in out.values())
    print("peak above the inputs: %d bytes, outputs %d bytes; one image is %d bytes" % (extra, outputs, Hf * Wf * 4))
    assert extra - outputs < Hf * Wf * 4
    assert int(out["counts"][0, 0, 0]) > 1000 and out["best"].tolist() == [0] * n


def test_the_entry_stays_inside_its_tensors(wanted, monkeypatch):
    name = "n3 C5 f32 K,depth per instance"
    args, kw = _device_args(vc.mixed_case(name))
    wargs, wkw = _device_args(vc.mixed_case("n1 C1 f32 whole frame"))
    with gb.filled_empties(), gb.guarded_calls(monkeypatch) as st:
        got = pose.verify_poses(*args, **kw)
        whole = pose.verify_poses(*wargs, **wkw)
    assert st.counts["gdm_pose_verify_hip"] == 2
    # the bands and the const inputs were checked by the wrapper; equality in every element says no output kept the allocator's fill
    _equal(got, wanted[name], "guarded")
    _equal(whole, wanted["n1 C1 f32 whole frame"], "guarded, whole frame")


def test_refusals():
    args, kw = _device_args(vc.mixed_case("n1 C1 f32 whole frame"))
    for bad, msg in ((dict(delta=0.0), "delta"), (dict(delta=float("nan")), "delta"), (dict(front_weight=-1.0), "front_weight"),
                     (dict(min_px=-1), "min_px"), (dict(near=-0.1), "near")):
        with pytest.raises(pose._lib.GdmError, match=msg):
            pose.verify_poses(*args, **dict(kw, **bad))
    with pytest.raises(ValueError, match="window"):
        pose.verify_poses(*args, **dict(kw, window=torch.zeros(2, 4, dtype=torch.int32, device="cuda")))
    with pytest.raises(ValueError, match="RT"):
        pose.verify_poses(args[0], args[1], args[2][0], args[3], args[4])
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def small_model():
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    M = 512
    model = GeoMatch(make_model_cfg(n_mesh_node=M), 1, model_points=synthetic.make_model_points(1, M))
    keys = json.load(open(os.path.join(G, "geomatch_state.json")))
    model.load_state_dict(synthetic.synthetic_state_dict({k: torch.zeros(v) for k, v in keys.items()}, seed=0), strict=False)
    return model.cuda().eval()


def test_verify_none_leaves_the_pipeline_step_as_it_was(small_model):
    b = synthetic.make_batch(seed=81, batch=2, n_points=1024)
    batch = {k: torch.from_numpy(b[k]).cuda() for k in ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")}
    with torch.no_grad():
        plain = infer.pipeline_step(small_model, batch, with_pose=True)
        none = infer.pipeline_step(small_model, batch, with_pose=True, verify=None)
        assert set(plain) == set(none)
        ok, bad = infer.outputs_equal(plain, none)
        assert ok, bad
        # with a verify dict the step returns one of the candidates, and says which
        m = render.demo_mesh(level=1)
        verify = dict(verts=m["verts"].astype(np.float32), faces=m["faces"], depth=torch.full((2, 48, 64), 0.5, device="cuda"),
                      K=np.array([[60.0, 0, 32.0], [0, 60.0, 24.0], [0, 0, 1.0]]), candidates=("kabsch", "ransac"), delta=0.02)
        out = infer.pipeline_step(small_model, batch, with_pose=True, verify=verify)
    assert set(out) - set(plain) == {"verify_score", "verify_which", "verify_counts", "verify_cand_RT"}
    assert out["verify_counts"].shape == (2, 2, 6) and out["verify_which"].dtype == torch.int32 and out["verify_score"].dtype == torch.float64
    assert gb.same_bits(out["verify_cand_RT"][:, 0].contiguous(), plain["RT"])
    pick = out["verify_which"].clamp_min(0).long()
    assert gb.same_bits(out["RT"], out["verify_cand_RT"][torch.arange(2, device="cuda"), pick])
    assert all(gb.same_bits(plain[k], out[k]) for k in plain if k not in ("RT", "valid"))


def test_train_lm_pose_verify_on_rendered_frames(tmp_path, capsys):
    """-state=test -data rendered --pose-verify (an untrained model: the poses mean nothing, the plumbing is what runs): a recall table
    per candidate and one for the selection, whose poses are the candidates' and whose csv score is the verification score."""
    from geometric_aware_dense_matching_amd import train_lm
    argv = ("-state=test -data rendered -cls_id=1 --batch-size 2 --n-points 1024 --n-mesh 256 --synthetic-items 4 -checkpoint %s "
            "--pose-verify --verify-delta 0.008 --verify-candidates kabsch,ransac,kabsch+icp --icp-iters 2 --eval-output %s" % (tmp_path, tmp_path)).split()
    res = train_lm.test(train_lm.build_parser().parse_args(argv))
    out = capsys.readouterr().out
    assert len(res) == 2 and all(r["RT"].shape == (2, 3, 4) and r["verify_counts"].shape == (2, 3, 6) for r in res)
    assert all(-1 <= int(w) < 3 for r in res for w in r["verify_which"]) and all(r["score"].shape == (2,) for r in res)
    tables = train_lm.test.last_candidate_tables
    assert list(tables) == ["kabsch", "ransac", "kabsch+icp"]
    for name, t in tables.items():
        assert "--pose-verify candidate %s:" % name in out
        (_, rec), = t.recalls.items()
        assert len(rec["ad_10"]) == 4
    assert "--pose-verify selection (delta 0.008 m):" in out
    csv = [f for f in train_lm.test.last_outputs if f.endswith(".csv")]
    assert len(csv) == 1
    scores = [float(ln.split(",")[3]) for ln in open(csv[0]).read().splitlines()[1:]]
    want = [float(s) for r in res for s in r["score"]]
    assert len(scores) == 4 and np.allclose(scores, want, rtol=1e-5, atol=1e-6)
