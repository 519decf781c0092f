"""GPU: pose refinement against the observed depth (gdm_pose_refine_depth_hip, pose.refine_poses_depth) -- one iteration
of the kernels against the host restatement, the rasterised input against the frame renderer, the free run and the converged case,
reproducibility and hipGraph capture, the memory condition, guard bands, refusals and the plumbing up to estimate_poses_verified and
infer.pipeline_step.  (This file sorts before tests/test_gpu_guard_bands.py, whose coverage test wants every entry to have run under
guards by then.)"""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import depth_refine_cases as dc
import guard_bands as gb
import verify_cases as vc
from geometric_aware_dense_matching_amd import infer, model_prep, pose, render, synthetic
from geometric_aware_dense_matching_amd.config import make_model_cfg

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# RT and err against the restatement after ONE iteration from identical fp64 poses.  The per-pair terms are the same fp64 single
# operations on both sides; the sums differ by their order only, at most P 2^-53 relative to the sum of magnitudes (1e-12 at P <= 10^4);
# a scaled pivot >= 1e-3 (asserted for every case in test_pose_depth_refine_cpu.py) amplifies that by at most 1e3; |xi| < 0.1; sin and
# cos may differ by a few ulp.
ONE_ITERATION_TOL = 1e-9


def _dev(case, RT=None):
    args, kw = dc.call_args(case)
    args = list(args)
    if RT is not None:
        args[2] = RT
    args = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args)
    kw = {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    return args, kw


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(a, b):
    return all(gb.same_bits(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", dc.SWEEP)
def test_one_iteration_equals_the_restatement(name):
    """From the case's poses and from the restatement's after 1 and 2 iterations: pairs, status and iters exactly (the rasteriser and
    the fp32 gate are bit-exact on both sides), RT and err to 1e-9."""
    case = dc.sweep_case(name)
    starts, answers = dc.sweep_starts(name)
    worst = 0.0
    for k in range(3):
        args, kw = _dev(case, starts[k])
        assert args[0].dtype == (torch.float32 if case["verts"].dtype == np.float32 else torch.float64)
        got = _host(pose.refine_poses_depth(*args, iters=1, **kw))
        want = answers[k]
        for key, dtype in (("RT", np.float64), ("status", np.int32), ("iters", np.int32), ("err", np.float64), ("pairs", np.int32)):
            assert got[key].dtype == dtype and got[key].shape == want[key].shape, (name, key)
        for key in ("pairs", "status", "iters"):
            assert np.array_equal(got[key], want[key]), "%s start %d: %s\n%s\n%s" % (name, k, key, got[key], want[key])
        still = want["status"] != 0                                        # starved, degenerate, invalid: the pose as it came
        assert got["RT"][still].tobytes() == starts[k][still].tobytes()
        dev = max(float(np.abs(got["RT"] - want["RT"])[~still].max(initial=0.0)), float(np.abs(got["err"] - want["err"]).max()))
        worst = max(worst, dev)
    print("%s: largest deviation of RT / err from the restatement over three starts %.2e" % (name, worst))
    assert worst <= ONE_ITERATION_TOL
    if name == "n1 C5 f32 four tiles":
        assert int(answers[0]["pairs"].max()) > 1500


@pytest.mark.parametrize("name", dc.SWEEP)
def test_pairs_equal_the_frame_renderer(name):
    """The pair count of iteration 1 from render_frames' depth and face images plus torch comparisons, with zero tolerance: the 64-bit
    LDS keys and raster_kernel's keys in memory select the same pixels.  (The composed sums, in torch's order, agree to rounding.)"""
    case = dc.sweep_case(name)
    args, kw = _dev(case)
    got = pose.refine_poses_depth(*args, iters=1, **kw)
    comp = pose.refine_sums_composed(*args, window=kw["window"], reject=kw["reject"], huber=kw["huber"], min_cos=kw["min_cos"], near=kw["near"])
    live = kw["cand_valid"].bool()
    assert comp["pairs"].dtype == torch.int32 and torch.equal(got["pairs"][live], comp["pairs"][live]), (got["pairs"], comp["pairs"])
    assert int(got["pairs"][~live].abs().sum()) == 0


@pytest.mark.parametrize("name", dc.FREE)
def test_free_run(name):
    """4 iterations in one call, tolerance 0: iters and status exactly; the final pose within 10 max(d, 1e-9) of the restatement's
    free run, d = the movement of the restatement's own result under 1e-12 perturbations of the start (measured on the host, 2.6e-12;
    the factor 10 allows for a snapped pixel that none of the 20 draws flipped); ADD to the planted pose within the CPU test's bound."""
    level, scene = name
    case, want = dc.free_case(name), dc.free_run(name)
    args, kw = _dev(case)
    got = _host(pose.refine_poses_depth(*args, iters=4, **kw))
    assert np.array_equal(got["iters"], want["iters"]) and np.array_equal(got["status"], want["status"]) and got["iters"].tolist() == [[4, 4]]
    dev = float(np.abs(got["RT"] - want["RT"]).max())
    p = dc.planted(level, scene)
    ratio = dc.add_error(p["verts"], got["RT"][0, 0], p["true"]) / p["add0"]
    print("%s: |RT - restatement| %.2e, pairs %s, ADD ratio %.2e" % (name, dev, got["pairs"].tolist(), ratio))
    assert np.array_equal(got["pairs"], want["pairs"])
    assert dev <= 10 * max(dc.FREE_PERTURBATION_D, 1e-9)
    assert ratio <= (0.25 if scene == "noise" else 0.01)


def test_converged_case_freezes():
    """tolerance from the restatement's trace: candidate 0 freezes with status 1 in iteration 3, and iterations after the freeze leave
    the pose, err and pairs bit-identical."""
    case, at = dc.converged_case()
    args, kw = _dev(case)
    want = pose.refine_poses_depth_numpy(*dc.call_args(case)[0], iters=6, **dc.call_args(case)[1])
    got3, got6 = (pose.refine_poses_depth(*args, iters=k, **kw) for k in (at, 6))
    assert got6["status"].tolist() == want["status"].tolist() == [[1, 1]] and got6["iters"].tolist() == want["iters"].tolist()
    assert int(got6["iters"][0, 0]) == at and _same(got3, got6)
    assert float(np.abs(got6["RT"].cpu().numpy() - want["RT"]).max()) <= 10 * max(dc.FREE_PERTURBATION_D, 1e-9)


def test_status_paths_and_gate_edges():
    """Status 2 (a 2 x 2 window, a pose behind near, a NaN pose), 3 (the flat triangle: a pivot of exactly 0), 4; the gate's edges."""
    p = dc.planted(2, "clean")
    start = p["start"][None, None]
    behind, nan = start.copy(), start.copy()
    behind[0, 0, 2, 3] = 0.01
    nan[0, 0, 1, 1] = np.nan
    RT = torch.from_numpy(np.concatenate([start, behind, nan, start], axis=1)).cuda()
    valid = torch.tensor([[True, True, True, False]], device="cuda")
    out = pose.refine_poses_depth(p["verts"], p["faces"], RT, torch.from_numpy(p["depth"]).cuda(), p["K"], iters=3, reject=p["reject"],
                                  near=p["near"], cand_valid=valid)
    assert out["status"].tolist() == [[0, 2, 2, 4]] and out["iters"].tolist() == [[3, 0, 0, 0]] and out["pairs"][0, 1:].tolist() == [0, 0, 0]
    assert gb.same_bits(out["RT"][0, 1:], RT[0, 1:]) and not gb.same_bits(out["RT"][0, 0], RT[0, 0])
    out = pose.refine_poses_depth(p["verts"], p["faces"], RT[:, :1], torch.from_numpy(p["depth"]).cuda(), p["K"], iters=3, near=p["near"],
                                  window=torch.tensor([[47, 39, 48, 40]], dtype=torch.int32, device="cuda"))
    assert out["status"].tolist() == [[2]] and int(out["pairs"]) <= 4 and gb.same_bits(out["RT"], RT[:, :1])
    f = dc.flat_case()
    fRT = torch.from_numpy(f["RT"]).cuda()
    out = pose.refine_poses_depth(f["verts"], f["faces"], fRT, torch.from_numpy(f["depth"]).cuda(), f["K"], iters=3, reject=f["reject"],
                                  near=f["near"])
    assert out["status"].tolist() == [[3]] and out["iters"].tolist() == [[0]] and int(out["pairs"]) > 500 and gb.same_bits(out["RT"], fRT)
    for dtype in (np.float32, np.float64):
        e = dc.edge_case(dtype)
        want = pose.refine_depth_sums_numpy(e["verts"], e["faces"], e["RT"][0, 0], e["depth"], e["K"], None, e["reject"], near=e["near"])
        out = pose.refine_poses_depth(torch.from_numpy(e["verts"]).cuda(), e["faces"], torch.from_numpy(e["RT"]).cuda(),
                                      torch.from_numpy(e["depth"]).cuda(), e["K"], iters=1, reject=e["reject"], near=e["near"])
        assert int(out["pairs"]) == want["pairs"] > 500


def test_reproducible_eager_and_graph_replayed():
    case = dc.sweep_case("n3 C5 f32 K,depth per instance")
    args, kw = _dev(case)
    verts, faces, RT, depth, K = args
    static_RT = RT.clone()

    def run():
        return pose.refine_poses_depth(verts, faces, static_RT, depth, K, iters=3, **kw)

    first = {k: v.clone() for k, v in run().items()}
    assert _same(first, run())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for _ in range(2):
        graph.replay()
        assert _same(first, out)
    static_RT.copy_(torch.from_numpy(dc.sweep_starts("n3 C5 f32 K,depth per instance")[0][1]).cuda())     # other poses, replayed
    graph.replay()
    replayed = {k: v.clone() for k, v in out.items()}
    assert _same(run(), replayed) and not gb.same_bits(replayed["RT"], first["RT"])


def test_peak_memory_is_the_planned_workspace():
    """n = 4, C = 8 at 480 x 640: above its inputs and outputs the call holds the planner's workspace and at most 4 KiB more -- a
    condition (no image per candidate exists), not a measurement."""
    n, C, Hf, Wf = 4, 8, 480, 640
    m = render.demo_mesh(level=2, seed=2)
    verts, faces = torch.from_numpy(m["verts"].astype(np.float32)).cuda(), torch.from_numpy(m["faces"]).cuda()
    true = vc.pose(vc.rot(0.7, (0.3, 1.0, 0.2)), (0.0, 0.0, 0.5))
    RT = torch.from_numpy(np.tile(vc.pose(vc.rot(0.72, (0.3, 1.0, 0.2)), (0.001, 0.0, 0.502)), (n, C, 1, 1))).cuda()
    K = torch.tensor([[572.4, 0.0, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]], dtype=torch.float64, device="cuda")
    from geometric_aware_dense_matching_amd import evaluation
    depth = evaluation.render_depth(verts, faces, torch.from_numpy(true[None]).cuda(), K, Hf, Wf, 0.05).expand(n, Hf, Wf).contiguous()
    window = torch.tensor([[250, 170, 400, 320]] * n, dtype=torch.int32, device="cuda")
    planned = pose.call("gdm_pose_refine_depth_workspace_bytes", n, C, Hf, Wf)
    assert planned == n * C * 8 * 10 * 32 * 8
    pose.refine_poses_depth(verts, faces, RT, depth, K, window=window, iters=2)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = pose.refine_poses_depth(verts, faces, RT, depth, K, window=window, iters=2)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    outputs = sum(max(512, -(-v.numel() * v.element_size() // 512) * 512) for v in out.values())
    print("peak above the inputs: %d bytes, outputs %d bytes, planned workspace %d bytes" % (extra, outputs, planned))
    assert extra - outputs <= planned + 4096
    assert out["status"].tolist() == [[0] * C] * n and int(out["pairs"].min()) > 1000


def test_the_entry_stays_inside_its_tensors(monkeypatch):
    """Under guard bands, with torch.empty() filled with NaN (the workspace too: a partial row no workgroup wrote would show): the
    guarded result equals the plain one bit for bit."""
    name = "n3 C5 f64 K,depth shared"                                     # windows across and outside the frame, a starved corner
    args, kw = _dev(dc.sweep_case(name))
    targs, tkw = _dev(dc.sweep_case("n1 C5 f32 four tiles"))
    plain = pose.refine_poses_depth(*args, iters=2, **kw)
    tplain = pose.refine_poses_depth(*targs, iters=2, **tkw)
    with gb.filled_empties(), gb.guarded_calls(monkeypatch) as st:
        got = pose.refine_poses_depth(*args, iters=2, **kw)
        tgot = pose.refine_poses_depth(*targs, iters=2, **tkw)
    assert st.counts["gdm_pose_refine_depth_hip"] == 2
    assert _same(plain, got) and _same(tplain, tgot)
    assert bool(torch.isfinite(got["RT"]).all()) and bool(torch.isfinite(got["err"]).all())


def test_refusals():
    args, kw = _dev(dc.sweep_case("n1 C1 f32 whole frame"))
    for bad, msg in ((dict(iters=0), "iters"), (dict(iters=65), "iters"), (dict(reject=0.0), "reject"), (dict(reject=float("inf")), "reject"),
                     (dict(huber=-1.0), "huber"), (dict(min_cos=1.0), "min_cos"), (dict(min_cos=-0.1), "min_cos"),
                     (dict(tolerance=-1.0), "tolerance"), (dict(pivot_min=0.0), "pivot_min"), (dict(near=-0.1), "near"),
                     (dict(min_px=-1), "min_px")):
        with pytest.raises(pose._lib.GdmError, match=msg):
            pose.refine_poses_depth(*args, **dict(dict(kw, iters=1), **bad))
    with pytest.raises(ValueError, match="window"):
        pose.refine_poses_depth(*args, **dict(kw, window=torch.zeros(2, 4, dtype=torch.int32, device="cuda")))
    ws = torch.empty(16, dtype=torch.float64, device="cuda")
    o = [torch.empty(12, dtype=torch.float64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"),
         torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.float64, device="cuda"),
         torch.empty(1, dtype=torch.int32, device="cuda")]
    with pytest.raises(pose._lib.GdmError, match="workspace_bytes"):
        pose.call("gdm_pose_refine_depth_hip", args[0], 0, args[1], args[2], args[4], 0, args[3], 1, None, None, 1, 1, args[0].shape[0],
                  args[1].shape[0], dc.H, dc.W, 0.05, 1, 0.01, 0.0, 0.0, 16, 0.0, 1e-6, ws, ws.numel() * 8, *o)
    torch.cuda.synchronize()


def test_rendered_frames_to_a_depth_refined_candidate():
    """estimate_poses_verified(("kabsch", "kabsch+depth")) on one RenderedFrames(keep_frames=True) batch: the kabsch rows are what the
    call without the new name gives, bit for bit; the refined candidate scores at least as well wherever its refinement ended with
    status 0 or 1; the selection follows the scores."""
    from geometric_aware_dense_matching_amd import train_lm
    mesh = render.demo_mesh(level=3)
    M, B, N, Hc, Wc = 1024, 2, 512, 120, 160
    K = np.array([[143.1, 0.0, 81.3], [0.0, 143.4, 60.5], [0.0, 0.0, 1.0]])
    model_xyz = torch.from_numpy(np.ascontiguousarray(model_prep.build_model_points(mesh, M)[:, :3])).cuda()
    scene = render.SceneMeshes([render._as_mesh(mesh), render._as_mesh(render.demo_mesh(level=2, seed=9)),
                                render._as_mesh(render.backdrop_mesh(K, Hc, Wc, z=1.5))])
    item = render.RenderedFrames(scene, 0, model_xyz, B, N, keep_frames=True, S_crop=64, seed=3, n_batches=1, K=K, H=Hc, W=Wc, S=4,
                                 z_range=(0.3, 0.6), backdrop_obj=2, build_pyramid=False, train=False).batch_at(0)
    cu = train_lm.device_targets(SimpleNamespace(model_emb=SimpleNamespace(xyz=model_xyz)), train_lm.to_device(item, torch.device("cuda")),
                                 torch.zeros(2, dtype=torch.int64, device="cuda"))
    match = cu["match_idx"]
    res = dict(mask=(match < M).to(torch.uint8), best_idx=match.clamp(max=M - 1).to(torch.int32).contiguous())
    verify = dict(verts=scene.verts[:len(mesh["verts"])], faces=scene.faces[:len(mesh["faces"])], depth=cu["frame_depth"], K=cu["K"],
                  window=pose.boxes_to_windows(cu["bbox"], Hc, Wc), delta=0.01)
    today = pose.estimate_poses_verified(res, cu["cld_rgb_nrm"], model_xyz, verify, candidates=("kabsch",))
    sel = pose.estimate_poses_verified(res, cu["cld_rgb_nrm"], model_xyz, verify, candidates=("kabsch", "kabsch+depth"), depth_iters=4)
    assert sel["names"] == ("kabsch", "kabsch+depth") and sel["cand_RT"].shape == (B, 2, 3, 4) and sel["cand_RT"].dtype == torch.float32
    for k in ("cand_RT", "cand_valid", "counts", "scores"):
        assert gb.same_bits(sel[k][:, 0].contiguous(), today[k][:, 0].contiguous()), k
    status = sel["depth_status"]
    assert status.dtype == torch.int32 and status[:, 0].tolist() == [-1] * B and all(0 <= s <= 4 for s in status[:, 1].tolist())
    ok = (status[:, 1] <= 1) & sel["cand_valid"][:, 0]
    assert sel["cand_valid"][:, 1].tolist() == ok.tolist() and bool(ok.any())
    s = sel["scores"]
    print("scores (kabsch, kabsch+depth) %s, status %s, which %s" % (s.cpu().numpy().round(4).tolist(), status[:, 1].tolist(), sel["which"].tolist()))
    assert bool((s[ok, 1] >= s[ok, 0]).all())
    _, best = pose.verify_select_numpy(sel["counts"].cpu().numpy(), cand_valid=sel["cand_valid"].cpu().numpy())
    assert sel["which"].tolist() == best.tolist()
    with pytest.raises(ValueError, match="candidates"):
        pose.estimate_poses_verified(res, cu["cld_rgb_nrm"], model_xyz, verify, candidates=("kabsch+depth+icp",))
    with pytest.raises(ValueError, match="depth_opts"):
        pose.estimate_poses_verified(res, cu["cld_rgb_nrm"], model_xyz, verify, candidates=("kabsch+depth",), depth_opts=dict(delta=1.0))


@pytest.fixture(scope="module")
def small_model():
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    M = 512
    model = GeoMatch(make_model_cfg(n_mesh_node=M), 1, model_points=synthetic.make_model_points(1, M))
    keys = json.load(open(os.path.join(G, "geomatch_state.json")))
    model.load_state_dict(synthetic.synthetic_state_dict({k: torch.zeros(v) for k, v in keys.items()}, seed=0), strict=False)
    return model.cuda().eval()


def test_pipeline_step_passes_the_depth_keys_through(small_model):
    """Without a +depth name pipeline_step(verify=...) gives what it gave (the kabsch candidate is the plain step's pose, bit for bit,
    and no new key appears); with one, the refined candidate joins the table and its status the outputs."""
    b = synthetic.make_batch(seed=81, batch=2, n_points=1024)
    batch = {k: torch.from_numpy(b[k]).cuda() for k in ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")}
    m = render.demo_mesh(level=1)
    verify = dict(verts=m["verts"].astype(np.float32), faces=m["faces"], depth=torch.full((2, 48, 64), 0.5, device="cuda"),
                  K=np.array([[60.0, 0, 32.0], [0, 60.0, 24.0], [0, 0, 1.0]]), candidates=("kabsch", "ransac"), delta=0.02)
    with torch.no_grad():
        plain = infer.pipeline_step(small_model, batch, with_pose=True)
        old = infer.pipeline_step(small_model, batch, with_pose=True, verify=verify)
        again = infer.pipeline_step(small_model, batch, with_pose=True, verify=dict(verify, depth_iters=2, depth_opts=dict(reject=0.02)))
        new = infer.pipeline_step(small_model, batch, with_pose=True,
                                  verify=dict(verify, candidates=("kabsch", "ransac", "kabsch+depth"), depth_iters=2, depth_opts=dict(reject=0.02)))
    assert set(old) - set(plain) == {"verify_score", "verify_which", "verify_counts", "verify_cand_RT"} and set(again) == set(old)
    assert gb.same_bits(old["verify_cand_RT"][:, 0].contiguous(), plain["RT"])
    ok, bad = infer.outputs_equal(old, again)
    assert ok, bad
    assert set(new) - set(old) == {"verify_depth_status"} and new["verify_cand_RT"].shape == (2, 3, 3, 4)
    assert gb.same_bits(new["verify_cand_RT"][:, :2].contiguous(), old["verify_cand_RT"])
    assert gb.same_bits(new["verify_counts"][:, :2].contiguous(), old["verify_counts"])
    assert new["verify_depth_status"].shape == (2, 3) and new["verify_depth_status"][:, :2].tolist() == [[-1, -1]] * 2


def test_train_lm_accepts_depth_candidates(tmp_path, capsys):
    from geometric_aware_dense_matching_amd import train_lm
    argv = ("-state=test -data rendered -cls_id=1 --batch-size 2 --n-points 1024 --n-mesh 256 --synthetic-items 2 -checkpoint %s "
            "--pose-verify --verify-candidates kabsch,kabsch+depth --depth-refine-iters 2 --depth-refine-reject 0.02 --eval-output %s"
            % (tmp_path, tmp_path)).split()
    res = train_lm.test(train_lm.build_parser().parse_args(argv))
    out = capsys.readouterr().out
    assert len(res) == 1 and res[0]["verify_counts"].shape == (2, 2, 6)
    assert list(train_lm.test.last_candidate_tables) == ["kabsch", "kabsch+depth"]
    assert "--pose-verify candidate kabsch:" in out and "--pose-verify candidate kabsch+depth:" in out
    with pytest.raises(SystemExit, match="verify-candidates"):
        train_lm.test(train_lm.build_parser().parse_args([a.replace("kabsch,kabsch+depth", "kabsch+depth+icp") for a in argv]))
