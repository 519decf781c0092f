"""GPU: the consensus fit (csrc/gdm_consensus.hip, include/gdm.h THE CONSENSUS RULE) against pose.consensus_poses_numpy on the seeded
batches of tests/consensus_cases.py.  The integer part of the rule (scores, degrees, seeds) is compared for equality; the fits to the
bounds tests/test_gpu_match_soft.py holds the weighted fit to, behind the conditioning gate of oracle/pose_ref.py; the counts to the
RANSAC tests' convention for pairs within 1e-5 m of the inlier distance.  What is left out is counted, and the count is asserted
(tests/test_consensus_cpu.py shows that the committed seeds leave out nothing).  Every library call runs between guard bands."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import consensus_cases as cc
import guard_bands as gb
from geometric_aware_dense_matching_amd import infer, model_prep, pose, render, synthetic
from geometric_aware_dense_matching_amd.config import make_model_cfg

pytestmark = pytest.mark.gpu

SENTINEL = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -1000]], np.float32)
KEYS = ("RT", "valid", "score", "degree", "seed_idx", "hyp_RT", "counts", "winner")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _inputs(bt, rows=None):
    rows = slice(None) if rows is None else rows
    return dict(mask=_cuda(bt["mask"][rows]), best_idx=_cuda(bt["idx"][rows])), _cuda(bt["cld"][rows]), _cuda(bt["model"])


def _np(out):
    return {k: out[k].cpu().numpy() for k in KEYS}


def _same(a, b):
    return all(gb.same_bits(a[k], b[k]) for k in KEYS)


def _compare(got, refs, crops, seeds=8):
    """One batch against the restatement of each of its crops -> (hypotheses behind the gate, hypotheses, crops excused)."""
    gated, total, excused = 0, 0, 0
    for b, (ref, crop) in enumerate(zip(refs, crops)):
        assert np.array_equal(got["score"][b], ref["score"]) and np.array_equal(got["degree"][b], ref["degree"]), b
        assert np.array_equal(got["seed_idx"][b], ref["seed_idx"]), (b, got["seed_idx"][b], ref["seed_idx"])
        for t in range(seeds):
            if ref["counts"][t] < 0:                                    # no seed, or fewer than 3 pairs of positive weight
                assert got["counts"][b, t] == -1 and np.array_equal(got["hyp_RT"][b, t], SENTINEL), (b, t)
                continue
            total += 1
            assert abs(int(got["counts"][b, t]) - int(ref["counts"][t])) <= ref["near"][t], (b, t, got["counts"][b, t], ref["counts"][t])
            if not cc.fit_gap(ref, crop, t) > 1e-3:
                gated += 1
                continue
            want = ref["hyp_RT"][t]
            err = np.abs(got["hyp_RT"][b, t].astype(np.float64) - want)
            assert err[:, :3].max() <= 1e-7, (b, t, float(err[:, :3].max()))
            assert err[:, 3].max() <= 2.0 ** -23 * max(1.0, float(np.abs(want[:, 3]).max())), (b, t, float(err[:, 3].max()))
        if not cc.winner_pinned(ref):
            excused += 1
            assert (got["winner"][b] >= 0) == bool(got["valid"][b])
            continue
        assert got["winner"][b] == ref["winner"] and bool(got["valid"][b]) == ref["valid"], (b, got["winner"][b], ref["winner"])
        if ref["valid"]:
            assert np.abs(got["RT"][b] - ref["RT"]).max() <= 1e-5, (b, float(np.abs(got["RT"][b] - ref["RT"]).max()))
        else:
            assert got["winner"][b] == -1 and np.array_equal(got["RT"][b], SENTINEL), b
    return gated, total, excused


@pytest.mark.parametrize("name", list(cc.BATCHES))
def test_consensus_vs_restatement(name, monkeypatch):
    bt, refs = cc.batch(name), cc.reference(name)
    res, cld, model = _inputs(bt)
    with gb.guarded_calls(monkeypatch) as calls:
        got = _np(pose.consensus_poses(res, cld, model, min_points=cc.MIN_POINTS))
    assert calls.counts["gdm_consensus_pose_hip"] == 1
    assert np.isfinite(got["RT"]).all() and np.isfinite(got["hyp_RT"]).all()
    gated, total, excused = _compare(got, refs, bt["crops"])
    print("%s: %d of %d hypotheses behind the conditioning gate, %d of %d crops excused" % (name, gated, total, excused, len(refs)))
    assert gated <= 0.05 * total and excused <= len(refs) // 16
    assert gated == 0 and excused == 0                                  # the committed seeds: tests/test_consensus_cpu.py


def test_degenerate_crops_give_the_sentinel():
    """An empty mask, MIN_POINTS - 1 points, and a crop whose pairs are all incompatible with one another (every s = 0: no seed)."""
    bt = cc.batch("3x65")
    res, cld, model = _inputs(bt)
    got = _np(pose.consensus_poses(res, cld, model, min_points=cc.MIN_POINTS))
    assert got["valid"].tolist() == [True, False, False] and got["winner"][1:].tolist() == [-1, -1]
    assert np.array_equal(got["RT"][1], SENTINEL) and np.array_equal(got["RT"][2], SENTINEL)
    assert (got["score"][1] == -1).all() and (got["seed_idx"][1] == -1).all() and (got["counts"][1] == -1).all()
    assert (got["score"][2] >= 0).sum() == cc.MIN_POINTS - 1
    N = 70
    rs = np.random.RandomState(5)
    scene = (rs.rand(1, N, 3) * 0.01 + [0, 0, 0.8]).astype(np.float32)  # scene points within 1.8 cm, their vertices metres apart
    cld = np.zeros((1, 9, N), np.float32)
    cld[0, :3] = scene[0].T
    model = (np.arange(N)[:, None] * np.array([1.0, 0.0, 0.0])).astype(np.float32)
    out = pose.consensus_poses(dict(mask=torch.ones(1, N, dtype=torch.uint8, device="cuda"), best_idx=torch.arange(N, dtype=torch.int32, device="cuda")[None]),
                               _cuda(cld), _cuda(model))
    out = _np(out)
    assert (out["score"] == 0).all() and (out["degree"] == 0).all() and (out["seed_idx"] == -1).all() and (out["counts"] == -1).all()
    assert not out["valid"][0] and out["winner"][0] == -1 and np.array_equal(out["RT"][0], SENTINEL)
    assert all(np.array_equal(out["hyp_RT"][0, t], SENTINEL) for t in range(8))


@pytest.mark.parametrize("name", ["3x65", "2x513"])
def test_a_crop_does_not_depend_on_its_neighbours(name):
    bt = cc.batch(name)
    B = len(bt["crops"])
    whole = pose.consensus_poses(*_inputs(bt), min_points=cc.MIN_POINTS)
    back = pose.consensus_poses(*_inputs(bt, slice(None, None, -1)), min_points=cc.MIN_POINTS)
    for b in range(B):
        alone = pose.consensus_poses(*_inputs(bt, slice(b, b + 1)), min_points=cc.MIN_POINTS)
        for k in KEYS:
            assert gb.same_bits(alone[k][0], whole[k][b].contiguous()), (b, k)
            assert gb.same_bits(back[k][B - 1 - b].contiguous(), whole[k][b].contiguous()), (b, k)


@pytest.mark.parametrize("name", ["2x130", "2x2048"])
def test_eager_calls_and_a_graph_replay_are_bit_identical(name):
    bt = cc.batch(name)
    res, cld, model = _inputs(bt)
    first = pose.consensus_poses(res, cld, model)
    second = pose.consensus_poses(res, cld, model)
    assert _same(first, second)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pose.consensus_poses(res, cld, model)
    for k in KEYS:
        out[k].fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(first, out)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(first, out)


def test_estimate_poses_takes_the_consensus_fit():
    bt = cc.batch("2x130")
    res, cld, model = _inputs(bt)
    opts = dict(consensus_tau=0.004, consensus_seeds=5, consensus_inlier_dist=0.01, min_points=6)
    direct = pose.consensus_poses(res, cld, model, 0.004, 5, 0.01, 6)
    est = pose.estimate_poses(res, cld, model, "consensus", 0, opts)
    assert gb.same_bits(est["RT"], direct["RT"]) and torch.equal(est["valid"], direct["valid"])
    RT, valid = pose.solve_poses(res, cld, model, 6, method="consensus", inlier_dist=0.01, consensus_tau=0.004, consensus_seeds=5)
    assert gb.same_bits(RT, direct["RT"]) and torch.equal(valid, direct["valid"])
    plain = pose.consensus_poses(res, cld, model)
    default = pose.estimate_poses(res, cld, model, "consensus")
    assert gb.same_bits(default["RT"], plain["RT"]) and not gb.same_bits(plain["RT"], direct["RT"])
    with_icp = pose.estimate_poses(res, cld, model, "consensus", 2)
    assert with_icp["icp_iters"].shape == (2,) and torch.isfinite(with_icp["RT"]).all()


def test_consensus_candidates_are_verified_against_the_depth_frame():
    """A small rendered batch (the one of tests/test_gpu_depth_verify.py): consensus and consensus+icp beside kabsch as candidates of
    estimate_poses_verified; `which` names one of them and each candidate is what estimate_poses gives for its name."""
    from geometric_aware_dense_matching_amd import train_lm
    mesh = render.demo_mesh(level=3)
    M, B, N, Hc, Wc = 1024, 2, 1024, 120, 160
    K = np.array([[143.1, 0.0, 81.3], [0.0, 143.4, 60.5], [0.0, 0.0, 1.0]])
    model_xyz = torch.from_numpy(np.ascontiguousarray(model_prep.build_model_points(mesh, M)[:, :3])).cuda()
    scene = render.SceneMeshes([render._as_mesh(mesh), render._as_mesh(render.demo_mesh(level=2, seed=9)),
                                render._as_mesh(render.backdrop_mesh(K, Hc, Wc, z=1.5))])
    kw = dict(S_crop=64, seed=3, n_batches=1, K=K, H=Hc, W=Wc, S=4, z_range=(0.3, 0.6), backdrop_obj=2, build_pyramid=False, train=False)
    item = render.RenderedFrames(scene, 0, model_xyz, B, N, keep_frames=True, **kw).batch_at(0)
    cu = train_lm.device_targets(SimpleNamespace(model_emb=SimpleNamespace(xyz=model_xyz)), train_lm.to_device(item, torch.device("cuda")),
                                 torch.zeros(2, dtype=torch.int64, device="cuda"))
    match = cu["match_idx"]
    res = dict(mask=(match < M).to(torch.uint8), best_idx=match.clamp(max=M - 1).to(torch.int32).contiguous())
    verify = dict(verts=scene.verts[:len(mesh["verts"])], faces=scene.faces[:len(mesh["faces"])], depth=cu["frame_depth"], K=cu["K"],
                  window=pose.boxes_to_windows(cu["bbox"], Hc, Wc), delta=0.01)
    names = ("kabsch", "consensus", "consensus+icp")
    sel = pose.estimate_poses_verified(res, cu["cld_rgb_nrm"], model_xyz, verify, candidates=names, icp_iters=4)
    which = sel["which"].tolist()
    print("winner per item %s, scores %s" % ([names[w] if w >= 0 else None for w in which], sel["scores"].cpu().numpy().round(4).tolist()))
    assert sel["names"] == names and sel["cand_RT"].shape == (B, 3, 3, 4)
    assert all(-1 <= w < 3 for w in which) and sel["valid"].tolist() == [w >= 0 for w in which] and any(w >= 0 for w in which)
    for c, name in enumerate(names):
        fit, _, icp = name.partition("+")
        one = pose.estimate_poses(res, cu["cld_rgb_nrm"], model_xyz, fit, 4 if icp else 0)
        assert gb.same_bits(one["RT"], sel["cand_RT"][:, c].contiguous()), name
    print("consensus - kabsch on ground-truth correspondences: max |dRT| = %.3g" % float((sel["cand_RT"][:, 1] - sel["cand_RT"][:, 0]).abs().max()))
    assert bool(sel["cand_valid"][:, 1].all())                          # fits on ground-truth correspondences


def test_the_pipeline_passes_the_consensus_fit_on():
    """pose_fit="consensus" through infer.pipeline_step, GraphedPipeline (bit-identical to the eager step, replayed on another batch),
    run_multi_object and train_lm's test entry point, on a small model with seeded weights: the plumbing is what runs."""
    from geometric_aware_dense_matching_amd import train_lm
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    M = 512
    model = GeoMatch(make_model_cfg(n_mesh_node=M), 1, model_points=synthetic.make_model_points(1, M))
    keys = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geomatch_state.json")))
    model.load_state_dict(synthetic.synthetic_state_dict({k: torch.zeros(v) for k, v in keys.items()}, seed=0), strict=False)
    model = model.cuda().eval()

    def batch(seed, B=2):
        b = synthetic.make_batch(seed=seed, batch=B, n_points=1024)
        return {k: torch.from_numpy(b[k]).cuda() for k in ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")}

    kw = dict(pose_fit="consensus", icp_iters=2, pose_opts=dict(consensus_seeds=4))
    b0, b1 = batch(81), batch(82)
    with torch.no_grad():
        e1 = infer.pipeline_step(model, b0, with_pose=True, **kw)
        direct = pose.consensus_poses(e1, b0["cld_rgb_nrm"], model.model_emb.xyz, seeds=4)
        plain = infer.pipeline_step(model, b0, with_pose=True, pose_fit="consensus", pose_opts=dict(consensus_seeds=4))
        assert gb.same_bits(plain["RT"], direct["RT"]) and torch.equal(plain["valid"], direct["valid"])
        gp = infer.GraphedPipeline(model, b0, with_pose=True, **kw)
        assert gp.check and all(c.get("bit_identical") for c in gp.check.values()), gp.check
        got = {k: v.clone() for k, v in gp(b1).items()}
        want = infer.pipeline_step(model, b1, with_pose=True, **kw)
        ok, bad = infer.outputs_equal(want, got)
        assert ok, bad
        out = infer.run_multi_object({1: model}, batch(83, B=3), [1, 1, 1], pose_fit="consensus")
    assert out["RT"].shape == (3, 3, 4) and bool(torch.isfinite(out["RT"]).all())
    argv = ("--gpus=0 -state=test -cls_id=1 --single-object --batch-size 2 --n-points 1024 --n-mesh 512 --synthetic-items 4 "
            "--pose-fit consensus --consensus-tau 0.004 --consensus-seeds 4 --consensus-inlier-dist 0.01").split()
    res = train_lm.test(train_lm.build_parser().parse_args(argv))
    assert len(res) == 2 and all(r["RT"].shape == (2, 3, 4) and bool(torch.isfinite(r["RT"]).all()) for r in res)


def test_train_lm_pose_verify_takes_the_consensus_candidates(tmp_path, capsys):
    """-state=test -data rendered --pose-verify with consensus names among the candidates (an untrained model: the plumbing is what
    runs): one recall table per candidate, `which` within range; an unknown name is still refused."""
    from geometric_aware_dense_matching_amd import train_lm
    base = "-state=test -data rendered -cls_id=1 --batch-size 2 --n-points 1024 --n-mesh 256 --synthetic-items 2 -checkpoint %s --pose-verify " % tmp_path
    names = ["kabsch", "consensus", "consensus+icp+depth"]
    argv = (base + "--verify-candidates %s --icp-iters 2 --consensus-seeds 4 --depth-refine-iters 1" % ",".join(names)).split()
    res = train_lm.test(train_lm.build_parser().parse_args(argv))
    out = capsys.readouterr().out
    assert len(res) == 1 and res[0]["RT"].shape == (2, 3, 4) and res[0]["verify_counts"].shape == (2, 3, 6)
    assert all(-1 <= int(w) < 3 for w in res[0]["verify_which"])
    assert list(train_lm.test.last_candidate_tables) == names and all("--pose-verify candidate %s:" % k in out for k in names)
    with pytest.raises(SystemExit, match="consensus, consensus\\+icp"):
        train_lm.test(train_lm.build_parser().parse_args((base + "--verify-candidates kabsch,spectral").split()))


def test_recovery_at_a_tenth_of_inliers():
    """(n, inlier share) = (513, 0.1), the eight seeds of the CPU test in one batch, its settings and its bound: ADD < 1e-3 m."""
    crops = [cc.recovery_crop(513, 0.1, seed) for seed in cc.RECOVERY_SEEDS]
    cld = np.zeros((len(crops), 9, 513), np.float32)
    for b, c in enumerate(crops):
        cld[b, :3] = c["scene"].T
    res = dict(mask=_cuda(np.stack([c["mask"] for c in crops])), best_idx=_cuda(np.stack([c["idx"] for c in crops])))
    out = pose.consensus_poses(res, _cuda(cld), _cuda(crops[0]["model"]), tau=0.003, seeds=8, inlier_dist=0.005)
    assert out["valid"].all()
    add = [cc.add_error(rt, c) for rt, c in zip(out["RT"].cpu().numpy(), crops)]
    RTk, vk = pose.solve_poses(res, _cuda(cld), _cuda(crops[0]["model"]))
    plain = [cc.add_error(rt, c) for rt, c in zip(RTk.cpu().numpy(), crops)]
    print("consensus worst ADD %.2e m, plain Kabsch best ADD %.2e m" % (max(add), min(plain)))
    assert max(add) < 1e-3 and min(plain) > 3e-3
