#!/usr/bin/env python3
"""Times the consensus pose fit (gdm_consensus_pose_hip, pose.consensus_poses) and writes profiles/pose_consensus.md
(--out).  B = 16 crops, N = 2048 points, M = 8192 vertices, S = 8 seeds, about 60 % of the points selected, inlier share 0.3, from the
generator of the tests (tests/consensus_cases.py).

  whole call       device events over replays of one hipGraph of pose.consensus_poses, alternating over `--rounds` rounds with
                   pose.ransac_poses at H = 20 / 256 / 1024 and pose.solve_poses on the same inputs; medians
  each kernel      the same call, eager, again in a child process under `rocprofv3 --kernel-trace --stats` (a run of its own: one
                   entry launches all six kernels, so events cannot part them)
  density          set bits of the compatibility matrix over n^2, from the degree output
  recovery         share of crops with ADD < 2 sigma = 1e-3 m for kabsch, ransac (H = 20, 1024) and consensus over inlier shares
                   0.5, 0.3, 0.2, 0.1, 0.05; at the defaults and at the settings of the recovery tests (tau 3 mm, inlier_dist 5 mm)
  sensed frames    ADD of kabsch, consensus and their +depth forms on render.RenderedFrames test batches with the depth sensor on and
                   ground-truth correspondences: the set-up of the ADD table of tools/depth_sensor_profile.py
No time is asserted anywhere.
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import consensus_cases as cc  # noqa: E402
from geometric_aware_dense_matching_amd import model_prep, pose, render  # noqa: E402
from geometric_aware_dense_matching_amd.sensor import DepthSensor  # noqa: E402

B, N, M, S = 16, 2048, 8192, 8
SHARES = (0.5, 0.3, 0.2, 0.1, 0.05)


def make_batch(f, mask_kind, seed, n_crops=B):
    model = cc.make_model(M, seed)
    crops = [cc.make_crop(model, N, f, ("profile", seed, b), mask_kind) for b in range(n_crops)]
    cld = np.zeros((n_crops, 9, N), np.float32)
    for b, c in enumerate(crops):
        cld[b, :3] = c["scene"].T
    res = dict(mask=torch.from_numpy(np.stack([c["mask"] for c in crops])).cuda(),
               best_idx=torch.from_numpy(np.stack([c["idx"] for c in crops])).cuda())
    return crops, res, torch.from_numpy(cld).cuda(), torch.from_numpy(model).cuda()


def graphed(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def timed(g, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernel_stats(reps):
    """This tool's eager calls again under rocprofv3 in a child process -> [(kernel, ms per call)] in launch order."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--only-eager", "--reps", str(reps)]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        rows = {}
        for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(fn)):
                if "consensus_" in r["Name"]:
                    key = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].strip()
                    rows[key] = rows.get(key, 0.0) + float(r["TotalDurationNs"]) / 1e6 / reps
    order = ["compact", "pairs", "score", "seeds", "fit", "select"]
    return sorted(rows.items(), key=lambda kv: next((i for i, o in enumerate(order) if o in kv[0]), 99))


def recovery(settings, n_crops):
    """-> {share: {method: share of crops with ADD < 1e-3}} with inlier_dist / tau = settings."""
    tau, dist = settings
    out = {}
    for f in SHARES:
        crops, res, cld, model = make_batch(f, "ones", 100 + int(1000 * f), n_crops)
        fits = {"kabsch": pose.solve_poses(res, cld, model)[0],
                "ransac H=20": pose.ransac_poses(res, cld, model, 20, dist)[0],
                "ransac H=1024": pose.ransac_poses(res, cld, model, 1024, dist)[0],
                "consensus": pose.consensus_poses(res, cld, model, tau, S, dist)["RT"]}
        out[f] = {k: float(np.mean([cc.add_error(rt, c) < 2 * cc.SIGMA for rt, c in zip(v.cpu().numpy(), crops)])) for k, v in fits.items()}
    return out


def sensed_table(dev, batches=2, Bc=8, Nc=512, Mc=1024):
    """ADD (metres) per candidate on sensed RenderedFrames test batches -> {name: (n, mean, median, max)}."""
    from types import SimpleNamespace
    from geometric_aware_dense_matching_amd import train_lm
    mesh = render.demo_mesh(level=3)
    Hc, Wc = 240, 320
    K = np.array([[286.2, 0.0, 162.6], [0.0, 286.8, 121.0], [0.0, 0.0, 1.0]])
    model_xyz = torch.from_numpy(np.ascontiguousarray(model_prep.build_model_points(mesh, Mc)[:, :3])).to(dev)
    scene = render.SceneMeshes([render._as_mesh(mesh), render._as_mesh(render.demo_mesh(level=2, seed=9)),
                                render._as_mesh(render.backdrop_mesh(K, Hc, Wc, z=1.5))])
    frames = render.RenderedFrames(scene, 0, model_xyz, Bc, Nc, keep_frames=True, S_crop=64, seed=5, n_batches=batches, K=K, H=Hc, W=Wc,
                                   S=4, z_range=(0.3, 0.6), backdrop_obj=2, build_pyramid=False, train=False, depth_sensor=DepthSensor())
    names = ("kabsch", "consensus", "kabsch+depth", "consensus+depth")
    adds = {k: [] for k in names}
    for b in range(batches):
        cu = train_lm.device_targets(SimpleNamespace(model_emb=SimpleNamespace(xyz=model_xyz)), train_lm.to_device(frames.batch_at(b), dev),
                                     torch.zeros(2, dtype=torch.int64, device=dev))
        match = cu["match_idx"]
        res = dict(mask=(match < Mc).to(torch.uint8), best_idx=match.clamp(max=Mc - 1).to(torch.int32).contiguous())
        verify = dict(verts=scene.verts[:len(mesh["verts"])], faces=scene.faces[:len(mesh["faces"])], depth=cu["frame_depth"], K=cu["K"],
                      window=pose.boxes_to_windows(cu["bbox"], Hc, Wc), delta=0.01)
        sel = pose.estimate_poses_verified(res, cu["cld_rgb_nrm"], model_xyz, verify, candidates=names, depth_iters=5)
        for c, k in enumerate(names):
            ok = sel["cand_valid"][:, c]
            adds[k] += pose.add_metric(sel["cand_RT"][:, c][ok], cu["RT"][ok][:, :3].float(), model_xyz).tolist()
    return {k: (len(v), float(np.mean(v)), float(np.median(v)), float(np.max(v))) if v else (0,) + (float("nan"),) * 3 for k, v in adds.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--crops", type=int, default=32, help="crops per inlier share of the recovery table")
    ap.add_argument("--no-kernel-stats", action="store_true")
    ap.add_argument("--only-eager", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "pose_consensus.md"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pose_consensus_profile needs the GPU"
    crops, res, cld, model = make_batch(0.3, "most", 0)
    if a.only_eager:
        for _ in range(a.reps):
            pose.consensus_poses(res, cld, model, seeds=S)
        torch.cuda.synchronize()
        return
    kernels = [] if a.no_kernel_stats else kernel_stats(a.reps)           # before this process has queued anything of its own
    forms = {"consensus_poses (S = 8)": lambda: pose.consensus_poses(res, cld, model, seeds=S),
             "ransac_poses H = 20": lambda: pose.ransac_poses(res, cld, model, 20),
             "ransac_poses H = 256": lambda: pose.ransac_poses(res, cld, model, 256),
             "ransac_poses H = 1024": lambda: pose.ransac_poses(res, cld, model, 1024),
             "solve_poses (kabsch)": lambda: pose.solve_poses(res, cld, model)}
    graphs = {k: graphed(fn) for k, fn in forms.items()}
    times = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, g in graphs.items():
            times[k].append(timed(g, a.iters))
    out = pose.consensus_poses(res, cld, model, seeds=S)
    n = (res["mask"] != 0).sum(1).double()
    deg = out["degree"].clamp_min(0).sum(1).double()
    density = (deg / (n * n)).cpu().numpy()
    add = [cc.add_error(rt, c) for rt, c in zip(out["RT"].cpu().numpy(), crops)]
    nbytes = pose.call("gdm_consensus_workspace_bytes", B, N, S)
    L = ["# Consensus pose fit: times and recovery", "",
         "`python tools/pose_consensus_profile.py` on %s, torch %s.  B = %d, N = %d, M = %d, S = %d; %d to %d selected pairs per crop, "
         "inlier share 0.3, sigma = 0.5 mm.  Device events round %d replays of one hipGraph per form, the forms alternating over %d "
         "rounds; median (min .. max) in ms.  Nothing here is a bound; nothing that is not listed was measured." %
         (torch.cuda.get_device_name(0), torch.__version__, B, N, M, S, int(n.min()), int(n.max()), a.iters, a.rounds), "",
         "| call | ms |", "|---|---|"]
    for k, v in times.items():
        L.append("| %s | %.4f (%.4f .. %.4f) |" % (k, float(np.median(v)), min(v), max(v)))
    L += ["", "Workspace of the consensus call: %.2f MiB (the n x n bit matrices are %.2f MiB of it).  Bit-matrix density (set bits over n^2): "
          "mean %.3f, %.3f .. %.3f over the crops.  Worst ADD of the timed batch: %.2e m." %
          (nbytes / 2 ** 20, B * N * (N // 64) * 8 / 2 ** 20, density.mean(), density.min(), density.max(), max(add)), ""]
    if kernels:
        L += ["## Kernels (`rocprofv3 --kernel-trace --stats`, a run of its own: %d eager calls, ms per call)" % a.reps, "",
              "| kernel | ms per call |", "|---|---|"]
        L += ["| %s | %.4f |" % kv for kv in kernels]
        L += ["| sum | %.4f |" % sum(v for _, v in kernels), ""]
    else:
        L += ["Per-kernel times: not measured in this run.", ""]
    for title, settings in (("the defaults: tau = 5 mm, inlier_dist = 15 mm (RANSAC's match_err too)", (0.005, 0.015)),
                            ("the recovery tests' settings: tau = 3 mm, inlier_dist = 5 mm (RANSAC's match_err too)", (0.003, 0.005))):
        table = recovery(settings, a.crops)
        cols = list(next(iter(table.values())))
        L += ["## Share of crops with ADD < 2 sigma = 1e-3 m at %s" % title, "",
              "%d crops per inlier share, n = N = %d pairs each, wrong pairs uniform over the %d vertices." % (a.crops, N, M), "",
              "| inlier share | " + " | ".join(cols) + " |", "|---|" + "---|" * len(cols)]
        L += ["| %.2f | " % f + " | ".join("%.2f" % table[f][c] for c in cols) + " |" for f in SHARES]
        L.append("")
    rows = sensed_table(torch.device("cuda"))
    L += ["## ADD on sensed frames with ground-truth correspondences", "",
          "2 `render.RenderedFrames` test batches of 8 crops, 512 points, 1024 vertices, `DepthSensor()` defaults; the consensus fit at its "
          "defaults; `+depth` = 5 iterations of `refine_poses_depth`.  The matches are ground truth, so there are no wrong pairs to reject: "
          "this shows what the fit does to a good start, not what it does to a bad one.", "",
          "| candidate | n | mean ADD, m | median | max |", "|---|---|---|---|---|"]
    L += ["| %s | %d | %.2e | %.2e | %.2e |" % ((k,) + v) for k, v in rows.items()]
    L.append("")
    text = "\n".join(L)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
