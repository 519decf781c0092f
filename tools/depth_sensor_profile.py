#!/usr/bin/env python3
"""Times the depth sensor (gdm_depth_sensor_hip, sensor.simulate_depth_sensor) and writes profiles/depth_sensor.md (--out).
Device-event times, the forms alternating over `--rounds` rounds, medians reported.

  the call         16 frames of 480 x 640 drawn by render.render_frames (three demo meshes on a backdrop, LineMOD's K), every stage on;
                   also with the shadow stage off and with the noise stage alone, to see what the halo and the window scan cost;
                   each eagerly and as ten calls captured in one hipGraph (the device's time without the host's share)
  beside it        the render_frames call that produced the frames, and a plain device copy that moves the same bytes: the kernel
                   reads 4 B and writes 5 B per pixel, so the copy is one of 4.5 B per pixel each way
  ADD              the candidate table of tools/pose_depth_refine_profile.py (kabsch, kabsch+icp, kabsch+depth on RenderedFrames test
                   batches with ground-truth correspondences) with the sensor off and on, on the same frames
No time is asserted anywhere; the ADD table is a record, not a gate.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from geometric_aware_dense_matching_amd import model_prep, pose, render, sensor, synthetic  # noqa: E402

H, W = 480, 640


def timed(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b) / iters


def graphed(fn, reps, iters):
    """ms per call of `fn` with `reps` calls captured in one hipGraph: the device's time, without the host's share of an eager call."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    graph.replay()
    return timed(graph.replay, iters)[1] / reps


def time_call(n, iters, rounds, dev):
    K = np.asarray(synthetic.LM_K, dtype=np.float64)
    meshes = [render.demo_mesh(level=5, seed=s) for s in (1, 2, 3)]
    scene = render.SceneMeshes([render._as_mesh(m) for m in meshes] + [render._as_mesh(render.backdrop_mesh(K, H, W, z=1.5))])
    slot_obj, RT = render.sample_scene_poses(n, 4, 7, K, H, W, z_range=(0.45, 1.0), target_obj=0, distractor_objs=(1, 2), backdrop_obj=3)
    so, RT_d, K_d = torch.from_numpy(slot_obj).to(dev), torch.from_numpy(RT).to(dev), torch.from_numpy(K).to(dev)
    K32 = K.astype(np.float32)
    full = sensor.DepthSensor()
    forms = {"all": full, "no_shadow": full.replace(stages=("range", "grazing", "jitter", "noise")), "noise_only": full.replace(stages=("noise",))}

    def draw():
        return render.render_frames(scene, so, RT_d, K_d, H, W)

    depth = draw()["depth"]
    src = torch.empty(int(n * H * W * 4.5), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    out = sensor.simulate_depth_sensor(depth, K32, full, seed=1)
    hist = torch.bincount(out["cause"].flatten().long(), minlength=6).tolist()
    ms = dict(render=[], copy=[], **{k: [] for k in forms})
    for _ in range(rounds):                                                # alternating: other people's work shares the machine
        for k, s in forms.items():
            ms[k].append(timed(lambda: sensor.simulate_depth_sensor(depth, K32, s, seed=1), iters)[1])
        ms["copy"].append(timed(lambda: dst.copy_(src), iters)[1])
        ms["render"].append(timed(draw, max(2, iters // 4))[1])
    res = {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}
    for k, s in forms.items():                                            # ten calls per graph: what the device alone needs
        res[k + "_graph"] = graphed(lambda: sensor.simulate_depth_sensor(depth, K32, s, seed=1), 10, max(2, iters // 4))
    res["copy_graph"] = graphed(lambda: dst.copy_(src), 10, max(2, iters // 4))
    return res, hist, sensor.frame_constants(K32, full)


def add_table(dev, depth_sensor, batches=2, B=8, N=512, M=1024):
    """ADD (mean vertex distance to the ground-truth pose, metres) of three candidates on RenderedFrames test batches: the set-up of
    tools/pose_depth_refine_profile.py, with `depth_sensor` between the renderer and everything that reads depth."""
    from geometric_aware_dense_matching_amd import train_lm
    mesh = render.demo_mesh(level=3)
    Hc, Wc = 240, 320
    K = np.array([[286.2, 0.0, 162.6], [0.0, 286.8, 121.0], [0.0, 0.0, 1.0]])
    table = model_prep.build_model_points(mesh, M)
    model_xyz = torch.from_numpy(np.ascontiguousarray(table[:, :3])).to(dev)
    model_nrm = torch.from_numpy(np.ascontiguousarray(table[:, 6:9])).to(dev)
    scene = render.SceneMeshes([render._as_mesh(mesh), render._as_mesh(render.demo_mesh(level=2, seed=9)),
                                render._as_mesh(render.backdrop_mesh(K, Hc, Wc, z=1.5))])
    frames = render.RenderedFrames(scene, 0, model_xyz, B, N, keep_frames=True, S_crop=64, seed=5, n_batches=batches, K=K, H=Hc, W=Wc, S=4,
                                   z_range=(0.3, 0.6), backdrop_obj=2, build_pyramid=False, train=False, depth_sensor=depth_sensor)
    names = ("kabsch", "kabsch+icp", "kabsch+depth")
    adds, status, causes = {k: [] for k in names}, [], np.zeros(6, dtype=np.int64)
    for b in range(batches):
        item = frames.batch_at(b)
        if "depth_cause" in item:
            causes += np.asarray(torch.bincount(item["depth_cause"].flatten().long(), minlength=6).tolist())
        cu = train_lm.device_targets(SimpleNamespace(model_emb=SimpleNamespace(xyz=model_xyz)), train_lm.to_device(item, dev),
                                     torch.zeros(2, dtype=torch.int64, device=dev))
        match = cu["match_idx"]
        res = dict(mask=(match < M).to(torch.uint8), best_idx=match.clamp(max=M - 1).to(torch.int32).contiguous())
        verify = dict(verts=scene.verts[:len(mesh["verts"])], faces=scene.faces[:len(mesh["faces"])], depth=cu["frame_depth"], K=cu["K"],
                      window=pose.boxes_to_windows(cu["bbox"], Hc, Wc), delta=0.01)
        sel = pose.estimate_poses_verified(res, cu["cld_rgb_nrm"], model_xyz, verify, candidates=names, icp_iters=10,
                                           pose_opts=dict(icp_metric="plane"), model_nrm=model_nrm, depth_iters=5)
        for c, k in enumerate(names):
            ok = sel["cand_valid"][:, c]
            adds[k] += pose.add_metric(sel["cand_RT"][:, c][ok], cu["RT"][ok][:, :3].float(), model_xyz).tolist()
        status += sel["depth_status"][:, 2].tolist()
    rows = {k: (len(v), float(np.mean(v)), float(np.median(v)), float(np.max(v))) if v else (0, float("nan"), float("nan"), float("nan"))
            for k, v in adds.items()}
    return rows, status, causes.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "depth_sensor.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
    dev = torch.device("cuda:0")
    ms, hist, (_fx, _fy, _cx, _cy, fb, wd) = time_call(args.n, args.iters, args.rounds, dev)
    px = args.n * H * W
    rng = lambda k: "%.3f (%.3f-%.3f)" % ms[k]
    row = lambda k: "%s | %.3f | %.0f" % (rng(k), ms[k + "_graph"], 9.0 * px / (ms[k + "_graph"] * 1e-3) / 1e9)
    L = ["# sensor.simulate_depth_sensor: time of the call, and what sensed depth does to the pose candidates", "",
         "Written by `tools/depth_sensor_profile.py` on %s: %d frames of %d x %d drawn by `render.render_frames` (three level-5 demo meshes "
         "and a backdrop, LineMOD's K: fb = %.2f, shadow window Wd = %d pixels), `DepthSensor()` defaults, device events.  Eager: %d rounds "
         "of %d calls alternating between the forms, medians (range) -- the host's share of a call included.  Graph: ten calls captured in "
         "one hipGraph, per call -- the device alone; the GB/s column is the 9 B per pixel the kernel must move over that time.  No time "
         "is asserted anywhere." %
         (torch.cuda.get_device_name(0), args.n, H, W, float(fb), wd, args.rounds, args.iters), "",
         "| form | eager, ms | in a graph, ms | GB/s |", "|---|---|---|---|",
         "| sensor, all stages | %s |" % row("all"),
         "| sensor, shadow stage off (no window columns, no scan) | %s |" % row("no_shadow"),
         "| sensor, noise and quantisation only | %s |" % row("noise_only"),
         "| device copy of the same bytes (4.5 B per pixel each way) | %s |" % row("copy"),
         "| the `render_frames` call that drew the frames | %s | | |" % rng("render"), "",
         "Causes over the %d pixels of the timed call (measured, empty, range, shadow, grazing, outside): %s." % (px, hist), ""]
    s_on = sensor.DepthSensor(z_min=0.25)
    L += ["## ADD on RenderedFrames test batches, sensor off and on (ground-truth correspondences, 240 x 320 frames, level-3 mesh)", "",
          "The set-up of `tools/pose_depth_refine_profile.py`, the same frames in both halves.  The targets stand at 0.3 to 0.6 m, so the "
          "sensor here is `%r`: with the default z_min of 0.4 m the nearer half of them would return no depth at all.  The crop's "
          "points, the verification and the `+depth` refinement all read the sensed frame; the correspondences stay the ground truth's.  "
          "A record, not a gate." % (s_on,), "",
          "| sensor | candidate | valid items | mean ADD, m | median | max |", "|---|---|---|---|---|---|"]
    notes = []
    for label, s in (("off", None), ("on", s_on)):
        rows, status, causes = add_table(dev, s)
        L += ["| %s | %s | %d | %.3e | %.3e | %.3e |" % ((label, k) + v) for k, v in rows.items()]
        notes.append("Sensor %s: refinement status of `kabsch+depth` per item %s%s." %
                     (label, status, "; causes of the frames' pixels %s" % causes if s is not None else ""))
    L += [""] + notes + [""]
    text = "\n".join(L)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
