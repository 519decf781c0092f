#!/usr/bin/env python3
"""Times pose refinement against the observed depth (gdm_pose_refine_depth_hip, pose.refine_poses_depth) and writes
profiles/pose_depth_refine.md (--out).  Device-event times, the forms alternating over `--rounds` rounds, medians reported.

  n = 16 instances, C = 8 candidates, 480 x 640 frames, 128 x 128 windows round the object, render.demo_mesh levels 3 and 5
  per iteration    one call with iters = 1 (the init launch, one accumulation, one solve), and a call with iters = 4 divided by 4
  yardstick 1      one pose.verify_poses call at the same shapes in the same run: an iteration does that call's rasterisation (with
                   64-bit keys) plus the accumulation
  yardstick 2      the composed form, pose.refine_sums_composed: render_frames' kernel into [n C, H, W] depth and face images plus
                   torch gathers and sums
  set-up share     the iters = 1 call again with every window moved to a corner no object reaches: the same tiles walk all F faces
                   and set them up, nothing is shaded or accumulated -- over the full iters = 1 call
  ADD              on render.RenderedFrames test batches with ground-truth correspondences: kabsch, kabsch+icp (point-to-plane) and
                   kabsch+depth through pose.estimate_poses_verified
No time is asserted anywhere.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from geometric_aware_dense_matching_amd import evaluation, model_prep, pose, render, synthetic  # noqa: E402

H, W = 480, 640


def rot(angle, axis):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx.dot(Kx)


def timed(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b) / iters


def time_level(level, n, C, win, iters, rounds, dev):
    K = np.asarray(synthetic.LM_K, dtype=np.float64)
    m = render.demo_mesh(level=level, seed=1)
    rs = np.random.RandomState(0)
    RT = np.zeros((n, C, 3, 4))
    window = np.zeros((n, 4), dtype=np.int32)
    for i in range(n):
        z = 0.45 + 0.01 * i                                               # about 0.1 across at 0.45..0.6: 95 to 130 pixels wide
        u, v = 100 + 22 * i, 100 + 12 * i                                  # with half a width, inside x < 512 and y < 352
        t = np.array([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z])
        R = rot(0.3 + 0.4 * i, (1.0, 0.5, 0.2 * i))
        for c in range(C):
            RT[i, c] = np.hstack([rot(0.01 * c, rs.randn(3)).dot(R), (t + 0.0005 * c * rs.randn(3))[:, None]])
        window[i] = [u - win // 2, v - win // 2, u + win // 2 - 1, v + win // 2 - 1]
    verts = torch.from_numpy(m["verts"].astype(np.float32)).to(dev)
    faces = torch.from_numpy(m["faces"]).to(dev)
    RT_d, K_d, win_d = torch.from_numpy(RT).to(dev), torch.from_numpy(K).to(dev), torch.from_numpy(window).to(dev)
    depth = evaluation.render_depth(verts, faces, RT_d[:, 0].contiguous(), K_d, H, W, 0.01)
    depth = torch.where(depth > 0, depth, torch.full_like(depth, 1.5))
    corner = torch.tensor([[W - win, H - win, W - 1, H - 1]] * n, dtype=torch.int32, device=dev)    # beyond every object (see above)

    def refine(k, w=win_d):
        return pose.refine_poses_depth(verts, faces, RT_d, depth, K_d, window=w, iters=k, reject=0.01, near=0.01)

    def verify():
        return pose.verify_poses(verts, faces, RT_d, depth, K_d, window=win_d, delta=0.01, near=0.01)

    def composed():
        return pose.refine_sums_composed(verts, faces, RT_d, depth, K_d, window=win_d, reject=0.01, near=0.01)

    one, four, comp = refine(1), refine(4), composed()
    res = dict(level=level, faces=int(faces.shape[0]), pairs_per_candidate=int(one["pairs"].sum()) // (n * C),
               status_after_4=sorted(set(four["status"].flatten().tolist())), corner_pairs=int(refine(1, corner)["pairs"].sum()),
               composed_pairs_equal=bool(torch.equal(comp["pairs"], one["pairs"])))
    ms = dict(one=[], four=[], verify=[], composed=[], setup=[])
    for _ in range(rounds):                                                # alternating: other people's work shares the machine
        ms["one"].append(timed(lambda: refine(1), iters)[1])
        ms["verify"].append(timed(verify, iters)[1])
        ms["four"].append(timed(lambda: refine(4), max(2, iters // 4))[1])
        ms["composed"].append(timed(composed, max(2, iters // 10))[1])
        ms["setup"].append(timed(lambda: refine(1, corner), iters)[1])
    res.update({k + "_ms": float(np.median(v)) for k, v in ms.items()})
    res.update({k + "_ms_range": (float(min(v)), float(max(v))) for k, v in ms.items()})
    return res


def add_table(dev, batches=2, B=8, N=512, M=1024):
    """ADD (mean vertex distance to the ground-truth pose, metres) of three candidates on RenderedFrames test batches."""
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
                                   z_range=(0.3, 0.6), backdrop_obj=2, build_pyramid=False, train=False)
    names = ("kabsch", "kabsch+icp", "kabsch+depth")
    adds, status = {k: [] for k in names}, []
    for b in range(batches):
        cu = train_lm.device_targets(SimpleNamespace(model_emb=SimpleNamespace(xyz=model_xyz)), train_lm.to_device(frames.batch_at(b), dev),
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
    return {k: (len(v), float(np.mean(v)), float(np.median(v)), float(np.max(v))) for k, v in adds.items()}, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--levels", type=str, default="3,5", help="render.demo_mesh levels: 20 * 4**level faces")
    ap.add_argument("--window", type=int, default=128)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "pose_depth_refine.md"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
    dev = torch.device("cuda:0")
    rows = [time_level(int(lv), args.n, args.candidates, args.window, args.iters, args.rounds, dev) for lv in args.levels.split(",")]
    adds, status = add_table(dev)
    L = ["# pose.refine_poses_depth: time per iteration", "",
         "Written by `tools/pose_depth_refine_profile.py` on %s: n = %d, C = %d, %d x %d frames, %d x %d windows, device events, %d rounds "
         "of %d calls alternating between the forms, medians (range).  No time is asserted anywhere." %
         (torch.cuda.get_device_name(0), args.n, args.candidates, H, W, args.window, args.window, args.rounds, args.iters), "",
         "| mesh | faces | pairs / candidate | iters = 1 call, ms | iters = 4 call / 4, ms | verify_poses, ms | composed form, ms | "
         "corner windows (set-up only), ms | set-up share |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        rng = lambda k: "%.3f (%.3f-%.3f)" % ((r[k + "_ms"],) + r[k + "_ms_range"])
        L.append("| level %d | %d | %d | %s | %.3f | %s | %s | %s | %.0f %% |" % (
            r["level"], r["faces"], r["pairs_per_candidate"], rng("one"), r["four_ms"] / 4, rng("verify"), rng("composed"), rng("setup"),
            100 * r["setup_ms"] / r["one_ms"]))
    L += ["", "Checks made in the run: " + "; ".join(
        "level %d: composed pair counts equal the kernel's: %s, status after 4 iterations %s, pairs with corner windows %d" %
        (r["level"], r["composed_pairs_equal"], r["status_after_4"], r["corner_pairs"]) for r in rows) + ".", "",
          "## ADD on RenderedFrames test batches (ground-truth correspondences, 240 x 320 frames, level-3 mesh)", "",
          "| candidate | valid items | mean ADD, m | median | max |", "|---|---|---|---|---|"]
    L += ["| %s | %d | %.3e | %.3e | %.3e |" % ((k,) + v) for k, v in adds.items()]
    L += ["", "Refinement status of `kabsch+depth` per item: %s." % status, ""]
    text = "\n".join(L)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
