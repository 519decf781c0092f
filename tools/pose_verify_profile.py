#!/usr/bin/env python3
"""Times pose verification against the observed depth (gdm_pose_verify_hip, pose.verify_poses) and, beside it, the same
counts composed from what the package offered before: evaluation.render_depth into an [n C, H, W] z-buffer plus torch comparisons
(pose.verify_counts_composed) -- the yardstick.  Device-event times, the two forms alternating over `--rounds` rounds, peak memory
of each, one JSON line; profiles/pose_verify.md holds a run.

  n = 16 instances, C = 8 candidates, render.demo_mesh(level=5) (20480 faces), 480 x 640 frames, 128 x 128 windows round the object
  set-up share: the fused call again with every window moved to a corner the object does not reach -- the same four tiles per
  candidate walk all F faces and set them up, and no pixel is shaded or classified -- over the full call.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from geometric_aware_dense_matching_amd import pose, render, synthetic  # noqa: E402

H, W = 480, 640


def rot(angle, axis):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx.dot(Kx)


def timed(fn, iters):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b) / iters, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--level", type=int, default=5, help="render.demo_mesh level: 20 * 4**level faces")
    ap.add_argument("--window", type=int, default=128)
    ap.add_argument("--no-composed", action="store_true", help="skip the composed form (a cleaner kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
    dev = torch.device("cuda:0")
    n, C, win = args.n, args.candidates, args.window
    K = np.asarray(synthetic.LM_K, dtype=np.float64)
    m = render.demo_mesh(level=args.level, seed=1)
    rs = np.random.RandomState(0)
    RT = np.zeros((n, C, 3, 4))
    window = np.zeros((n, 4), dtype=np.int32)
    for i in range(n):
        z = 0.45 + 0.01 * i                                               # about 0.1 across at 0.45..0.6: 95 to 130 pixels wide
        u, v = 100 + 22 * i, 100 + 12 * i                                  # with half a width, inside x < 512 and y < 352
        t = np.array([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z])
        R = rot(0.3 + 0.4 * i, (1.0, 0.5, 0.2 * i))
        for c in range(C):
            RT[i, c] = np.hstack([rot(0.03 * c, rs.randn(3)).dot(R), (t + 0.002 * c * rs.randn(3))[:, None]])
        window[i] = [u - win // 2, v - win // 2, u + win // 2 - 1, v + win // 2 - 1]
    verts = torch.from_numpy(m["verts"].astype(np.float32)).to(dev)
    faces = torch.from_numpy(m["faces"]).to(dev)
    RT_d, K_d, win_d = torch.from_numpy(RT).to(dev), torch.from_numpy(K).to(dev), torch.from_numpy(window).to(dev)
    from geometric_aware_dense_matching_amd import evaluation
    depth = evaluation.render_depth(verts, faces, RT_d[:, 0].contiguous(), K_d, H, W, 0.01)
    depth = torch.where(depth > 0, depth + 0.002, torch.full_like(depth, 1.5))
    corner = torch.tensor([[W - win, H - win, W - 1, H - 1]] * n, dtype=torch.int32, device=dev)    # beyond every object (see above)

    def fused(w=win_d):
        return pose.verify_poses(verts, faces, RT_d, depth, K_d, window=w, delta=0.01, near=0.01)

    def composed():
        return pose.verify_counts_composed(verts, faces, RT_d, depth, K_d, window=win_d, delta=0.01, near=0.01)

    out = fused()
    empty = fused(corner)
    res = dict(n=n, C=C, faces=int(faces.shape[0]), H=H, W=W, window=win, tile=pose.VERIFY_TILE, iters=args.iters, rounds=args.rounds,
               model_px_per_candidate=int(out["counts"][:, :, 0].sum()) // (n * C), corner_windows_model_px=int(empty["counts"][:, :, 0].sum()))
    if not args.no_composed:
        res["composed_equals_fused"] = bool(torch.equal(composed(), out["counts"]))
    f_ms, c_ms, s_ms = [], [], []
    for _ in range(args.rounds):                                           # alternating: other people's work shares the machine
        _, ms, f_mem = timed(fused, args.iters)
        f_ms.append(ms)
        if not args.no_composed:
            _, ms, c_mem = timed(composed, max(2, args.iters // 5))
            c_ms.append(ms)
        _, ms, _ = timed(lambda: fused(corner), args.iters)
        s_ms.append(ms)
    res.update(fused_ms=[round(x, 4) for x in f_ms], fused_peak_bytes=int(f_mem), setup_only_ms=[round(x, 4) for x in s_ms],
               setup_share=round(float(np.median(s_ms) / np.median(f_ms)), 3))
    if not args.no_composed:
        res.update(composed_ms=[round(x, 4) for x in c_ms], composed_peak_bytes=int(c_mem),
                   composed_over_fused=round(float(np.median(c_ms) / np.median(f_ms)), 2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
