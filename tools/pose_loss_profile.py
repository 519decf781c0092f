#!/usr/bin/env python
"""Measurements of the pose-fit loss (pose.kabsch_pose_loss) on the GPU, written to profiles/pose_fit_loss.md.

  operator   forward + backward at the training shape (B = 24, N = 4096, K = 256 and 1024, S = 1) beside the plain-torch reference
             (pose.kabsch_pose_loss_reference: torch.linalg.svd and autograd) on the same GPU and the same inputs, in f32 and f64;
             device events round `--iters` calls, `--repeats` windows, median and spread, after a warm-up of every shape
  --step     the training step at the reference default shape with the loss off and on (tools/bench_train.py's step, eager)
  kernels    run the tool under `rocprofv3 --kernel-trace --stats -- python tools/pose_loss_profile.py --trace-only` in a call of its
             own for per-kernel times; this tool does not trace.

    python tools/pose_loss_profile.py [--iters 50] [--repeats 7] [--step] [--out profiles/pose_fit_loss.md]
It needs a GPU: without one it stops, it does not fall back."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from geometric_aware_dense_matching_amd import pose  # noqa: E402


def make_inputs(B, N, K, seed=0):
    """Soft vertices near the true model points of a posed crop, weights in (0.2, 1], a ground truth a few degrees off."""
    rs = np.random.RandomState(seed)
    A = rs.uniform(-0.1, 0.1, (B, N, 3))
    R = np.stack([np.linalg.qr(rs.randn(3, 3))[0] for _ in range(B)])
    R[np.linalg.det(R) < 0, :, 0] *= -1
    t = rs.uniform(-0.2, 0.2, (B, 3)) + [0, 0, 0.8]
    cld = rs.randn(B, 9, N)
    cld[:, :3] = np.einsum("bij,bnj->bin", R, A) + t[:, :, None] + 2e-3 * rs.randn(B, 3, N)
    gt = np.concatenate([R, t[:, :, None] + 0.005], axis=2)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return f(cld), f(A), f(rs.uniform(0.2, 1.0, (B, N))), f(gt), f(rs.uniform(-0.1, 0.1, (K, 3)))


def timed(fn, iters, repeats):
    """Median and (min, max) of `repeats` windows of `iters` calls, microseconds per call, by device events."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(per), min(per), max(per)


def operator_rows(iters, repeats):
    rows = []
    for K in (256, 1024):
        cld, A, w, gt, X = make_inputs(24, 4096, K)
        up = torch.rand(24, device="cuda") + 0.5

        def kernel():
            a, ww = A.detach().requires_grad_(True), w.detach().requires_grad_(True)
            out = pose.kabsch_pose_loss(cld, a, ww, gt, X)
            torch.autograd.grad((out[0] * up).sum(), (a, ww))

        def reference(dt):
            c, g, x, u = cld.to(dt), gt.to(dt), X.to(dt), up.to(dt)

            def run():
                a, ww = A.to(dt).requires_grad_(True), w.to(dt).requires_grad_(True)
                out = pose.kabsch_pose_loss_reference(c, a, ww, g, x)
                torch.autograd.grad((out[0] * u).sum(), (a, ww))
            return run
        rows.append(("kernels, f32 in / f64 inside", K) + timed(kernel, iters, repeats))
        rows.append(("torch reference, f32", K) + timed(reference(torch.float32), max(iters // 10, 3), repeats))
        rows.append(("torch reference, f64", K) + timed(reference(torch.float64), max(iters // 10, 3), repeats))
    return rows


def step_rows(iters, repeats):
    """The eager training step at the reference default shape (tools/bench_train.py's model and batch), loss off / on."""
    from geometric_aware_dense_matching_amd import train_lm
    args = train_lm.build_parser().parse_args(["-cls_id=1", "--batch-size", "24"])
    dev = torch.device("cuda", 0)
    rows = []
    for tag, wp in (("pose loss off", 0.0), ("pose loss on (weight 1, K = 256, uniform)", 1.0)):
        torch.manual_seed(0)
        model = train_lm.build_model(args, 1).to(dev).train()
        model.pose_loss_weight = wp
        opt = torch.optim.Adam(model.parameters(), lr=1e-6)
        ds = train_lm.SyntheticCrops(args.batch_size, args.n_points, args.n_mesh, seed=3)
        batch = torch.utils.data.default_collate([ds[i] for i in range(args.batch_size)])

        def step():
            out, _ = train_lm.model_fn_dec(model, batch, dev)
            out["loss"].backward()
            opt.step()
            opt.zero_grad()
        rows.append((tag, "B=%d N=%d M=%d" % (args.batch_size, args.n_points, args.n_mesh)) + timed(step, iters, repeats))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step", action="store_true", help="also time the eager training step with the loss off and on")
    ap.add_argument("--step-iters", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true", help="run the operator a few times and write nothing (for rocprofv3)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_fit_loss.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_loss_profile: no GPU; a time is measured on the GPU or not at all")
    if a.trace_only:
        operator_rows(5, 1)
        return
    lines = ["# The pose-fit loss: measurements", "",
             "Written by `tools/pose_loss_profile.py` on %s (%s, torch %s).  Microseconds per call, device events round %d calls"
             % (time.strftime("%Y-%m-%d"), torch.cuda.get_device_name(0), torch.__version__, a.iters),
             "(a tenth of that for the reference), %d windows: median (min - max), after a warm-up of every shape." % a.repeats, "",
             "## Operator, forward + backward, B = 24, N = 4096, S = 1", "",
             "| path | K | median us | min - max us |", "|---|---|---|---|"]
    for name, K, med, lo, hi in operator_rows(a.iters, a.repeats):
        lines.append("| %s | %d | %.1f | %.1f - %.1f |" % (name, K, med, lo, hi))
    lines += ["", "The reference fits the 24 crops in a Python loop (`torch.linalg.svd` per crop) and reads states on the host; the",
              "operator is three launches with no host read.  Per-kernel times: not measured here (run the tool with `--trace-only`",
              "under `rocprofv3 --kernel-trace --stats` in a call of its own)."]
    if a.step:
        lines += ["", "## Eager training step, reference default shape", "", "| step | shape | median us | min - max us |", "|---|---|---|---|"]
        for name, shape, med, lo, hi in step_rows(a.step_iters, min(a.repeats, 4)):
            lines.append("| %s | %s | %.0f | %.0f - %.0f |" % (name, shape, med, lo, hi))
        lines += ["", "With the weight 0 nothing of the loss runs (tests/test_gpu_pose_loss.py holds the keys and the launches' absence), so",
                  "the step against the parent commit is the parent's own step; four alternating runs against a parent checkout: not measured."]
    lines += ["", "## Learnability", "",
              "Held-out ADD of `kabsch` and of the soft weighted fit after training with and without `--pose-loss-weight`: not measured.",
              "Whether the term helps a trained network is open."]
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
