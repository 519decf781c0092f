"""Timing of the ground-truth targets (targets.pose_gt_info: hidden-point removal + nearest visible vertex) at two shapes:
B=24, N=4096, M=4096 (the reference's training batch) and B=16, N=2048, M=8192 (the headline shape).  Data: the synthetic
ellipsoid model (synthetic.make_model_points), poses at 0.5-1.2 m, half the points on the camera-facing side of the posed model
plus 1-2 mm noise, the rest background.  Device-event timing of back-to-back eager calls and of hipGraph replays after a warm-up;
with --kernel-stats the same workload runs again in a child process under `rocprofv3 --kernel-trace --stats` and the per-kernel
totals are added.  The host cost of the reference's way (scipy ConvexHull of the flipped points + sklearn 1-NN, one crop at a time
on one core) is added where scipy and sklearn import.
    python tools/bench_targets.py [--reps 20] [--kernel-stats] [--out profiles/targets_bench.json]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from geometric_aware_dense_matching_amd import synthetic, targets  # noqa: E402

SHAPES = [(24, 4096, 4096), (16, 2048, 8192)]


def make(B, N, M, seed=0):
    rs = np.random.RandomState(seed)
    model = (synthetic.make_model_points(seed, M)[:, :3] / 1000.0).astype(np.float32)
    RT = np.zeros((B, 3, 4), np.float32)
    cld = np.zeros((B, N, 3), np.float32)
    lab = np.zeros((B, N), np.uint8)
    for b in range(B):
        q, _ = np.linalg.qr(rs.randn(3, 3))
        q *= np.sign(np.linalg.det(q))
        t = np.array([rs.uniform(-0.1, 0.1), rs.uniform(-0.1, 0.1), rs.uniform(0.5, 1.2)])
        RT[b, :, :3], RT[b, :, 3] = q, t
        posed = model @ q.T + t
        front = np.where(posed[:, 2] < np.median(posed[:, 2]))[0]
        n = N // 2
        cld[b, :n] = posed[rs.choice(front, n)] + 0.0015 * rs.randn(n, 3)
        cld[b, n:] = posed.mean(0) + rs.uniform(-0.15, 0.15, size=(N - n, 3))
        lab[b, :n] = 1
    return model, RT, cld, lab


def timeit(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def run_shape(B, N, M, reps):
    model, RT, cld, lab = make(B, N, M)
    dev = torch.device("cuda")
    m, r, c, l = (torch.from_numpy(x).to(dev) for x in (model, RT, cld, lab))
    eager = timeit(lambda: targets.pose_gt_info(c, l, r, m), reps)
    hpr_only = timeit(lambda: targets.visible_vertices(m, r), reps)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        targets.pose_gt_info(c, l, r, m)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = targets.pose_gt_info(c, l, r, m)
    replay = timeit(g.replay, reps)
    want = targets.pose_gt_info(c, l, r, m)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], want[k]) for k in want), "replay differs from eager"
    row = dict(B=B, N=N, M=M, eager_ms_per_batch=round(eager, 3), replay_ms_per_batch=round(replay, 3),
               hpr_only_eager_ms=round(hpr_only, 3), visible_per_crop=float(want["visible_flag"].float().sum(1).mean()),
               valid=int(want["valid"].sum()))
    try:
        from scipy.spatial import ConvexHull
        from sklearn.neighbors import NearestNeighbors
        cam = targets.default_cam_center(RT)
        hull_s, nn_s, reps_cpu = 0.0, 0.0, min(B, 4)
        for b in range(reps_cpu):
            f = targets.spherical_flip(model, cam[b])
            t0 = time.perf_counter()
            vis = ConvexHull(np.append(f, [[0, 0, 0]], axis=0)).vertices[:-1]
            t1 = time.perf_counter()
            posed = np.dot(model[vis], RT[b, :, :3].T) + RT[b, :, 3:].T
            NearestNeighbors(n_neighbors=1).fit(posed).kneighbors(cld[b][lab[b] > 0], return_distance=True)
            t2 = time.perf_counter()
            hull_s += t1 - t0
            nn_s += t2 - t1
        row["cpu_reference_way_ms_per_crop"] = dict(convex_hull=round(1e3 * hull_s / reps_cpu, 2), sklearn_nn=round(1e3 * nn_s / reps_cpu, 2),
                                                    batch_one_core=round(1e3 * (hull_s + nn_s) / reps_cpu * B, 1))
    except ImportError as e:
        row["cpu_reference_way_ms_per_crop"] = "not measured: %s" % e
    return row


def kernel_stats(reps):
    """Re-run this tool (eager calls only) under rocprofv3 in a child process; -> {shape: {kernel: ms per batch}}."""
    out = {}
    for B, N, M in SHAPES:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
                   os.path.abspath(__file__), "--only-eager", "%d,%d,%d" % (B, N, M), "--reps", str(reps)]
            subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            rows = {}
            for fn in files:
                for r in csv.DictReader(open(fn)):
                    name = r["Name"]
                    if "hpr_" in name or "targets_" in name:
                        key = name.replace("(anonymous namespace)::", "").split("(")[0].strip()
                        rows[key] = rows.get(key, 0.0) + float(r["TotalDurationNs"]) / 1e6 / (reps + 3)
            out["B%d_N%d_M%d" % (B, N, M)] = {k: round(v, 4) for k, v in sorted(rows.items(), key=lambda kv: -kv[1])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--only-eager", type=str, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_targets needs the GPU"
    if a.only_eager:
        B, N, M = (int(x) for x in a.only_eager.split(","))
        model, RT, cld, lab = make(B, N, M)
        m, r, c, l = (torch.from_numpy(x).cuda() for x in (model, RT, cld, lab))
        for _ in range(a.reps + 3):
            targets.pose_gt_info(c, l, r, m)
        torch.cuda.synchronize()
        return
    res = dict(shapes=[run_shape(B, N, M, a.reps) for B, N, M in SHAPES], reps=a.reps, device=torch.cuda.get_device_name(0),
               torch=torch.__version__, note="device events around back-to-back calls; replay = one hipGraph of the whole pose_gt_info")
    if a.kernel_stats:
        res["kernel_ms_per_batch"] = kernel_stats(a.reps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
