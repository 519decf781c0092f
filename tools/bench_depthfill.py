"""Timing of depth completion and of the YCB-V item (frontend.fill_depth, make_inputs_from_boxes(depth_fill=...)) at B=16, 480x640
frames, S=256, N=2048, beside the LineMOD item of tools/bench_frontend.py row (c):
  (e) fill_depth multiscale on the crops              (f) fill_depth fast
  (g) fill_depth multiscale + depth_normals on the crops, eager, and as one hipGraph replay
  (h) make_inputs_from_boxes(depth_fill="multiscale") without the pyramid      (c) the same with depth_fill=None
The crops are the detection-box crops of bench_frontend's frames (5 % holes, parts outside the frame).  Device events around
back-to-back calls after a warm-up, `--rounds` repeated measurements, the variants alternating inside a round.  With --kernel-stats
the eager (e) + (f) run again in a child process under `rocprofv3 --kernel-trace --stats`.
    python tools/bench_depthfill.py [--reps 200] [--rounds 3] [--kernel-stats] [--out profiles/depthfill_bench.json]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_frontend as bf  # noqa: E402
from geometric_aware_dense_matching_amd import frontend  # noqa: E402

B, S, N = bf.B, bf.S, bf.N


def make():
    t = bf.make()
    t["crop_depth"] = frontend.crop_from_boxes(t["rgb"], t["depth"], None, t["K"], t["center"], t["scale"], S)["depth"]
    return t


def fill_normals(t):
    return frontend.depth_normals(frontend.fill_depth(t["crop_depth"]), t["K"])


def measure(t, reps, rounds):
    fns = {
        "e_fill_depth_multiscale": lambda: frontend.fill_depth(t["crop_depth"]),
        "f_fill_depth_fast": lambda: frontend.fill_depth(t["crop_depth"], mode="fast"),
        "g_fill_plus_normals_eager": lambda: fill_normals(t),
        "h_ycbv_item_no_pyramid": lambda: frontend.make_inputs_from_boxes(t["rgb"], t["depth"], t["K"], t["box"], S, N, mask=t["mask"],
                                                                          depth_fill="multiscale"),
        "c_linemod_item_no_pyramid": lambda: frontend.make_inputs_from_boxes(t["rgb"], t["depth"], t["K"], t["box"], S, N,
                                                                             mask=t["mask"]),
    }
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fill_normals(t)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fill_normals(t)
    g.replay()
    want = fill_normals(t)
    torch.cuda.synchronize()
    assert torch.equal(out, want), "replay differs from eager"
    fns["g_fill_plus_normals_graph_replay"] = g.replay
    with bf._NoPyramid():
        for fn in fns.values():
            for _ in range(5):
                fn()
        rows = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                rows[k].append(bf.timeit(fn, reps))
    return rows


def kernel_stats(reps):
    """Re-run the eager (e) + (f) under rocprofv3 in a child process; -> {kernel: ms per call}."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--only-kernels", "--reps", str(reps)]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        rows = {}
        for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(fn)):
                if "fill_" in r["Name"]:
                    key = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].strip()
                    rows[key] = rows.get(key, 0.0) + float(r["TotalDurationNs"]) / 1e6 / reps
    return {k: round(v, 4) for k, v in sorted(rows.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--only-kernels", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depthfill needs the GPU"
    t = make()
    if a.only_kernels:
        for _ in range(a.reps):
            frontend.fill_depth(t["crop_depth"])
            frontend.fill_depth(t["crop_depth"], mode="fast")
        torch.cuda.synchronize()
        return
    rows = measure(t, a.reps, a.rounds)
    filled = frontend.fill_depth(t["crop_depth"])
    res = dict(B=B, S=S, N=N, reps=a.reps, rounds=a.rounds,
               ms_per_batch={k: dict(median=round(float(np.median(v)), 4), runs=[round(x, 4) for x in v]) for k, v in rows.items()},
               launches=dict(multiscale="1 memset + 3 kernels", fast="1 kernel"),
               valid_fraction=dict(crop=round(float((t["crop_depth"] > 1e-6).float().mean()), 4),
                                   filled=round(float((filled > 1e-6).float().mean()), 4)),
               device=torch.cuda.get_device_name(0), torch=torch.__version__,
               note="device events around back-to-back calls, median of the rounds; the pyramid is stubbed out of (h) and (c)")
    if a.kernel_stats:
        res["kernel_ms_per_call"] = kernel_stats(a.reps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
