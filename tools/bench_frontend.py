"""Timing of the box front end (frontend.depth_normals, crop_from_boxes, make_inputs_from_boxes) at B=16, 480x640 frames, S=256,
N=2048, beside the integer-crop front end it extends (frontend.make_inputs, unchanged):
  (a) depth_normals                                   (b) crop_from_boxes at the detection boxes, and at identity boxes
  (c) make_inputs_from_boxes without the pyramid      (d) make_inputs without the pyramid, same frames, identity boxes
  (d_crop) the crop part of (d): depth_to_xyz + the fancy-indexing crops of rgb, normals and mask, as make_inputs does them
"Without the pyramid": pyramid.build_pyramid is stubbed out for the timed calls (it is the same call in (c) and (d)).  Data:
synthetic.make_frame frames with synthetic.make_box_mask detections.  Device events around back-to-back eager calls after a
warm-up, `--rounds` repeated measurements of each, the variants alternating inside a round; (a)+(b) also as hipGraph replays.  With
--kernel-stats the eager (a)+(b) run again in a child process under `rocprofv3 --kernel-trace --stats`.
    python tools/bench_frontend.py [--reps 200] [--rounds 3] [--kernel-stats] [--out profiles/frontend_bench.json]"""
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

from geometric_aware_dense_matching_amd import frontend, synthetic  # noqa: E402

B, H, W, S, N = 16, 480, 640, 256, 2048
HEADLINE_STEP_MS = 3.1              # the headline step this front end feeds (B=16, N=2048 x M=8192), DESIGN.md 5


def make(seed=0):
    rs = np.random.RandomState(seed)
    fr = [synthetic.make_frame(rs) for _ in range(B)]
    det = [synthetic.make_box_mask(rs) for _ in range(B)]
    t = dict(depth=np.stack([f[0] for f in fr]), rgb=np.stack([f[1] for f in fr]), mask=np.stack([d[1] for d in det]),
             box=np.stack([d[0] for d in det]), K=np.stack([synthetic.LM_K] * B))
    t = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
    t["origin"] = torch.tensor([[(37 * b) % (W - S), (23 * b) % (H - S)] for b in range(B)], dtype=torch.int32, device="cuda")
    t["id_center"] = t["origin"].float() + S / 2.0
    t["id_scale"] = torch.full((B,), float(S), device="cuda")
    t["center"], t["scale"] = frontend.dzi_boxes(t["box"], (H, W))
    t["normals"] = frontend.depth_normals(t["depth"], t["K"])
    t["rgb_norm"] = ((t["rgb"].float() / 255.0 - torch.tensor(synthetic.COLOR_MEAN, device="cuda"))
                     / torch.tensor(synthetic.COLOR_STD_CROP, device="cuda")).permute(0, 3, 1, 2).contiguous()
    return t


def old_crop(t):
    """The crop part of frontend.make_inputs, as it does it."""
    depth, origin = t["depth"], t["origin"]
    xyz = frontend.depth_to_xyz(depth, t["K"], origin, S)
    ys = (origin[:, 1:2].long() + torch.arange(S, device=depth.device)[None]).clamp(0, depth.shape[1] - 1)
    xs = (origin[:, 0:1].long() + torch.arange(S, device=depth.device)[None]).clamp(0, depth.shape[2] - 1)
    bidx = torch.arange(B, device=depth.device)[:, None, None]
    rgb_c = t["rgb_norm"][bidx, :, ys[:, :, None], xs[:, None, :]].permute(0, 3, 1, 2).contiguous()
    nrm_c = t["normals"][bidx, :, ys[:, :, None], xs[:, None, :]].permute(0, 3, 1, 2).contiguous()
    msk = t["mask"][bidx, ys[:, :, None], xs[:, None, :]].reshape(B, S * S)
    return xyz, rgb_c, nrm_c, msk


def variants(t):
    return {
        "a_depth_normals": lambda: frontend.depth_normals(t["depth"], t["K"]),
        "b_crop_from_boxes": lambda: frontend.crop_from_boxes(t["rgb"], t["depth"], t["normals"], t["K"], t["center"], t["scale"], S,
                                                              mask=t["mask"]),
        "b_crop_from_boxes_identity": lambda: frontend.crop_from_boxes(t["rgb"], t["depth"], t["normals"], t["K"], t["id_center"],
                                                                       t["id_scale"], S, mask=t["mask"]),
        "c_make_inputs_from_boxes_no_pyramid": lambda: frontend.make_inputs_from_boxes(t["rgb"], t["depth"], t["K"], t["box"], S, N,
                                                                                       mask=t["mask"]),
        "d_make_inputs_no_pyramid": lambda: frontend.make_inputs(t["rgb_norm"], t["depth"], t["normals"], t["K"], t["origin"], S, N,
                                                                 mask=t["mask"]),
        "d_crop_part_of_make_inputs": lambda: old_crop(t),
    }


def timeit(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


class _NoPyramid:
    """Stubs pyramid.build_pyramid out of frontend for the timed calls."""

    def __enter__(self):
        self.saved = frontend.pyramid.build_pyramid
        frontend.pyramid.build_pyramid = lambda cld, xyz: {}

    def __exit__(self, *exc):
        frontend.pyramid.build_pyramid = self.saved


def measure(t, reps, rounds):
    fns = variants(t)
    with _NoPyramid():
        for fn in fns.values():                                            # warm up every shape
            for _ in range(5):
                fn()
        rows = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():                                      # alternating inside a round
                rows[k].append(timeit(fn, reps))

    def graph_normals_crop():
        n = frontend.depth_normals(t["depth"], t["K"])
        return frontend.crop_from_boxes(t["rgb"], t["depth"], n, t["K"], t["center"], t["scale"], S, mask=t["mask"])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graph_normals_crop()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = graph_normals_crop()
    g.replay()
    want = graph_normals_crop()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], want[k]) for k in want), "replay differs from eager"
    rows["a_plus_b_graph_replay"] = [timeit(g.replay, reps) for _ in range(rounds)]
    return rows


def kernel_stats(reps):
    """Re-run the eager (a) + (b) under rocprofv3 in a child process; -> {kernel: ms per call}."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--only-kernels", "--reps", str(reps)]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        rows = {}
        for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(fn)):
                if "depth_normals_kernel" in r["Name"] or "warp_crop_kernel" in r["Name"]:
                    key = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].strip()
                    calls = reps + (1 if "depth_normals" in key else 0)               # make() computes the normals once more
                    rows[key] = rows.get(key, 0.0) + float(r["TotalDurationNs"]) / 1e6 / calls
    return {k: round(v, 4) for k, v in sorted(rows.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--only-kernels", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_frontend needs the GPU"
    t = make()
    if a.only_kernels:
        for _ in range(a.reps):
            n = frontend.depth_normals(t["depth"], t["K"])
            frontend.crop_from_boxes(t["rgb"], t["depth"], n, t["K"], t["center"], t["scale"], S, mask=t["mask"])
        torch.cuda.synchronize()
        return
    rows = measure(t, a.reps, a.rounds)
    med = {k: float(np.median(v)) for k, v in rows.items()}
    spread = max(max(rows[k]) - min(rows[k]) for k in ("b_crop_from_boxes_identity", "d_crop_part_of_make_inputs"))
    res = dict(B=B, H=H, W=W, S=S, N=N, reps=a.reps, rounds=a.rounds,
               ms_per_batch={k: dict(median=round(med[k], 4), runs=[round(x, 4) for x in v]) for k, v in rows.items()},
               a_plus_b_ms=round(med["a_depth_normals"] + med["b_crop_from_boxes"], 4),
               a_plus_b_share_of_headline_step=round((med["a_depth_normals"] + med["b_crop_from_boxes"]) / HEADLINE_STEP_MS, 4),
               headline_step_ms=HEADLINE_STEP_MS,
               spread_ms=round(spread, 4),
               b_not_slower_than_crop_part_of_d=bool(med["b_crop_from_boxes_identity"] <= med["d_crop_part_of_make_inputs"] + spread),
               bytes_per_batch=dict(a_read=B * H * W * 4, a_write=B * 3 * H * W * 4, b_write=B * S * S * (12 + 12 + 12 + 4 + 1)),
               device=torch.cuda.get_device_name(0), torch=torch.__version__,
               note="device events around back-to-back eager calls, median of the rounds; the pyramid is stubbed out of (c) and (d)")
    if a.kernel_stats:
        res["kernel_ms_per_call"] = kernel_stats(a.reps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
