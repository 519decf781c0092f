"""Timing of the hash-sampled item and of the graphed frames-to-poses pipeline at B = 16 and B = 1, 480x640 frames,
S = 256, N = 2048, headline model (M = 8192):
  (a) make_inputs_from_boxes without the pyramid, sampler="torch"   -- tools/bench_frontend.py leg (c), the path this replaces
  (b) the same with sampler="hash"
  (c) a frame to a pose the way it went before: eager make_inputs_from_boxes (sampler="torch", no pyramid, so that none is built
      twice) followed by one infer.GraphedPipeline call on rgb / cld_rgb_nrm / choose / dpt_xyz
  (d) one infer.GraphedFramePipeline call on the frame buffers
Method as in tools/bench_frontend.py: synthetic.make_frame frames with synthetic.make_box_mask detections, device events around
`--reps` back-to-back calls after a warm-up, `--rounds` repeated measurements, the legs alternating inside a round, the median of
the rounds.  With --kernel-stats the eager (b) runs again in a child process under `rocprofv3 --kernel-trace --stats` and the
sampling kernel's time per call is added.
    python tools/bench_frames.py [--reps 200] [--rounds 3] [--kernel-stats] [--out profiles/frames_bench.json]"""
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

from geometric_aware_dense_matching_amd import frontend, infer, synthetic  # noqa: E402
from geometric_aware_dense_matching_amd.config import make_model_cfg  # noqa: E402

H, W, S, N, M = 480, 640, 256, 2048, 8192
KEYS = ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")


def make_frames(B, seed=0):
    rs = np.random.RandomState(seed)
    fr = [synthetic.make_frame(rs) for _ in range(B)]
    det = [synthetic.make_box_mask(rs) for _ in range(B)]
    t = dict(depth=np.stack([f[0] for f in fr]), rgb_u8=np.stack([f[1] for f in fr]), mask=np.stack([d[1] for d in det]),
             bbox_xyxy=np.stack([d[0] for d in det]), K=np.stack([synthetic.LM_K] * B))
    return {k: torch.from_numpy(v).cuda() for k, v in t.items()}


def make_model():
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    model = GeoMatch(make_model_cfg(n_mesh_node=M, num_points=N), 1, model_points=synthetic.make_model_points(1, M))
    sd = synthetic.synthetic_state_dict({k: v for k, v in model.state_dict().items() if not k.startswith("model_emb.mesh_graph")
                                         and k not in ("model_emb.xyz", "model_emb.const_one")}, seed=0)
    model.load_state_dict(sd, strict=False)
    return model.cuda().eval()


def item(f, sampler):
    return frontend.make_inputs_from_boxes(f["rgb_u8"], f["depth"], f["K"], f["bbox_xyxy"], S, N, mask=f["mask"], sampler=sampler,
                                           build_pyramid=False)


def timeit(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def measure(model, B, reps, rounds):
    f = make_frames(B)
    with torch.no_grad():
        gp = infer.GraphedPipeline(model, {k: item(f, "torch")[k] for k in KEYS})
        gf = infer.GraphedFramePipeline(model, f, S, N)

        def parent_way():
            d = item(f, "torch")
            return gp({k: d[k] for k in KEYS})

        fns = {"a_item_torch_sampler": lambda: item(f, "torch"), "b_item_hash_sampler": lambda: item(f, "hash"),
               "c_eager_item_then_graphed_pipeline": parent_way, "d_graphed_frame_pipeline": lambda: gf(f)}
        for fn in fns.values():
            for _ in range(5):
                fn()
        rows = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():                                      # alternating inside a round
                rows[k].append(timeit(fn, reps))
    med = {k: float(np.median(v)) for k, v in rows.items()}
    spread = {k: max(v) - min(v) for k, v in rows.items()}
    res = dict(ms_per_batch={k: dict(median=round(med[k], 4), runs=[round(x, 4) for x in v]) for k, v in rows.items()},
               forms=dict(graphed_pipeline=gp.form, graphed_frame_pipeline=gf.form),
               b_beats_a_by_more_than_the_spread=bool(med["a_item_torch_sampler"] - med["b_item_hash_sampler"]
                                                      > max(spread["a_item_torch_sampler"], spread["b_item_hash_sampler"])),
               d_beats_c_by_more_than_the_spread=bool(med["c_eager_item_then_graphed_pipeline"] - med["d_graphed_frame_pipeline"]
                                                      > max(spread["c_eager_item_then_graphed_pipeline"],
                                                            spread["d_graphed_frame_pipeline"])))
    del gp, gf
    return res


def kernel_stats(reps):
    """Re-run the eager (b) at B = 16 under rocprofv3 in a child process; -> {kernel: ms per call} of the front end's own kernels."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--only-kernels", "--reps", str(reps)]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        rows = {}
        for fn in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(fn)):
                if any(s in r["Name"] for s in ("sample_assemble_kernel", "depth_normals_kernel", "warp_crop_kernel")):
                    key = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].strip()
                    rows[key] = rows.get(key, 0.0) + float(r["TotalDurationNs"]) / 1e6 / int(r.get("Calls") or reps)
    return {k: round(v, 4) for k, v in sorted(rows.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--only-kernels", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_frames needs the GPU"
    if a.only_kernels:
        f = make_frames(16)
        for _ in range(a.reps):
            item(f, "hash")
        torch.cuda.synchronize()
        return
    model = make_model()
    res = dict(H=H, W=W, S=S, N=N, M=M, reps=a.reps, rounds=a.rounds, B16=measure(model, 16, a.reps, a.rounds),
               B1=measure(model, 1, a.reps, a.rounds), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               note="device events around back-to-back calls, median of the rounds; (a), (b) and the eager part of (c) build no pyramid")
    if a.kernel_stats:
        res["kernel_ms_per_call_B16"] = kernel_stats(a.reps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
