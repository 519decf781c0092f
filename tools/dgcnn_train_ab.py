"""One training step of the DGCNN variant on its two training paths, `train_path = "modules"` (dense distances, library convolutions
on edge tensors: the parent's code, untouched) and `train_path = "fused"` (feature-space kNN, ops.edge_block_train), on the same commit.

    python tools/dgcnn_train_ab.py measure [--B 24 --N 4096 --M 4096 --steps 20 --warmup 3 --rounds 3] --out ab.json
        times both paths in ONE process, alternating per round (device events around `steps` back-to-back steps, every shape warmed
        up first), and takes each path's peak-memory growth over one step.  A step = forward + losses + backward (no optimizer: it is
        the same for both).  If the module path does not fit at B, B is halved until it does; the B used is recorded.
    rocprofv3 --kernel-trace --stats ... -- python tools/dgcnn_train_ab.py profile [--B ..]
        the fused step alone, for a kernel trace in a run of its own
    python tools/dgcnn_train_ab.py report --json ab.json --stats <kernel_stats.csv> --out profiles/dgcnn_train_fused.md
        no GPU needed: writes the document from the two files
"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _setup(B, N, M):
    import torch
    from geometric_aware_dense_matching_amd import synthetic, train_lm
    from geometric_aware_dense_matching_amd.config import make_dgcnn_cfg
    from geometric_aware_dense_matching_amd.geoMatch_DGCNN import GeoMatch
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = GeoMatch(make_dgcnn_cfg(n_mesh_node=M, dataset="ycbv"), 2, model_points=synthetic.make_model_points(2, M, 269.573)).to(dev).train()
    model.model_emb.k = 20                                      # the reference's mesh trunk
    ds = train_lm.SyntheticCrops(B, N, M, seed=5)
    batch = torch.utils.data.default_collate([ds[i] for i in range(B)])
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def step(path):
        model.train_path = path
        model.zero_grad(set_to_none=True)
        out, _ = train_lm.model_fn_dec(model, batch, dev)
        out["loss"].backward()
        return out["loss"].detach()

    return torch, model, step


def measure(a):
    import torch
    B = a.B
    while True:
        try:
            torch_, model, step = _setup(B, a.N, a.M)
            for _ in range(a.warmup):
                for path in ("modules", "fused"):
                    loss = step(path)
            torch.cuda.synchronize()
            break
        except torch.cuda.OutOfMemoryError:
            if B <= 1:
                raise
            del model, step
            torch.cuda.empty_cache()
            B //= 2
    res = {"B": B, "B_asked": a.B, "N": a.N, "M": a.M, "k": [16, 20], "steps": a.steps, "warmup": a.warmup, "rounds": [], "peak_mb": {},
           "loss": {}, "device": torch.cuda.get_device_name(0)}
    for path in ("modules", "fused"):
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res["loss"][path] = float(step(path))
        torch.cuda.synchronize()
        res["peak_mb"][path] = (torch.cuda.max_memory_allocated() - base) / 1e6
    for r in range(a.rounds):
        row = {}
        for path in (("modules", "fused") if r % 2 == 0 else ("fused", "modules")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step(path)
            e1.record()
            torch.cuda.synchronize()
            row[path] = e0.elapsed_time(e1) / a.steps
        res["rounds"].append(row)
        print("round %d: modules %.2f ms, fused %.2f ms per step" % (r, row["modules"], row["fused"]), flush=True)
    res["ms"] = {p: statistics.median(r[p] for r in res["rounds"]) for p in ("modules", "fused")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("B", "N", "M", "ms", "peak_mb", "loss")}))


def profile(a):
    torch, model, step = _setup(a.B, a.N, a.M)
    for _ in range(a.warmup + 5):
        step("fused")
    torch.cuda.synchronize()


def report(a):
    res = json.load(open(a.json))
    rows = []
    if a.stats:
        with open(a.stats) as fh:
            for row in csv.DictReader(fh):
                rows.append((row["Name"], int(float(row["Calls"])), float(row["TotalDurationNs"]), float(row["Percentage"])))
    rows.sort(key=lambda r: -r[2])
    ms, pk = res["ms"], res["peak_mb"]
    spread = {p: max(r[p] for r in res["rounds"]) - min(r[p] for r in res["rounds"]) for p in ms}
    faster = ms["fused"] < ms["modules"]
    L = ["# DGCNN variant: the fused training path against the module path", "",
         "`tools/dgcnn_train_ab.py` on one %s: one training step (forward of both trunks + heads + losses + backward, no optimizer) at" % (a.device or res["device"]),
         "B = %d%s, N = %d scene points, M = %d model vertices, k = 16 (cloud) / 20 (mesh).  Both paths in ONE process on the same commit,"
         % (res["B"], "" if res["B"] == res["B_asked"] else " (B = %d asked; halved until the module path fit)" % res["B_asked"], res["N"], res["M"]),
         "alternating per round; %d rounds of %d back-to-back steps between device events after %d warm-up steps of each path; the median" % (len(res["rounds"]), res["steps"], res["warmup"]),
         "round counts.", "",
         "| path | ms / step | spread over the rounds | peak growth over one step |", "|---|---|---|---|",
         "| `train_path = \"modules\"` (dense distances, library convolutions on edge tensors) | %.2f | %.2f | %.0f MB |" % (ms["modules"], spread["modules"], pk["modules"]),
         "| `train_path = \"fused\"` (`feature_knn`, `edge_block_train`, split conv7) | %.2f | %.2f | %.0f MB |" % (ms["fused"], spread["fused"], pk["fused"]), "",
         "Rounds (ms): " + "; ".join("modules %.2f / fused %.2f" % (r["modules"], r["fused"]) for r in res["rounds"]) + ".", "",
         ("The fused step is %.2fx faster and its peak is %.2fx smaller." % (ms["modules"] / ms["fused"], pk["modules"] / pk["fused"])) if faster else
         ("The fused step is NOT faster: %.2fx the module path's time.  Its peak is %.2fx smaller; the path is kept for its memory."
          % (ms["fused"] / ms["modules"], pk["modules"] / pk["fused"])),
         "Loss of the measured step: modules %.6f, fused %.6f (the graphs of the two paths differ at fp32 near-ties of the kNN)." % (res["loss"]["modules"], res["loss"]["fused"]), ""]
    if rows:
        total = sum(r[2] for r in rows)
        nsteps = res["warmup"] + 5
        L += ["## Kernels of the fused step (`rocprofv3 --kernel-trace --stats`, a run of its own: %d fused steps, set-up included)" % nsteps, "",
              "| kernel | calls | total ms | share |", "|---|---|---|---|"]
        for name, calls, ns, pct in rows[:a.top]:
            short = name.replace("(anonymous namespace)::", "")
            short = short[:short.index("(")] if "(" in short and not short.startswith("void at::") else short[:100]
            L.append("| `%s` | %d | %.2f | %.1f %% |" % (short[:100], calls, ns / 1e6, 100.0 * ns / total))
        L += ["", "All kernels of the run: %.1f ms over %d steps = %.2f ms of kernel time per step." % (total / 1e6, nsteps, total / 1e6 / nsteps), ""]
    with open(a.out, "w") as f:
        f.write("\n".join(L))
    print("\n".join(L))


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["measure", "profile", "report"])
    p.add_argument("--B", type=int, default=24)
    p.add_argument("--N", type=int, default=4096)
    p.add_argument("--M", type=int, default=4096)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--top", type=int, default=25)
    p.add_argument("--out", type=str, default="dgcnn_train_ab.json")
    p.add_argument("--json", type=str, default="dgcnn_train_ab.json")
    p.add_argument("--stats", type=str, default=None)
    p.add_argument("--device", type=str, default=None, help="report: the device's name, if the runtime's own (recorded by `measure`) is generic")
    a = p.parse_args()
    {"measure": measure, "profile": profile, "report": report}[a.mode](a)
