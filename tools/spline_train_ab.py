"""The mesh branch's two training paths, `SplineCNN_Mesh.train_path = "dense"` (the [M, 125*C] table on the library GEMM, atomic
backward: the parent's code, untouched) and `"grouped"` (edge-grouped launches, gather-form backward), on the same commit.

    python tools/spline_train_ab.py measure [--B 24 --N 4096 --M 4096 --steps 20 --warmup 3 --rounds 3] --out ab.json
        TIMES only, both paths in ONE process, alternating per round: the whole GeoMatch training step (forward + losses + backward, no
        optimizer: it is the same for both) and the mesh branch alone (forward + backward of model.model_emb), device events around
        `steps` back-to-back runs.
    python tools/spline_train_ab.py peak --path grouped|dense --out peak_<path>.json
        MEMORY, one path COLD in a process of its own, so that everything the path brings -- pooled operand buffers, workspaces, the
        static maps -- is counted for it and for it alone: peak growth and what stays allocated over the first pass of the mesh branch,
        then torch.cuda.max_memory_allocated over two whole steps.
    rocprofv3 --kernel-trace --stats ... -- python tools/spline_train_ab.py profile --path grouped|dense
        the mesh branch alone on one path (forward + backward, warmup + 10 passes), for a kernel trace in a run of its own
    python tools/spline_train_ab.py report --json ab.json --peak-grouped .. --peak-dense .. --stats-grouped <kernel_stats.csv> --stats-dense <kernel_stats.csv> --out profiles/spline_train_grouped.md
        no GPU needed: writes the whole document from the files
"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PATHS = ("dense", "grouped")
PROFILE_PASSES = 10


def _setup(B, N, M, with_batch=True):
    import torch
    from geometric_aware_dense_matching_amd import synthetic, train_lm
    from geometric_aware_dense_matching_amd.config import make_model_cfg
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = GeoMatch(make_model_cfg(n_mesh_node=M, num_points=N), 1, model_points=synthetic.make_model_points(1, M)).to(dev).train()
    batch = None
    if with_batch:
        ds = train_lm.SyntheticCrops(B, N, M, seed=5)
        batch = torch.utils.data.default_collate([ds[i] for i in range(B)])
        batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    w = torch.randn(128, M, device=dev)

    def step(path):
        model.model_emb.train_path = path
        model.zero_grad(set_to_none=True)
        out, _ = train_lm.model_fn_dec(model, batch, dev)
        out["loss"].backward()
        return out["loss"].detach()

    def branch(path):
        model.model_emb.train_path = path
        model.model_emb.zero_grad(set_to_none=True)
        out = model.model_emb()
        (out * w).sum().backward()
        return out.detach()

    return torch, model, step, branch


def _timed(torch, fn, path, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn(path)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def measure(a):
    torch, model, step, branch = _setup(a.B, a.N, a.M)
    for _ in range(a.warmup):
        for path in PATHS:
            step(path)
            branch(path)
    torch.cuda.synchronize()
    pairs = model.model_emb._pairs
    res = {"B": a.B, "N": a.N, "M": a.M, "steps": a.steps, "warmup": a.warmup, "rounds": [], "device": torch.cuda.get_device_name(0),
           "pair_rows": int(pairs["rowidx"].shape[0]), "unique_pairs": int(pairs["blk_rows"].sum()), "largest_block": int(pairs["blk_rows"].max())}
    for r in range(a.rounds):
        row = {}
        for path in (PATHS if r % 2 == 0 else PATHS[::-1]):
            row["step_" + path] = _timed(torch, step, path, a.steps)
            row["branch_" + path] = _timed(torch, branch, path, a.steps)
        res["rounds"].append(row)
        print("round %d: step dense %.2f / grouped %.2f ms, mesh branch dense %.3f / grouped %.3f ms"
              % (r, row["step_dense"], row["step_grouped"], row["branch_dense"], row["branch_grouped"]), flush=True)
    res["ms"] = {k: statistics.median(r[k] for r in res["rounds"]) for k in res["rounds"][0]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("B", "N", "M", "ms")}))


def peak(a):
    """One path, cold: nothing of the other path has run in this process."""
    torch, model, step, branch = _setup(a.B, a.N, a.M)
    model.model_emb.train_path = a.path
    model.model_emb._ensure_graph()                             # the kNN graph and the forward bookkeeping: the same on both paths
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    branch(a.path)
    torch.cuda.synchronize()
    res = {"path": a.path, "B": a.B, "N": a.N, "M": a.M,
           "branch_peak_growth_mb": (torch.cuda.max_memory_allocated() - base) / 1e6}
    model.model_emb.zero_grad(set_to_none=True)
    res["branch_kept_mb"] = (torch.cuda.memory_allocated() - base) / 1e6      # pooled buffers, caches, maps: what stays after the pass
    torch.cuda.reset_peak_memory_stats()
    for _ in range(2):
        loss = step(a.path)
    torch.cuda.synchronize()
    res["step_max_allocated_mb"] = torch.cuda.max_memory_allocated() / 1e6
    res["loss"] = float(loss)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def profile(a):
    torch, model, step, branch = _setup(a.B, a.N, a.M, with_batch=False)
    for _ in range(a.warmup + PROFILE_PASSES):
        branch(a.path)
    torch.cuda.synchronize()


def _stats(path):
    rows = []
    if path:
        with open(path) as fh:
            for row in csv.DictReader(fh):
                rows.append((row["Name"], int(float(row["Calls"])), float(row["TotalDurationNs"])))
    rows.sort(key=lambda r: -r[2])
    return rows


def report(a):
    res = json.load(open(a.json))
    pk = {p: json.load(open(f)) for p, f in (("dense", a.peak_dense), ("grouped", a.peak_grouped)) if f}
    ms = res["ms"]
    spread = {k: max(r[k] for r in res["rounds"]) - min(r[k] for r in res["rounds"]) for k in ms}
    L = ["# Mesh branch: the grouped training path against the dense one", "",
         "`tools/spline_train_ab.py` on one %s, at the reference training shape: B = %d, N = %d scene points, M = %d model vertices" % (a.device or res["device"], res["B"], res["N"], res["M"]),
         "(%d pair rows with padding, %d unique (source, kernel index) pairs, largest kernel-index block %d rows; the dense table has %d rows)."
         % (res["pair_rows"], res["unique_pairs"], res["largest_block"], res["M"] * 125),
         "`train_path = \"dense\"` is the parent commit's code, untouched.  A step = forward + losses + backward of `GeoMatch` (no optimizer);",
         "the mesh branch = forward + backward of `model.model_emb` alone.", "",
         "## Time", "",
         "Both paths in ONE process, alternating per round; %d rounds of %d back-to-back runs between device events after %d warm-up runs of" % (len(res["rounds"]), res["steps"], res["warmup"]),
         "each; the median round counts.", "",
         "| | `dense` | `grouped` |", "|---|---|---|",
         "| training step, ms (spread over the rounds) | %.2f (%.2f) | %.2f (%.2f) |" % (ms["step_dense"], spread["step_dense"], ms["step_grouped"], spread["step_grouped"]),
         "| mesh branch alone, forward + backward, ms (spread) | %.3f (%.3f) | %.3f (%.3f) |" % (ms["branch_dense"], spread["branch_dense"], ms["branch_grouped"], spread["branch_grouped"]), "",
         "Rounds (ms, step dense / grouped, branch dense / grouped): " + "; ".join("%.2f / %.2f, %.3f / %.3f" % (r["step_dense"], r["step_grouped"], r["branch_dense"], r["branch_grouped"]) for r in res["rounds"]) + ".", ""]
    noise = max(spread["step_dense"], spread["step_grouped"])
    diff = ms["step_dense"] - ms["step_grouped"]
    L += [("The step on `grouped` is faster by %.2f ms, more than the spread of the rounds (%.2f ms)." % (diff, noise)) if diff > noise else
          ("The step on `grouped` is NOT faster (dense - grouped = %.2f ms against a spread of %.2f ms)." % (diff, noise)),
          "The default stays `dense` either way.", ""]
    if len(pk) == 2:
        L += ["## Memory", "",
              "Each path COLD in a process of its own (`peak --path ..`), so that what a path brings with it -- the pooled zero-bordered",
              "operand buffer of the packed pair gradient (3 (R + 2) x 512 B), the per-tile partials of the weight gradient, the inverse maps --",
              "is counted for that path and only for it.", "",
              "| | `dense` | `grouped` |", "|---|---|---|",
              "| peak growth over the first pass of the mesh branch, MB | %.0f | %.0f |" % (pk["dense"]["branch_peak_growth_mb"], pk["grouped"]["branch_peak_growth_mb"]),
              "| still allocated after that pass (pooled buffers, caches, maps), MB | %.0f | %.0f |" % (pk["dense"]["branch_kept_mb"], pk["grouped"]["branch_kept_mb"]),
              "| `torch.cuda.max_memory_allocated` over two whole steps, MB | %.0f | %.0f |" % (pk["dense"]["step_max_allocated_mb"], pk["grouped"]["step_max_allocated_mb"]),
              "| loss of the second step | %.6f | %.6f |" % (pk["dense"]["loss"], pk["grouped"]["loss"]), "",
              "The two losses come from different dropout draws (no common seed here; the tests compare the paths under one seed).", ""]
    for path, stats in (("grouped", a.stats_grouped), ("dense", a.stats_dense)):
        rows = _stats(stats)
        if not rows:
            continue
        npass = res["warmup"] + PROFILE_PASSES
        total = sum(r[2] for r in rows)
        L += ["## Kernels of the mesh branch on `%s` (`rocprofv3 --kernel-trace --stats`, a run of its own: %d forward + backward passes, set-up included)" % (path, npass), "",
              "| kernel | calls | total ms | ms per pass |", "|---|---|---|---|"]
        for name, calls, ns in rows[:a.top]:
            short = name.replace("(anonymous namespace)::", "")
            short = short[:short.index("(")] if "(" in short and not short.startswith("void at::") else short
            L.append("| `%s` | %d | %.3f | %.4f |" % (short[:110], calls, ns / 1e6, ns / 1e6 / npass))
        lib = sum(r[2] for r in rows if r[0].startswith("Cijk_"))
        L += ["", "All kernels of the run: %.2f ms over %d passes = %.3f ms of kernel time per pass (the graph's construction, once, included); "
              "of that, hipBLASLt (`Cijk_*`) kernels %.3f ms per pass." % (total / 1e6, npass, total / 1e6 / npass, lib / 1e6 / npass), ""]
    L += ["## Commands", "",
          "    python tools/spline_train_ab.py measure --out out/ab.json",
          "    python tools/spline_train_ab.py peak --path dense --out out/peak_dense.json",
          "    python tools/spline_train_ab.py peak --path grouped --out out/peak_grouped.json",
          "    rocprofv3 --kernel-trace --stats --output-format csv -d out/grouped -o g -- python tools/spline_train_ab.py profile --path grouped",
          "    rocprofv3 --kernel-trace --stats --output-format csv -d out/dense -o d -- python tools/spline_train_ab.py profile --path dense",
          "    python tools/spline_train_ab.py report --json out/ab.json --peak-dense out/peak_dense.json --peak-grouped out/peak_grouped.json \\",
          "        --stats-grouped <g_kernel_stats.csv> --stats-dense <d_kernel_stats.csv> --out profiles/spline_train_grouped.md", ""]
    with open(a.out, "w") as f:
        f.write("\n".join(L))
    print("\n".join(L))


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["measure", "peak", "profile", "report"])
    p.add_argument("--B", type=int, default=24)
    p.add_argument("--N", type=int, default=4096)
    p.add_argument("--M", type=int, default=4096)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--top", type=int, default=22)
    p.add_argument("--path", type=str, default="grouped", choices=PATHS)
    p.add_argument("--out", type=str, default="spline_train_ab.json")
    p.add_argument("--json", type=str, default="spline_train_ab.json")
    p.add_argument("--peak-grouped", dest="peak_grouped", type=str, default=None)
    p.add_argument("--peak-dense", dest="peak_dense", type=str, default=None)
    p.add_argument("--stats-grouped", dest="stats_grouped", type=str, default=None)
    p.add_argument("--stats-dense", dest="stats_dense", type=str, default=None)
    p.add_argument("--device", type=str, default=None, help="report: the device's name, if the runtime's own (recorded by `measure`) is generic")
    a = p.parse_args()
    {"measure": measure, "peak": peak, "profile": profile, "report": report}[a.mode](a)
