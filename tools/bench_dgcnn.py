"""geoMatch_DGCNN variant (BASELINE config 4): the default eval forward + matching against the fused inference path, in ONE run.

Forms, timed alternately (round-robin, `--rounds` rounds of `--steps` steps each, every form warmed up first; the median round counts):
  parent_a / parent_b   model(inputs) + matching.match_frames, eager: the default forward (dense [B,n,n] distances, library GEMMs).
                        Timed twice per round: the difference between the two is the run-to-run spread of this run
  fused_eager           infer.pipeline_step(model, inputs, with_pose=False): the fused trunks + the same matching, eager
  fused_graph           the same step as one hipGraph replay (infer.GraphedPipeline)
and the graph construction alone, `dgcnn.knn` (GEMM + top-k over [B,n,n]) against `ops.feature_knn`, at (B16, C64, n2048, k16) and
(B1, C64, n8192, k20).  Peak memory per form is the growth of torch.cuda.max_memory_allocated over one step after warm-up; for the
graph, whose replay allocates nothing, over building the pipeline, and what the kept capture goes on holding.
`--profile` adds the fused eager step's kernels (torch profiler) and the share of its kernel time and launches that is not this
package's HIP code.  `--only-fused N` runs N fused eager steps and nothing else (the body for `rocprofv3 --kernel-trace --stats`).
Prints one JSON line last.  Development aid."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from geometric_aware_dense_matching_amd import dgcnn, infer, matching, ops, synthetic  # noqa: E402
from geometric_aware_dense_matching_amd.geoMatch_DGCNN import GeoMatch  # noqa: E402


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def alternate(forms, rounds, steps, warmup):
    """{name: [ms per round]}: every form warmed up, then `rounds` passes over all forms in order."""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(rounds):
        for name, fn in forms.items():
            ms[name].append(timed(fn, steps))
    return ms


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 1e6, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--mesh", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--only-fused", type=int, default=0)
    args = ap.parse_args()
    B, N, M = args.batch, args.points, args.mesh
    model = GeoMatch(dict(feat_dim=128, k=16, embed_dim=1024, dropout=0.1, n_mesh_node=M), 1,
                     model_points=synthetic.make_model_points(1, M)).cuda().eval()
    batch = synthetic.make_batch(seed=1, batch=B, n_points=N)
    inp = {"cld_rgb_nrm": torch.from_numpy(batch["cld_rgb_nrm"]).cuda()}

    def parent():
        with torch.no_grad():
            return matching.match_frames(model(inp))

    def fused_eager():
        with torch.no_grad():
            return infer.pipeline_step(model, inp, with_pose=False)

    if args.only_fused:
        for _ in range(args.only_fused):
            fused_eager()
        torch.cuda.synchronize()
        return
    out = {"batch": B, "points": N, "mesh": M, "rounds": args.rounds, "steps": args.steps}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    gp = infer.GraphedPipeline(model, inp, with_pose=False)
    gp(inp)
    torch.cuda.synchronize()
    # the replay allocates nothing: its memory is the capture's private pool, so the figure is what building the pipeline (warm-up, the
    # candidate forms) peaked at, and what the kept form goes on holding
    graph_peak, graph_held = torch.cuda.max_memory_allocated() - held, torch.cuda.memory_allocated() - held
    out["graph_form"] = gp.form
    forms = {"parent_a": parent, "fused_eager": fused_eager, "fused_graph": lambda: gp(inp), "parent_b": parent}
    ms = alternate(forms, args.rounds, args.steps, args.warmup)
    out["step"] = {name: {"ms": round(statistics.median(v), 3), "crops_per_s": round(B / statistics.median(v) * 1e3, 1),
                          "rounds_ms": [round(t, 3) for t in v]} for name, v in ms.items()}
    out["peak_mb"] = {"parent": peak_mb(parent), "fused_eager": peak_mb(fused_eager), "fused_graph_build": round(graph_peak / 1e6, 1),
                      "fused_graph_held": round(graph_held / 1e6, 1)}
    out["knn"] = {}
    for (b, c, n, k) in ((16, 64, 2048, 16), (1, 64, 8192, 20)):
        x = torch.nn.functional.leaky_relu(torch.randn(b, c, n, generator=torch.Generator().manual_seed(n)), 0.2).cuda()
        kms = alternate({"parent_a": lambda: dgcnn.knn(x, k), "feature_knn": lambda: ops.feature_knn(x, k), "parent_b": lambda: dgcnn.knn(x, k)},
                        args.rounds, 20, args.warmup)
        out["knn"]["B%d_C%d_n%d_k%d" % (b, c, n, k)] = dict(
            {name: {"ms": round(statistics.median(v), 4), "rounds_ms": [round(t, 4) for t in v]} for name, v in kms.items()},
            peak_mb={"parent": peak_mb(lambda: dgcnn.knn(x, k)), "feature_knn": peak_mb(lambda: ops.feature_knn(x, k))})
    if args.profile:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fused_eager()
            torch.cuda.synchronize()
        rows = sorted(((getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0), e.key, e.count)
                       for e in prof.key_averages()), reverse=True)
        rows = [r for r in rows if r[0] > 0]
        own = lambda name: "anonymous namespace" in name or "_GLOBAL__N_" in name       # this package's kernels live in unnamed namespaces
        total_t, total_n = sum(r[0] for r in rows), sum(r[2] for r in rows)
        lib = [r for r in rows if not own(r[1])]
        out["fused_eager_profile"] = {"kernel_us": round(total_t, 1), "launches": total_n,
                                      "library_share_of_time": round(sum(r[0] for r in lib) / max(total_t, 1e-9), 4),
                                      "library_share_of_launches": round(sum(r[2] for r in lib) / max(total_n, 1), 4),
                                      "library_kernels": [[round(t, 1), c, k[:90]] for t, k, c in lib]}
        for t, k, c in rows[:16]:
            print("%9.1f us  x%-3d %s" % (t, c, k[:120]))
    for name, v in out["step"].items():
        print("%-12s %8.3f ms/step  %8.1f crops/s" % (name, v["ms"], v["crops_per_s"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
