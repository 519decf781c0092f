#!/usr/bin/env python
"""Every 1x1 layer one training step of a model configuration reaches through ops.wx / ops.conv1x1_train / ops.conv1x1_train_w, with
its shapes and the engines ops.train_plan names for its three products (forward W.x, input gradient W^T.go, weight gradient go.x^T).

  python tools/list_train_products.py                      # the default LM-O training configuration; needs no GPU
  python tools/list_train_products.py --calls FILE          # another recorded list of calls
  python tools/list_train_products.py --record FILE [--batch 24 --npoints 4096 --mesh 4096]
                                                            # one training step on the GPU with the entry points noted -> FILE

The plan is computed from the shapes alone; only --record, which finds out WHICH shapes a configuration reaches, runs the model.
The default list, tests/golden/train_calls_lmo.json, is that record for batch 24, 4096 scene points, 4096 model vertices."""
import argparse
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import train_products as tp  # noqa: E402


def record(path, B, N, M):
    import torch
    from geometric_aware_dense_matching_amd import ops, synthetic, train_lm
    from geometric_aware_dense_matching_amd.config import make_model_cfg
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = GeoMatch(make_model_cfg(n_mesh_node=M, num_points=N), 1, model_points=synthetic.make_model_points(1, M))
    model = model.to(dev).train()
    ds = train_lm.SyntheticCrops(B, N, M, seed=0)
    batch = torch.utils.data.default_collate([ds[i] for i in range(B)])
    with tp.noting_entries(ops) as calls:
        out, _ = train_lm.model_fn_dec(model, batch, dev)
        out["loss"].backward()
    torch.cuda.synchronize()
    count = collections.Counter(tuple(c) for c in calls)
    with open(path, "w") as f:
        f.write('{"config": %s,\n"calls": [\n%s\n]}\n' % (json.dumps({"model": "geoMatch", "batch": B, "n_points": N, "n_model": M}),
                                                      ",\n".join(json.dumps(list(c) + [k]) for c, k in count.items())))


def table(doc):
    """Markdown rows, largest product first."""
    from geometric_aware_dense_matching_amd import ops
    lines = ["| entry | from | calls | B | Cin | Cout | n | bias | GFLOP | Function | forward | input gradient | weight gradient | fits |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    inherited = []
    for entry, B, cin, cout, n, bias, src, calls in sorted(doc["calls"], key=lambda c: -c[1] * c[2] * c[3] * c[4]):
        p = ops.train_plan(entry, B, cin, cout, n, cuda=True, bias_grad=bias)
        lines.append("| `%s` | %s | %d | %d | %d | %d | %d | %s | %.2f | `%s` | %s | %s | %s | %s |" % (
            entry, src, calls, B, cin, cout, n, "yes" if bias else "-", 2e-9 * B * n * cin * cout, p.function, p.fwd, p.dgrad,
            " > ".join(p.wgrad), "yes" if p.fits else "NO"))
        if not p.asks_mfma and "gemm_wgrad" in ops.train_plan("wx", B, cin, cout, n, cuda=True).wgrad:
            inherited.append((entry, src, B, cin, cout, n))
    return lines, inherited


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", default=os.path.join(tp.GOLDEN, "train_calls_lmo.json"))
    ap.add_argument("--record", metavar="FILE", default=None)
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--npoints", type=int, default=4096)
    ap.add_argument("--mesh", type=int, default=4096)
    args = ap.parse_args()
    if args.record:
        record(args.record, args.batch, args.npoints, args.mesh)
        args.calls = args.record
    with open(args.calls) as f:
        doc = json.load(f)
    lines, inherited = table(doc)
    print("1x1 training products of %s" % json.dumps(doc["config"]))
    print("\n".join(lines))
    print("\nLayers whose weight gradient `gemm_wgrad` would take through `ops.wx` but which go through `_Conv1x1Train` "
          "(the inherited asymmetry of ops.train_plan): %s" % (", ".join(map(str, inherited)) or "none"))


if __name__ == "__main__":
    main()
