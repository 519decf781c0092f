"""Times the model-preparation kernels on the GPU (profiles/model_prep.md is written from its output):
  * farthest-point sampling, one launch per pick (ops.furthestsampling_wide) against one workgroup (ops.furthestsampling), at the
    pipeline's shape (n = 262144 candidates, m = 8192 picks) and at smaller n with m = n / 32, to place the crossover
    model_prep.FPS_WIDE_MIN_N; the two forms alternate inside one process and their picks are compared;
  * the wide form at n = 262144 for several workgroup counts;
  * surface sampling and the farthest pair on a sphere mesh of BOP size.
Every time is a host clock round work that ends in a device synchronise, after a warm-up of the same shape; the minimum and the median
of the repetitions are kept.  There is no GPU-less mode: without a device it fails.

    python tools/bench_model_prep.py [--out profiles/model_prep.json] [--reps 3] [--quick]
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geometric_aware_dense_matching_amd import model_prep, ops  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, {"min_ms": round(min(ts) * 1e3, 3), "median_ms": round(float(np.median(ts)) * 1e3, 3), "reps": reps}


def uv_sphere(rows, cols, radius=100.0):
    """A latitude / longitude sphere: rows * cols vertices, 2 * (rows - 1) * cols triangles (degenerate ones at the poles included)."""
    th = np.linspace(0.0, np.pi, rows)[:, None]
    ph = np.linspace(0.0, 2 * np.pi, cols, endpoint=False)[None, :]
    unit = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th) * np.ones_like(ph)], axis=-1).reshape(-1, 3)
    r, c = np.meshgrid(np.arange(rows - 1), np.arange(cols), indexing="ij")
    a, b = r * cols + c, r * cols + (c + 1) % cols
    faces = np.concatenate([np.stack([a, a + cols, b], -1).reshape(-1, 3), np.stack([b, a + cols, b + cols], -1).reshape(-1, 3)])
    return unit * radius, faces.astype(np.int32), unit.astype(np.float32)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--quick", action="store_true", help="small shapes only (a rehearsal of the script, not a measurement)")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_model_prep.py measures on the GPU and found none")
    res = {"device": torch.cuda.get_device_name(0), "fps": [], "fps_groups": [], "kernels": []}
    shapes = [(1024, 32), (4096, 128)] if args.quick else \
        [(1024, 32), (2048, 64), (4096, 128), (8192, 256), (16384, 512), (32768, 1024), (65536, 2048), (262144, 8192)]
    for n, m in shapes:
        xyz = torch.from_numpy(np.random.default_rng(zlib.crc32(b"fps %d" % n)).standard_normal((1, n, 3)).astype(np.float32)).cuda()
        rows = {}
        for _ in range(2):                                                 # alternate the two forms
            for name, fn in (("one_workgroup", lambda: ops.furthestsampling(xyz, m)), ("wide", lambda: ops.furthestsampling_wide(xyz, m))):
                out, t = timed(fn, args.reps)
                rows.setdefault(name, []).append((out, t))
        same = all(torch.equal(o, rows["wide"][0][0]) for name in rows for o, _ in rows[name])
        row = {"n": n, "m": m, "groups": int(ops.call("gdm_fps_wide_groups", n)), "same_picks": bool(same)}
        for name in rows:
            best = min(t["min_ms"] for _, t in rows[name])
            row[name] = {"min_ms": best, "median_ms": [t["median_ms"] for _, t in rows[name]], "us_per_pick": round(best * 1e3 / m, 3)}
        res["fps"].append(row)
        print(json.dumps(row), flush=True)
    if not args.quick:
        n, m = 262144, 2048
        xyz = torch.from_numpy(np.random.default_rng(zlib.crc32(b"fps groups")).standard_normal((1, n, 3)).astype(np.float32)).cuda()
        for groups in (64, 128, 256, 512, 1024):
            _, t = timed(lambda: ops.furthestsampling_wide(xyz, m, groups), args.reps)
            row = {"n": n, "m": m, "groups": groups, "min_ms": t["min_ms"], "us_per_pick": round(t["min_ms"] * 1e3 / m, 3)}
            res["fps_groups"].append(row)
            print(json.dumps(row), flush=True)
    rows_, cols_ = (64, 128) if args.quick else (256, 512)
    verts, faces, normals = uv_sphere(rows_, cols_)
    colors = np.clip(np.rint(normals * 127 + 128), 0, 255).astype(np.float32)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (verts.astype(np.float32), faces, normals, colors,
                                                                       model_prep.face_cdf(verts, faces))]
    S = 8192 if args.quick else 262144
    _, t = timed(lambda: ops.surface_sample(*dev, S, 0), args.reps)
    row = {"kernel": "surface_sample (with the wrapper's checks of faces and cdf)", "V": len(verts), "F": len(faces), "S": S, **t}
    res["kernels"].append(row)
    print(json.dumps(row), flush=True)
    out = torch.empty((S, 9), dtype=torch.float32, device="cuda")
    _, t = timed(lambda: ops.call("gdm_surface_sample_hip", *dev, len(verts), len(faces), S, 0, out), args.reps)
    row = {"kernel": "gdm_surface_sample_hip alone", "V": len(verts), "F": len(faces), "S": S, **t}
    res["kernels"].append(row)
    print(json.dumps(row), flush=True)
    _, t = timed(lambda: ops.point_diameter(dev[0]), args.reps)
    pairs = len(verts) * (len(verts) - 1) // 2
    row = {"kernel": "point_diameter", "V": len(verts), "pairs": pairs, **t, "gpairs_per_s": round(pairs / t["min_ms"] / 1e6, 2)}
    res["kernels"].append(row)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
