#!/usr/bin/env python3
"""Times the BOP pose-error kernels (gdm_bop.hip) on an LM-sized case and, beside each, a chunked torch composition of the
reference's formulas (lib/pysixd/pose_error.py:84-179) on the same card with its peak memory -- the yardstick, since nothing older
computes these errors.  Meant to be run once plainly (device-event times, one JSON line) and once under
`rocprofv3 --kernel-trace --stats -- python tools/bop_errors_profile.py --iters 5` (kernel times); profiles/bop_errors.md holds both.

  MSSD / MSPD   n = 16 instances, M = 8192 model points, S = 314 symmetries (one continuous axis at max_sym_disc_step = 0.01)
  render + VSD  n = 16, 640 x 480, the squashed icosphere of the tests at 5 subdivisions (20480 faces), both poses rendered and scored
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import bop_inputs as bi  # noqa: E402
from geometric_aware_dense_matching_amd import evaluation as ev  # noqa: E402

LM_K = bi.LM_K
H, W = 480, 640


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b) / iters, torch.cuda.max_memory_allocated() - base


def torch_mssd_mspd(RT_est, RT_gt, pts, sym_R, sym_t, K, chunk=16):
    """The reference's formulas as batched fp64 torch operations, `chunk` symmetries at a time ([n, chunk, M, 3] temporaries)."""
    def project(X):
        h = X @ K.T
        return h[..., :2] / h[..., 2:3]
    pe = pts @ RT_est[:, :, :3].transpose(1, 2) + RT_est[:, None, :, 3]                      # [n, M, 3]
    ue = project(pe)
    e3, e2 = [], []
    for s0 in range(0, sym_R.shape[0], chunk):
        Rs = torch.einsum("nij,sjk->nsik", RT_gt[:, :, :3], sym_R[s0:s0 + chunk])
        ts = torch.einsum("nij,sj->nsi", RT_gt[:, :, :3], sym_t[s0:s0 + chunk]) + RT_gt[:, None, :, 3]
        pg = torch.einsum("nsij,mj->nsmi", Rs, pts) + ts[:, :, None, :]
        e3.append((pe[:, None] - pg).norm(dim=3).amax(dim=2))
        e2.append((ue[:, None] - project(pg)).norm(dim=3).amax(dim=2))
    e3, e2 = torch.cat(e3, dim=1), torch.cat(e2, dim=1)
    return e3.amin(dim=1), e2.amin(dim=1)


def torch_vsd(d_est, d_gt, d_test, K, delta, taus, diameter):
    ys, xs = torch.meshgrid(torch.arange(H, device=d_est.device, dtype=torch.float64),
                            torch.arange(W, device=d_est.device, dtype=torch.float64), indexing="ij")
    px, py = (xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1]

    def dist(d):
        d = d.double()
        return torch.sqrt((px * d) ** 2 + (py * d) ** 2 + d ** 2)
    dt, dg, de = dist(d_test), dist(d_gt), dist(d_est)

    def vis(dm):
        return ((dm.float() - dt.float() <= delta) | (dt == 0)) & (dm > 0)
    vg = vis(dg)
    ve = vis(de) | (vg & (de > 0))
    inter, union = vg & ve, vg | ve
    cost = (dg - de).abs() / diameter
    u = union.sum(dim=(1, 2)).double()
    comp = u - inter.sum(dim=(1, 2)).double()
    errs = [((inter & (cost >= t)).sum(dim=(1, 2)).double() + comp) / u for t in taus]
    return torch.where(u[:, None] > 0, torch.stack(errs, dim=1), torch.ones((), dtype=torch.float64, device=u.device))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch compositions (a cleaner kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
    dev = torch.device("cuda:0")
    n = args.n
    res = {"n": n}

    # MSSD / MSPD
    pts, _, _ = bi.mssd_inputs(M=8192, n=1, seed=3)
    rs = np.random.RandomState(0)
    RT_gt = np.stack([np.hstack([bi.rot(rs.rand() * 3, rs.randn(3)), np.array([[0.05 * rs.randn()], [0.05 * rs.randn()], [0.8]])])
                      for _ in range(n)])
    RT_est = RT_gt.copy()
    for i in range(n):
        RT_est[i, :, :3] = bi.rot(0.1, rs.randn(3)) @ RT_gt[i, :, :3]
        RT_est[i, :, 3] += 0.005 * rs.randn(3)
    sym_R, sym_t = ev.symmetry_transformations(bi.MODEL_INFOS["continuous"], 0.01, scale=0.001)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (RT_est, RT_gt, pts, sym_R, sym_t, LM_K)]
    out, ms, mem = timed(lambda: ev.mssd_mspd(*d), args.iters)
    res["mssd_mspd"] = dict(M=8192, S=int(sym_R.shape[0]), hip_ms=round(ms, 4), hip_peak_bytes=int(mem))
    if not args.no_torch:
        tout, tms, tmem = timed(lambda: torch_mssd_mspd(*d), max(2, args.iters // 4))
        res["mssd_mspd"].update(torch_ms=round(tms, 4), torch_peak_bytes=int(tmem), torch_chunk=16,
                                max_rel_diff=float(max(((out[0] - tout[0]).abs() / tout[0]).max(), ((out[1] - tout[1]).abs() / tout[1]).max())))

    # render both poses + VSD
    verts, faces = bi.icosphere(5, 0.05)
    verts = verts * np.array([1.6, 1.0, 0.7])
    diam = 0.16
    g = np.stack([np.hstack([bi.rot(0.7 + 0.1 * i, (1, 2, 3)), np.array([[0.01 * (i % 4)], [-0.005], [0.6 + 0.02 * i]])]) for i in range(n)])
    e = g.copy()
    for i in range(n):
        e[i, :, :3] = bi.rot(0.08, rs.randn(3)) @ g[i, :, :3]
        e[i, :, 3] += 0.004 * rs.randn(3)
    vd, fd, gd, ed, Kd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (verts, faces, g, e, LM_K))
    d_gt = ev.render_depth(vd, fd, gd, Kd, H, W, 0.01)
    d_test = torch.where(d_gt > 0, d_gt + 0.003, torch.full_like(d_gt, 1.5))
    taus = bi.TAUS
    _, ms_r, mem_r = timed(lambda: ev.render_depth(vd, fd, torch.cat([ed, gd]), Kd, H, W, 0.01), args.iters)
    d_est = ev.render_depth(vd, fd, ed, Kd, H, W, 0.01)
    verr, ms_v, mem_v = timed(lambda: ev.vsd(d_est, d_gt, d_test, Kd, 0.015, taus, diameter=diam), args.iters)
    ferr, ms_f, mem_f = timed(lambda: ev.vsd_from_poses(vd, fd, ed, gd, d_test, Kd, 0.015, taus, diameter=diam, near=0.01), args.iters)
    res["render_vsd"] = dict(H=H, W=W, faces=int(faces.shape[0]), covered_px_per_image=int((d_gt > 0).sum() // n),
                             render_2n_ms=round(ms_r, 4), render_peak_bytes=int(mem_r), vsd_ms=round(ms_v, 4), vsd_peak_bytes=int(mem_v),
                             vsd_from_poses_ms=round(ms_f, 4), vsd_from_poses_peak_bytes=int(mem_f),
                             from_poses_equals_given_images=bool(torch.equal(verr, ferr)))
    if not args.no_torch:
        terr, tms, tmem = timed(lambda: torch_vsd(d_est, d_gt, d_test, Kd, 0.015, taus, diam), max(2, args.iters // 4))
        res["render_vsd"].update(torch_vsd_ms=round(tms, 4), torch_vsd_peak_bytes=int(tmem), vsd_equal_torch=bool(torch.equal(verr, terr)),
                                 note="the render has no torch counterpart")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
