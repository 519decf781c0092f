"""The soft-assignment training operator on the MI355X, written to profiles/soft_coord.md (run once):
  * device-event times of the forward, grad x and grad y launches of csrc/gdm_softcoord.hip at R = 49152, M = 4096 and R = 32768,
    M = 8192, the two packs the operator repeats, and the operator end to end (forward + backward through autograd);
  * in the same run: ops.circle_match forward + backward, and loss.soft_coord_reference (the [R, M] similarity materialised) under
    autograd, each with its peak memory;
  * the training step at B = 24, N = M = 4096 with both losses on against both weights 0 (the step as it was), alternating;
  * the measured maxima of the error quantities tests/test_gpu_soft_coord.py bounds, over its shapes, temperatures and families.
    python tools/soft_coord_profile.py [--out profiles/soft_coord.md] [--no-step]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from geometric_aware_dense_matching_amd import _lib, loss, ops


def timed(fn, reps=20, warm=3):
    """Median device-event time (ms) of fn over `reps` calls after `warm` warm-up calls."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def peak_of(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def kernel_times(R, M, gamma, lines):
    dev = torch.device("cuda")
    L = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(R + M)
    x0 = torch.nn.functional.normalize(torch.randn(R, 128, device=dev, generator=g), dim=1)
    y0 = torch.nn.functional.normalize(torch.randn(M, 128, device=dev, generator=g), dim=1)
    xyz = torch.rand(M, 3, device=dev, generator=g) * 0.2 - 0.1
    a, b = torch.randn(R, device=dev, generator=g), torch.randn(R, 3, device=dev, generator=g)
    st = lambda: torch.cuda.current_stream().cuda_stream
    xr, xt, _ = ops._cm_pack(x0)
    yr, yt, _ = ops._cm_pack(y0)
    lse, soft = torch.empty(R, device=dev), torch.empty(R, 3, device=dev)
    P, Mp = L.gdm_soft_coord_bwd_parts(R, M), (M + 127) // 128 * 128
    gx, gy, part = torch.empty(R, 128, device=dev), torch.empty(M, 128, device=dev), torch.empty(P, Mp, 128, device=dev)
    args = (xr.data_ptr(), xt.data_ptr(), yr.data_ptr(), yt.data_ptr(), xyz.data_ptr(), R, M, gamma)
    fwd = lambda: ops.check(L.gdm_soft_coord_fwd_hip(*args, lse.data_ptr(), soft.data_ptr(), st()), "fwd")
    fwd()
    kb = torch.cat([(a - (b * soft).sum(1)).unsqueeze(1), b], dim=1).contiguous()
    bx = lambda: ops.check(L.gdm_soft_coord_bwd_hip(*args, lse.data_ptr(), kb.data_ptr(), gx.data_ptr(), None, None, st()), "gx")
    by = lambda: ops.check(L.gdm_soft_coord_bwd_hip(*args, lse.data_ptr(), kb.data_ptr(), None, part.data_ptr(), gy.data_ptr(), st()), "gy")
    packs = lambda: (ops._cm_pack(x0), ops._cm_pack(y0))

    def op():
        x, y = x0.clone().requires_grad_(True), y0.clone().requires_grad_(True)
        l, s = ops.soft_coord_match(x, y, xyz, gamma)
        ((l * a).sum() + (s * b).sum()).backward()

    def ref():
        x, y = x0.clone().requires_grad_(True), y0.clone().requires_grad_(True)
        l, s = loss.soft_coord_reference(x, y, xyz, gamma)
        ((l * a).sum() + (s * b).sum()).backward()

    rs = np.random.RandomState(0)
    B = 24
    vis = torch.from_numpy((rs.rand(B, M) < 0.6).astype(np.uint8)).to(dev)
    gidx = torch.from_numpy(rs.randint(0, M + 1, size=R).astype(np.int32)).to(dev)
    item = torch.from_numpy(np.sort(rs.randint(0, B, size=R)).astype(np.int32)).to(dev)
    nbr, visb = ops.circle_nbr_table(xyz, 0.004), ops.circle_visbits(vis)

    def circle():
        x, y = x0.clone().requires_grad_(True), y0.clone().requires_grad_(True)
        ops.circle_match(x, y, gidx, item, nbr=nbr, visb=visb).sum().backward()

    flops_s = 2.0 * 3 * R * Mp * 128                               # one S tile: three bf16 products per fp32 product
    lines.append("\n### R = %d, M = %d, gamma = %g (P = %d row slices for grad y)\n" % (R, M, gamma, P))
    lines.append("| what | median ms | min | max | peak MiB over the inputs |\n|---|---|---|---|---|")
    for name, fn, mem in (("forward launch (`soft_coord_kernel<0>`)", fwd, None), ("grad x launch (`soft_coord_kernel<1>`)", bx, None),
                          ("grad y launches (`soft_coord_kernel<2>` + partial sum)", by, None),
                          ("the two packs (x and y; repeated beside the circle loss's own)", packs, None),
                          ("`ops.soft_coord_match` forward + backward (autograd, packs included)", op, True),
                          ("`ops.circle_match` forward + backward", circle, True),
                          ("`loss.soft_coord_reference` forward + backward (materialised)", ref, True)):
        med, lo, hi = timed(fn)
        lines.append("| %s | %.3f | %.3f | %.3f | %s |" % (name, med, lo, hi, "%.0f" % peak_of(fn) if mem else "-"))
        print(lines[-1], flush=True)
    t_op, t_ref = timed(op)[0], timed(ref)[0]
    lines.append("\nOne S tile pass is %.1f GFLOP of bf16 MFMA work (three products per fp32 product); the forward does one, each gradient two." % (flops_s / 1e9))
    lines.append("The operator %s the materialised form in time at this shape: %.3f ms against %.3f ms (forward + backward)."
                 % ("beats" if t_op < t_ref else "DOES NOT beat", t_op, t_ref))


def step_times(lines):
    from geometric_aware_dense_matching_amd import synthetic, train_lm
    from geometric_aware_dense_matching_amd.config import make_model_cfg
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    B, N, M = 24, 4096, 4096
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = GeoMatch(make_model_cfg(n_mesh_node=M, num_points=N), 1, model_points=synthetic.make_model_points(1, M)).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-5)
    ds = train_lm.SyntheticCrops(B, N, M, seed=0)
    cu = train_lm.to_device(torch.utils.data.default_collate([ds[i] for i in range(B)]), dev)

    def step(on):
        model.soft_xyz_weight = model.soft_nll_weight = 1.0 if on else 0.0
        out, _ = train_lm.model_fn_dec(model, dict(cu), dev)
        out["loss"].backward()
        opt.step()
        opt.zero_grad()
        return out

    for on in (False, True, False, True):
        step(on)
    torch.cuda.synchronize()
    res = {False: [], True: []}
    for _ in range(6):                                            # alternating, host clock around a synchronise
        for on in (False, True):
            t0 = time.perf_counter()
            out = step(on)
            torch.cuda.synchronize()
            res[on].append((time.perf_counter() - t0) * 1e3)
    lines.append("\n### Training step, eager, B = %d, N = M = %d (forward + losses + backward + Adam; host clock around a synchronise, alternating)\n" % (B, N))
    lines.append("| step | median ms | min | max |\n|---|---|---|---|")
    for on in (False, True):
        v = res[on]
        lines.append("| %s | %.1f | %.1f | %.1f |" % ("both losses on (weights 1)" if on else "both weights 0 (the step as it was)", np.median(v), min(v), max(v)))
        print(lines[-1], flush=True)
    lines.append("\nThe losses add %.1f ms to the eager step; the operator's share is its forward + backward time above, the rest is the torch "
                 "operations around it (row gathers, smooth L1, per-item sums; not profiled apart)." % (np.median(res[True]) - np.median(res[False])))
    lines.append("\nLast values with the losses on: soft_xyz_loss %.6f m, soft_nll_loss %.4f (synthetic data, an untrained network: no claim)."
                 % (float(out["soft_xyz_loss"].detach()), float(out["soft_nll_loss"].detach())))


def error_maxima(lines):
    import soft_coord_cases as sc
    shapes = [(1, 1), (5, 31), (127, 64), (128, 65), (129, 130), (300, 1000), (257, 4097)]
    worst = dict(lse=0.0, soft=0.0, gx=0.0, gy=0.0, rx=0.0, ry=0.0, lse_abs=0.0, soft_abs=0.0)
    for R, M in shapes:
        for gamma in (1.0, 16.0, 40.0):
            for family in ("random", "copy"):
                x, y, xyz, a, b = sc.make_case(R, M, seed=1000 * R + M, family=family)
                t64 = [torch.from_numpy(v).double() for v in (x, y, xyz, a, b)]
                ref = sc.analytic(*t64, gamma)
                bnd = sc.bounds(ref, t64[4], t64[2], gamma, R, M)
                xd, yd = torch.from_numpy(x).cuda().requires_grad_(True), torch.from_numpy(y).cuda().requires_grad_(True)
                lse, soft = ops.soft_coord_match(xd, yd, torch.from_numpy(xyz).cuda(), gamma)
                ((lse * torch.from_numpy(a).cuda()).sum() + (soft * torch.from_numpy(b).cuda()).sum()).backward()
                el = (lse.detach().double().cpu() - ref["lse"]).abs().max().item()
                es = (soft.detach().double().cpu() - ref["soft"]).abs().max().item()
                ex = (xd.grad.double().cpu() - ref["gx"]).abs().numpy()
                ey = (yd.grad.double().cpu() - ref["gy"]).abs().numpy()
                for k, v in (("lse", el / bnd["lse"]), ("soft", es / bnd["soft"]), ("gx", (ex.max(1) / bnd["gx"]).max()),
                             ("gy", (ey.max(1) / bnd["gy"]).max()), ("rx", ex.max() / ref["gx"].abs().max().item()),
                             ("ry", ey.max() / ref["gy"].abs().max().item()), ("lse_abs", el), ("soft_abs", es)):
                    worst[k] = max(worst[k], float(v))
    lines.append("\n### Measured maxima of the bounded error quantities (the 7 shapes x gamma in {1, 16, 40} x {random, bit-copy} of the GPU test)\n")
    lines.append("| quantity | measured maximum |\n|---|---|")
    lines.append("| lse error / (gamma delta + 1e-5) | %.3e (largest absolute error %.3e) |" % (worst["lse"], worst["lse_abs"]))
    lines.append("| soft error / (E rho + 1e-6) | %.3e (largest absolute error %.3e m) |" % (worst["soft"], worst["soft_abs"]))
    lines.append("| gx error / its per-row bound | %.3e |" % worst["gx"])
    lines.append("| gy error / its per-column bound | %.3e |" % worst["gy"])
    lines.append("| max abs gx error / max abs gx (bound 1e-2) | %.3e |" % worst["rx"])
    lines.append("| max abs gy error / max abs gy (bound 1e-2) | %.3e |" % worst["ry"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_coord.md"))
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("soft_coord_profile.py measures on the GPU; there is nothing to record without one")
    lines = ["# Soft-assignment training operator: measured on one MI355X (`tools/soft_coord_profile.py`)\n",
             "Device-event times, median of 20 calls after 3 warm-up calls, one process; torch %s.  Synthetic unit descriptors." % torch.__version__]
    kernel_times(49152, 4096, 16.0, lines)
    kernel_times(32768, 8192, 16.0, lines)
    if not args.no_step:
        step_times(lines)
    error_maxima(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
