#!/usr/bin/env python3
"""Costs of two-way matching and the cycle filter at the headline shape (B = 16, N = 2048, M = 8192, split-bf16) in ONE run on the
GPU; writes profiles/match_twoway.md.

  (a) one-way     gdm_match_packed_hip of the PARENT commit's build (a second libgdm_hip.so, --parent-lib) and of this build, on
                  the same packed rows, alternating window by window
  (b) two-way     gdm_match_twoway_packed_hip: key memset, panel kernel, row merge, key decode
  (c) composed    ops.match(return_sim=True) + the masked column maximum in torch, with its peak memory
  (d) filter      gdm_match_cycle_hip
  odd shapes      (a') and (b) through ops at N = 300 (a crop boundary inside most row blocks) and N = 20 (a crop shorter than a wave tile:
                  the crop loop runs twice or more per 64-column step and crops past the LDS slots go to the keys directly)
  (e) step        infer.pipeline_step(with_pose=True) eager, with and without pair_filter="cycle", alternating
  survival        the planted case of tests/test_gpu_match_twoway.py (match_twoway_cases.filter_case) at N = 2048: the share of the
                  planted wrong pairs that the filter keeps at radius 0, 0.005 and 0.02

Timing as tools/match_soft_profile.py (device events, warm-up, windows of at least --window seconds, --rounds windows per variant,
variants alternating).  The parent's library is built beforehand, where the repository's history is at hand:
    python tools/match_soft_profile.py --build-parent HEAD~1 build/parent_lib
    python tools/match_twoway_profile.py --parent-lib build/parent_lib/geometric_aware_dense_matching_amd/libgdm_hip.so"""
import argparse
import ctypes
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from match_soft_profile import alternate, fmt          # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--npoints", type=int, default=2048)
    ap.add_argument("--mesh", type=int, default=8192)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="skip the pipeline_step timings")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_twoway.md"))
    args = ap.parse_args()

    import torch
    import match_twoway_cases as mc
    from geometric_aware_dense_matching_amd import _lib, infer, ops, pose, synthetic
    from geometric_aware_dense_matching_amd.config import make_model_cfg
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    if not torch.cuda.is_available():
        raise SystemExit("match_twoway_profile: needs the GPU (a CPU run measures nothing)")
    B, N, M = args.batch, args.npoints, args.mesh
    L = _lib.lib()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        res, argtypes = _lib.SIGNATURES["gdm_match_packed_hip"]
        parent.gdm_match_packed_hip.restype, parent.gdm_match_packed_hip.argtypes = res, argtypes
        assert not hasattr(parent, "gdm_match_twoway_packed_hip"), "--parent-lib is not the parent's library"
    dev = torch.device("cuda:0")
    prec = ops.MATCH_BF16X3
    lines = ["# Two-way matching and the cycle filter: cost at B = %d, N = %d, M = %d, split-bf16" % (B, N, M), "",
             "Written by `python tools/match_twoway_profile.py %s` on %s." % (" ".join(sys.argv[1:]), torch.cuda.get_device_name(0)),
             "Device events, warmed up, windows of at least %.2f s of back-to-back launches; microseconds per launch sequence, "
             "median (min, max) over the windows; variants alternate window by window." % args.window, ""]

    rs = np.random.RandomState(zlib.crc32(b"match_twoway_profile"))
    scene = torch.from_numpy(rs.randn(B, 128, N).astype(np.float32) * rs.rand(B, 1, N).astype(np.float32) * 3).to(dev)
    model = torch.from_numpy(rs.randn(128, M).astype(np.float32)).to(dev)
    mask = torch.from_numpy((rs.rand(B, N) < 0.6).astype(np.uint8)).to(dev)
    cld = torch.from_numpy(rs.uniform(-0.1, 0.1, (B, 9, N)).astype(np.float32)).to(dev)
    srows, mrows = ops.match_pack2(scene, model, prec)
    part = torch.empty(int(L.gdm_match_twoway_partial_bytes(B, N, M)), dtype=torch.uint8, device=dev)
    hard_bytes = int(L.gdm_match_partial_bytes(B, N))
    bi, ci = torch.empty((B, N), dtype=torch.int32, device=dev), torch.empty((B, M), dtype=torch.int32, device=dev)
    bs, cs = torch.empty((B, N), dtype=torch.float32, device=dev), torch.empty((B, M), dtype=torch.float32, device=dev)
    pm, pc = torch.empty((B, N), dtype=torch.uint8, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
    d2 = torch.empty((B, N), dtype=torch.float32, device=dev)

    def hard(lib):
        rc = lib.gdm_match_packed_hip(srows.data_ptr(), mrows.data_ptr(), B * N, M, prec, bi.data_ptr(), bs.data_ptr(), None,
                                      part.data_ptr(), hard_bytes, ops._stream())
        assert rc == 0, rc

    def twoway():
        rc = L.gdm_match_twoway_packed_hip(srows.data_ptr(), mrows.data_ptr(), mask.data_ptr(), B, N, M, prec, bi.data_ptr(), bs.data_ptr(),
                                           ci.data_ptr(), cs.data_ptr(), part.data_ptr(), part.numel(), ops._stream())
        assert rc == 0, rc

    def cycle():
        rc = L.gdm_match_cycle_hip(cld.data_ptr(), cld.stride(0), 1, N, bi.data_ptr(), ci.data_ptr(), mask.data_ptr(), B, N, M, 0.005,
                                   pm.data_ptr(), pc.data_ptr(), d2.data_ptr(), ops._stream())
        assert rc == 0, rc

    sim_out = torch.empty((B, N, M), dtype=torch.float32, device=dev)
    neg = torch.tensor(float("-inf"), device=dev)

    def composed():
        sim = ops.match_packed(srows, mrows, B, N, M, prec, return_sim=True, sim_out=sim_out)[2]
        return torch.where(mask[:, :, None] != 0, sim, neg).max(dim=1)

    fns = {}
    if parent is not None:
        fns["(a) one-way, parent commit"] = lambda: hard(parent)
    fns["(a') one-way, this commit"] = lambda: hard(L)
    fns["(b) two-way (key memset + panel kernel + row merge + key decode)"] = twoway
    fns["(d) cycle filter"] = cycle
    twoway()
    t = alternate(fns, args.window, args.rounds, torch)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base_mem = torch.cuda.memory_allocated()
    t.update(alternate({"(c) composed: match(return_sim) + masked column max in torch": composed}, args.window, max(args.rounds // 2, 2), torch))
    peak = torch.cuda.max_memory_allocated() - base_mem + sim_out.numel() * 4
    lines += ["## Matching launches", "", "| variant | us |", "|---|---|"] + ["| %s | %s |" % (k, fmt(v)) for k, v in t.items()]
    med = {k[:3]: float(np.median(v)) for k, v in t.items()}
    a = med.get("(a)", med["(a'"])
    lines += ["", "(b) / (a) = %.2f (two one-way launches, the cost of the reverse direction by swapped operands, would be 2.00); "
              "(c) / (b) = %.1f; (c) holds %.2f GB at its peak (the matrix and torch's temporaries), (b) a workspace of %.1f MB." %
              (med["(b)"] / a, med["(c)"] / med["(b)"], peak / 1e9, part.numel() / 1e6)]
    # what the timed launches computed: the two-way pairs against the one-way launch, the columns against the composed route
    twoway()
    got = (bi.clone(), bs.clone(), ci.clone(), cs.clone())
    hard(L)
    cv, cix = composed()
    torch.cuda.synchronize()
    lines += ["", "Two-way best_idx / best_sim against the one-way launch: %s.  col_sim against the composed route: %s; col_idx: %s "
              "(torch.max names some maximal row, the kernel the lowest)." %
              ("bit-identical" if torch.equal(got[0], bi) and torch.equal(got[1], bs) else "DIFFERENT",
               "equal" if torch.equal(got[3], cv) else "DIFFERENT", "%d of %d equal" % (int((got[2] == cix).sum()), B * M)), ""]

    # shapes off the headline: the same number of rows, crops that do not end on row blocks
    lines += ["## Odd crop lengths (same %d rows and M; through ops.match_packed / ops.match_twoway_packed)" % (B * N), "",
              "| B x N | one-way us | two-way us | ratio |", "|---|---|---|---|"]
    for b2, n2 in ((B * N // 300, 300), (B * N // 20, 20)):
        sc = scene.permute(1, 0, 2).reshape(128, B * N)[:, :b2 * n2].reshape(128, b2, n2).permute(1, 0, 2).contiguous()
        sr, mr = ops.match_pack2(sc, model, prec)
        mk = mask.reshape(-1)[:b2 * n2].reshape(b2, n2).contiguous()
        t2 = alternate({"one": lambda: ops.match_packed(sr, mr, b2, n2, M, prec), "two": lambda: ops.match_twoway_packed(sr, mr, mk, b2, n2, M, prec)},
                       args.window, max(args.rounds // 2, 2), torch)
        lines.append("| %d x %d | %s | %s | %.2f |" % (b2, n2, fmt(t2["one"]), fmt(t2["two"]), float(np.median(t2["two"])) / float(np.median(t2["one"]))))
    lines.append("")

    # survival of planted wrong pairs
    c = mc.filter_case(B=2, N=N, M=M, name="match_twoway_profile filter")
    cu = {k: torch.from_numpy(v).to(dev) for k, v in c.items()}
    ones = torch.ones((2, N), dtype=torch.uint8, device=dev)
    fbi, fbs, fci, fcs = ops.match_twoway(cu["scene"], cu["model"], ones, prec)
    wrong = cu["inlier"] == 0
    lines += ["## Planted wrong pairs that survive the filter (unpinned observation)", "",
              "match_twoway_cases.filter_case at B = 2, N = %d, M = %d: %d planted wrong pairs (each claims an inlier's vertex from more "
              "than 5 cm away), %d inliers." % (N, M, int(wrong.sum()), int((~wrong).sum())), "",
              "| radius (m) | wrong pairs kept | share | inliers kept |", "|---|---|---|---|"]
    for radius in (0.0, 0.005, 0.02):
        keep = ops.match_cycle(cu["cld"], fbi, fci, ones, radius)[0] != 0
        lines.append("| %g | %d | %.4f | %d of %d |" % (radius, int((keep & wrong).sum()), float((keep & wrong).sum()) / max(int(wrong.sum()), 1),
                                                       int((keep & ~wrong).sum()), int((~wrong).sum())))
    lines.append("")

    if not args.no_step:
        torch.manual_seed(0)
        net = GeoMatch(make_model_cfg(n_mesh_node=M, num_points=N), 1, model_points=synthetic.make_model_points(1, M))
        tmpl = {k: v for k, v in net.state_dict().items()
                if not k.startswith("model_emb.mesh_graph") and k not in ("model_emb.xyz", "model_emb.const_one")}
        net.load_state_dict(synthetic.synthetic_state_dict(tmpl, seed=0), strict=False)
        net = net.to(dev).eval()
        batch = synthetic.make_batch(seed=100, batch=B, n_points=N)
        inputs = {k: torch.from_numpy(batch[k]).to(dev) for k in ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")}
        kinds = {"Kabsch (default)": dict(), "Kabsch behind pair_filter=cycle": dict(pose_opts=dict(pair_filter="cycle"))}
        with torch.no_grad():
            t = alternate({k: (lambda kw=kw: infer.pipeline_step(net, inputs, with_pose=True, **kw)) for k, kw in kinds.items()},
                          args.window, args.rounds, torch)
            out = infer.pipeline_step(net, inputs, with_pose=True, pose_opts=dict(pair_filter="cycle"))
        lines += ["## (e) pipeline_step(with_pose=True), eager, bf16x3", "", "| pose stage | us per step |", "|---|---|"]
        lines += ["| %s | %s |" % (k, fmt(v)) for k, v in t.items()]
        lines += ["", "(Seeded weights, no checkpoint: %d of %d points are masked and the filter keeps %d of them at the default radius "
                  "%g m; the figure says what the launches cost, nothing about what the filter is worth on a trained network.)" %
                  (int(out["count"].sum()), B * N, int(out["pair_count"].sum()), pose.CYCLE_RADIUS), ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
