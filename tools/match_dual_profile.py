#!/usr/bin/env python3
"""Costs of dual-softmax matching at the headline shape (B = 16, N = 2048, M = 8192, split-bf16) in ONE run on the GPU, and the
registers, scratch and LDS of the new kernel from the compiler's resource-usage remarks; writes profiles/match_dual.md.

  (a) soft        gdm_match_soft_packed_hip of the PARENT commit's build (a second libgdm_hip.so, --parent-lib) and of this build
  (b) two-way     gdm_match_twoway_packed_hip, likewise
  (c) dual        gdm_match_dual_packed_hip: key memset, panel kernel, row merge, column kernel, row kernel
  (d) composed    ops.match_packed(return_sim=True) + the same row and column reductions in torch, with its peak memory
  odd shapes      (a), (b), (c) through ops at N = 300 and N = 20: the dual kernel's row blocks never span a crop, so a crop of 300
                  points takes two row blocks (the second 44 rows long) and a crop of 20 points a whole row block

Timing as tools/match_soft_profile.py (device events, warm-up, windows of at least --window seconds, --rounds windows per variant,
variants alternating).  The parent's library is built beforehand, where the repository's history is at hand:
    python tools/match_soft_profile.py --build-parent HEAD~1 build/parent_lib
    python tools/match_dual_profile.py --parent-lib build/parent_lib/geometric_aware_dense_matching_amd/libgdm_hip.so"""
import argparse
import ctypes
import os
import re
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from match_soft_profile import alternate, fmt          # noqa: E402

CSRC = os.path.join(ROOT, "geometric_aware_dense_matching_amd", "csrc")
LDS_BYTES = 128 * 1024 + 256 * 3 * 4 + 256 * 8 + 8 * 256 * 4          # panel + xyz + keys + 8 waves x 256 column sums (DUAL_LDS_BYTES)


def resources():
    """{kernel: (VGPRs, AGPRs, scratch bytes per lane)} of the panel kernels of gdm_match.hip, from -Rpass-analysis with the Makefile's flags."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", mk, flags=re.M))
    flags = var["CXXFLAGS"].replace("$(ARCH)", var["ARCH"]).split()
    cmd = [os.environ.get("HIPCC", var["HIPCC"])] + flags + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                                              os.path.join(CSRC, "gdm_match.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stderr
    out = {}
    for m in re.finditer(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", text, flags=re.S):
        k = re.search(r"(match_panel_(?:soft|twoway|dual)_kernel)ILi(\d)E", m.group(1))
        if k:
            out["%s<%s>" % (k.group(1), "BF16X3" if k.group(2) == "0" else "F32")] = tuple(int(x) for x in m.groups()[1:])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--npoints", type=int, default=2048)
    ap.add_argument("--mesh", type=int, default=8192)
    ap.add_argument("--gamma", type=float, default=16.0)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-resources", action="store_true", help="skip the compile that reads the resource-usage remarks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_dual.md"))
    args = ap.parse_args()

    import torch
    from geometric_aware_dense_matching_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("match_dual_profile: needs the GPU (a CPU run measures nothing)")
    B, N, M, gamma = args.batch, args.npoints, args.mesh, args.gamma
    L = _lib.lib()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("gdm_match_soft_packed_hip", "gdm_match_twoway_packed_hip"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
        assert not hasattr(parent, "gdm_match_dual_packed_hip"), "--parent-lib is not the parent's library"
    dev = torch.device("cuda:0")
    prec = ops.MATCH_BF16X3
    argv = [a for i, a in enumerate(sys.argv[1:], 1) if a != "--out" and sys.argv[i - 1] != "--out"]          # where it was written is no setting
    lines = ["# Dual-softmax matching: cost at B = %d, N = %d, M = %d, split-bf16, gamma = %g" % (B, N, M, gamma), "",
             "Written by `python tools/match_dual_profile.py %s` on %s." % (" ".join(argv), torch.cuda.get_device_name(0)),
             "Device events, warmed up, windows of at least %.2f s of back-to-back launches; microseconds per launch sequence, "
             "median (min, max) over the windows; variants alternate window by window." % args.window, ""]

    if not args.no_resources:
        res = resources()
        lines += ["## Registers, scratch and LDS (the compiler's resource-usage remarks; 8 waves per workgroup, one workgroup per CU, "
                  "256 VGPRs per wave)", "", "| kernel | VGPRs | AGPRs | scratch bytes per lane | LDS bytes per workgroup (dynamic) |",
                  "|---|---|---|---|---|"]
        lds = {"soft": 128 * 1024 + 3072, "twoway": 128 * 1024 + 4096, "dual": LDS_BYTES}
        for k in sorted(res):
            lines.append("| `%s` | %d | %d | %d | %d |" % ((k,) + res[k] + (lds[k.split("_")[2]],)))
        assert all(v[2] == 0 for k, v in res.items() if "dual" in k), "the dual kernel must not spill"
        lines += ["", "The form that shipped is the fused one: one pass of MFMAs gives the row softmax, the column arg-max and the column "
                  "sum, with no scratch.  It fits because a step of the dual kernel is one 32-column accumulator block (16 VGPRs) where "
                  "the soft and two-way kernels take two (32), and because what the column bookkeeping and the row-block tail derive from "
                  "the lane index is formed where it is used instead of being held across the products.", ""]

    rs = np.random.RandomState(zlib.crc32(b"match_dual_profile"))
    scene = torch.from_numpy(rs.randn(B, 128, N).astype(np.float32) * rs.rand(B, 1, N).astype(np.float32) * 3).to(dev)
    model = torch.from_numpy(rs.randn(128, M).astype(np.float32)).to(dev)
    xyz = torch.from_numpy(rs.uniform(-0.05, 0.05, (M, 3)).astype(np.float32)).to(dev)
    mask = torch.from_numpy((rs.rand(B, N) < 0.6).astype(np.uint8)).to(dev)
    srows, mrows = ops.match_pack2(scene, model, prec)
    part = torch.empty(int(L.gdm_match_dual_partial_bytes(B, N, M)), dtype=torch.uint8, device=dev)
    f32, i32 = torch.float32, torch.int32
    o = {k: torch.empty(s, dtype=t, device=dev) for k, s, t in
         (("best_idx", (B, N), i32), ("best_sim", (B, N), f32), ("lse", (B, N), f32), ("conf", (B, N), f32), ("soft_xyz", (B, N, 3), f32),
          ("col_idx", (B, M), i32), ("col_sim", (B, M), f32), ("col_lse", (B, M), f32), ("col_conf", (B, M), f32), ("dual", (B, N), f32))}
    p = {k: v.data_ptr() for k, v in o.items()}

    def soft(lib):
        rc = lib.gdm_match_soft_packed_hip(srows.data_ptr(), mrows.data_ptr(), xyz.data_ptr(), B * N, M, prec, gamma, p["best_idx"],
                                           p["best_sim"], p["lse"], p["conf"], p["soft_xyz"], part.data_ptr(),
                                           int(L.gdm_match_soft_partial_bytes(B, N)), ops._stream())
        assert rc == 0, rc

    def twoway(lib):
        rc = lib.gdm_match_twoway_packed_hip(srows.data_ptr(), mrows.data_ptr(), mask.data_ptr(), B, N, M, prec, p["best_idx"], p["best_sim"],
                                             p["col_idx"], p["col_sim"], part.data_ptr(), int(L.gdm_match_twoway_partial_bytes(B, N, M)),
                                             ops._stream())
        assert rc == 0, rc

    def dual():
        rc = L.gdm_match_dual_packed_hip(srows.data_ptr(), mrows.data_ptr(), xyz.data_ptr(), mask.data_ptr(), B, N, M, prec, gamma,
                                         *[p[k] for k in ops.DUAL_KEYS], part.data_ptr(), part.numel(), ops._stream())
        assert rc == 0, rc

    sim_out = torch.empty((B, N, M), dtype=torch.float32, device=dev)
    neg = torch.tensor(float("-inf"), device=dev)

    def composed():
        sim = ops.match_packed(srows, mrows, B, N, M, prec, return_sim=True, sim_out=sim_out)[2]
        w = torch.exp(gamma * (sim - 1))
        Z = w.sum(dim=2)
        bs, bi = sim.max(dim=2)
        wb = torch.exp(gamma * (bs - 1))
        conf = wb / Z
        sxyz = (w @ xyz) / Z[:, :, None]
        on = mask[:, :, None] != 0
        Zc = torch.where(on, w, torch.zeros((), device=dev)).sum(dim=1)
        cs, ci = torch.where(on, sim, neg).max(dim=1)
        col_conf = torch.exp(gamma * (cs - 1)) / Zc
        d = conf * wb / Zc.gather(1, bi) * (mask != 0)
        return dict(best_idx=bi, best_sim=bs, lse=gamma + torch.log(Z), conf=conf, soft_xyz=sxyz, col_idx=ci, col_sim=cs,
                    col_lse=gamma + torch.log(Zc), col_conf=col_conf, dual=d)

    fns = {}
    if parent is not None:
        fns["(a) soft, parent commit"] = lambda: soft(parent)
        fns["(b) two-way, parent commit"] = lambda: twoway(parent)
    fns["(a') soft, this commit"] = lambda: soft(L)
    fns["(b') two-way, this commit"] = lambda: twoway(L)
    fns["(c) dual (key memset + panel kernel + row merge + column kernel + row kernel)"] = dual
    dual()
    t = alternate(fns, args.window, args.rounds, torch)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base_mem = torch.cuda.memory_allocated()
    t.update(alternate({"(d) composed: match(return_sim) + row and column reductions in torch": composed}, args.window,
                       max(args.rounds // 2, 2), torch))
    peak = torch.cuda.max_memory_allocated() - base_mem + sim_out.numel() * 4
    lines += ["## Matching launches", "", "| variant | us |", "|---|---|"] + ["| %s | %s |" % (k, fmt(v)) for k, v in t.items()]
    med = {k[:3]: float(np.median(v)) for k, v in t.items()}
    spread = {k[:3]: max(v) - min(v) for k, v in t.items()}
    a, b = med.get("(a)", med["(a'"]), med.get("(b)", med["(b'"])
    saving = a + b - med["(c)"]
    noise = spread.get("(a)", spread["(a'"]) + spread.get("(b)", spread["(b'"]) + spread["(c)"]
    lines += ["", "(a) + (b) = %.1f us, (c) = %.1f us: the dual sequence is %s the two sequences it replaces by %.1f us (%.0f %%), "
              "against %.1f us of spread (max - min) summed over the three sets of windows.  (c) / (a) = %.2f, (c) / (b) = %.2f.  "
              "(d) / (c) = %.1f; (d) holds %.2f GB at its peak (the matrix and torch's temporaries), (c) a workspace of %.1f MB." %
              (a + b, med["(c)"], "below" if saving > 0 else "ABOVE", abs(saving), 100 * abs(saving) / (a + b), noise, med["(c)"] / a,
               med["(c)"] / b, med["(d)"] / med["(c)"], peak / 1e9, part.numel() / 1e6)]
    # what the timed launches computed
    dual()
    got = {k: v.clone() for k, v in o.items()}
    soft(L)
    rows_same = all(torch.equal(got[k].view(i32), o[k].view(i32)) for k in ("best_idx", "best_sim", "lse", "conf", "soft_xyz"))
    twoway(L)
    cols_same = all(torch.equal(got[k].view(i32), o[k].view(i32)) for k in ("col_idx", "col_sim"))
    ref = composed()
    torch.cuda.synchronize()
    on = (mask != 0).any(dim=1)
    diffs = {k: float((got[k][on] - ref[k][on]).abs().max()) for k in ("col_lse", "col_conf", "dual")}
    lines += ["", "Dual rows against the soft launch: %s; dual col_idx / col_sim against the two-way launch: %s.  Against the composed "
              "route (fp32 sums in torch's order): max |col_lse| difference %.3g, col_conf %.3g, dual %.3g." %
              ("bit-identical" if rows_same else "DIFFERENT", "bit-identical" if cols_same else "DIFFERENT", diffs["col_lse"],
               diffs["col_conf"], diffs["dual"]), ""]

    lines += ["## Odd crop lengths (same %d rows and M; through ops.match_soft_packed / match_twoway_packed / match_dual_packed)" % (B * N), "",
              "| B x N | soft us | two-way us | dual us | dual / (soft + two-way) |", "|---|---|---|---|---|"]
    for b2, n2 in ((B * N // 300, 300), (B * N // 20, 20)):
        sc = scene.permute(1, 0, 2).reshape(128, B * N)[:, :b2 * n2].reshape(128, b2, n2).permute(1, 0, 2).contiguous()
        sr, mr = ops.match_pack2(sc, model, prec)
        mk = mask.reshape(-1)[:b2 * n2].reshape(b2, n2).contiguous()
        t2 = alternate({"soft": lambda: ops.match_soft_packed(sr, mr, xyz, b2, n2, M, prec, gamma),
                        "two": lambda: ops.match_twoway_packed(sr, mr, mk, b2, n2, M, prec),
                        "dual": lambda: ops.match_dual_packed(sr, mr, xyz, mk, b2, n2, M, prec, gamma)},
                       args.window, max(args.rounds // 2, 2), torch)
        m2 = {k: float(np.median(v)) for k, v in t2.items()}
        lines.append("| %d x %d | %s | %s | %s | %.2f |" % (b2, n2, fmt(t2["soft"]), fmt(t2["two"]), fmt(t2["dual"]),
                                                            m2["dual"] / (m2["soft"] + m2["two"])))
    lines += ["", "gamma and `cycle_radius` are defaults of a definition, not tuned values.  There is no checkpoint: whether weighing the fit "
              "by `dual` helps a trained network is unmeasured.", ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
