#!/usr/bin/env python3
"""Costs and errors of soft-assignment matching at the headline shape (B = 16, N = 2048, M = 8192), both precisions, in ONE run on
the GPU; writes profiles/match_soft.md.

  hard path   gdm_match_packed_hip of THIS build and of the PARENT commit's build (a second libgdm_hip.so, --parent-lib), on the
              same packed rows, alternating between the two libraries window by window: the check that nothing existing moved.
              Equal means within the spread of repeated windows of the same code.
  soft path   gdm_match_soft_packed_hip under the same conditions.
  step time   infer.pipeline_step(with_pose=True) eager: Kabsch, confidence-weighted Kabsch on soft targets, RANSAC with 20
              hypotheses.
  errors      the measured maxima of the two error checks of tests/test_gpu_match_soft.py at this shape (fp64 over the kernel's own
              similarities; the fp64 restatement from the descriptors), crop by crop.

Timing: device events around windows of at least --window seconds of back-to-back launches, after a warm-up; --rounds windows per
variant.  The parent's library is built beforehand, where the repository's history is at hand:
    python tools/match_soft_profile.py --build-parent HEAD~1 build/parent_lib      (git archive + make; no GPU needed)
    python tools/match_soft_profile.py --parent-lib build/parent_lib/geometric_aware_dense_matching_amd/libgdm_hip.so"""
import argparse
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "geometric_aware_dense_matching_amd"


def build_parent(rev, out_dir):
    """The csrc/ and include/ of `rev`, unpacked under out_dir and built there with its own Makefile."""
    os.makedirs(out_dir, exist_ok=True)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, PKG + "/csrc", "include"], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", out_dir], input=tar, check=True)
    subprocess.run(["make", "-s", "-j16", "-C", os.path.join(out_dir, PKG, "csrc")], check=True)
    print(os.path.join(out_dir, PKG, "libgdm_hip.so"))


def windows(fn, seconds, rounds, torch):
    """-> microseconds per call of each of `rounds` windows of at least `seconds`."""
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(50):
        fn()
    b.record()
    torch.cuda.synchronize()
    n = max(50, int(seconds * 1e3 / max(a.elapsed_time(b) / 50, 1e-4)) + 1)
    out = []
    for _ in range(rounds):
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / n)
    return out


def alternate(fns, seconds, rounds, torch):
    """Windows of the variants in turn (a, b, c, a, b, c, ...) -> {name: [us per call]}."""
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            got[k] += windows(fn, seconds, 1, torch)
    return got


def fmt(v):
    return "%.1f (min %.1f, max %.1f, %d windows)" % (float(np.median(v)), min(v), max(v), len(v))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--build-parent", nargs=2, metavar=("REV", "DIR"), default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--npoints", type=int, default=2048)
    ap.add_argument("--mesh", type=int, default=8192)
    ap.add_argument("--gamma", type=float, default=16.0)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="skip the pipeline_step timings")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_soft.md"))
    args = ap.parse_args()
    if args.build_parent:
        return build_parent(*args.build_parent)

    import torch
    from geometric_aware_dense_matching_amd import _lib, infer, matching, ops, synthetic
    from geometric_aware_dense_matching_amd.config import make_model_cfg
    from geometric_aware_dense_matching_amd.geoMatch import GeoMatch
    if not torch.cuda.is_available():
        raise SystemExit("match_soft_profile: needs the GPU (a CPU run measures nothing)")
    B, N, M, gamma = args.batch, args.npoints, args.mesh, args.gamma
    L = _lib.lib()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        res, argtypes = _lib.SIGNATURES["gdm_match_packed_hip"]
        parent.gdm_match_packed_hip.restype, parent.gdm_match_packed_hip.argtypes = res, argtypes
        assert not hasattr(parent, "gdm_match_soft_packed_hip"), "--parent-lib is not the parent's library"
    dev = torch.device("cuda:0")
    lines = ["# Soft-assignment matching: cost and error at B = %d, N = %d, M = %d, gamma = %g" % (B, N, M, gamma), "",
             "Written by `python tools/match_soft_profile.py %s` on %s." % (" ".join(sys.argv[1:]), torch.cuda.get_device_name(0)),
             "Device events, warmed up, windows of at least %.2f s of back-to-back launches; microseconds per launch sequence, "
             "median (min, max) over the windows; variants alternate window by window." % args.window, ""]

    rs = np.random.RandomState(zlib.crc32(b"match_soft_profile"))
    scene = torch.from_numpy(rs.randn(B, 128, N).astype(np.float32) * rs.rand(B, 1, N).astype(np.float32) * 3).to(dev)
    model = torch.from_numpy(rs.randn(128, M).astype(np.float32)).to(dev)
    xyz = torch.from_numpy((0.05 * rs.uniform(-1, 1, (M, 3))).astype(np.float32)).to(dev)
    for prec, pname in ((ops.MATCH_BF16X3, "bf16x3"), (ops.MATCH_F32, "f32")):
        srows, mrows = ops.match_pack2(scene, model, prec)
        part = torch.empty(int(L.gdm_match_soft_partial_bytes(B, N)), dtype=torch.uint8, device=dev)
        bi = torch.empty((B, N), dtype=torch.int32, device=dev)
        bs, lse, conf = (torch.empty((B, N), dtype=torch.float32, device=dev) for _ in range(3))
        sx = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
        hard_bytes = int(L.gdm_match_partial_bytes(B, N))

        def hard(lib):
            rc = lib.gdm_match_packed_hip(srows.data_ptr(), mrows.data_ptr(), B * N, M, prec, bi.data_ptr(), bs.data_ptr(), None,
                                          part.data_ptr(), hard_bytes, ops._stream())
            assert rc == 0, rc

        def soft():
            rc = L.gdm_match_soft_packed_hip(srows.data_ptr(), mrows.data_ptr(), xyz.data_ptr(), B * N, M, prec, gamma, bi.data_ptr(),
                                             bs.data_ptr(), lse.data_ptr(), conf.data_ptr(), sx.data_ptr(), part.data_ptr(),
                                             part.numel(), ops._stream())
            assert rc == 0, rc

        fns = {"hard, this commit": lambda: hard(L)}
        if parent is not None:
            fns["hard, parent commit"] = lambda: hard(parent)
        fns["hard, this commit again"] = lambda: hard(L)
        fns["soft"] = soft
        t = alternate(fns, args.window, args.rounds, torch)
        lines += ["## %s: matching launches (arg-max [+ merge]; soft + merge)" % pname, "", "| variant | us |", "|---|---|"]
        lines += ["| %s | %s |" % (k, fmt(v)) for k, v in t.items()]
        if parent is not None:
            hard(parent)
            a = (bi.clone(), bs.clone())
            hard(L)
            lines += ["", "Outputs of the two libraries on these rows: %s." %
                      ("bit-identical" if torch.equal(a[0], bi) and torch.equal(a[1], bs) else "DIFFERENT")]
        lines.append("")

        # errors, crop by crop (the [N, M] fp64 matrices of one crop at a time)
        soft()
        hb = ops.match_packed(srows, mrows, B, N, M, prec)
        torch.cuda.synchronize()
        pairs_equal = torch.equal(hb[0], bi) and torch.equal(hb[1], bs)
        u, delta = 2.0 ** -24, 1e-4
        c, E = (M + 8 * gamma + 8) * u, np.expm1(2 * gamma * delta)
        x64 = xyz.cpu().numpy().astype(np.float64)
        rho, xmax = float(np.linalg.norm(x64 - x64.mean(0), axis=1).max()), float(np.abs(x64).max())
        worst = dict(a_lse=0.0, a_conf=0.0, a_soft=0.0, b_lse=0.0, b_conf=0.0, b_soft=0.0)
        mh = model.cpu().numpy()
        for b in range(B):
            sim = ops.match(scene[b:b + 1], model, prec, return_sim=True)[2][0].cpu().numpy()
            g = [t_[b].cpu().numpy().astype(np.float64) for t_ in (lse, conf, sx)]
            for tag, ref in (("a", matching.match_soft_numpy(sim, None, x64, gamma)),
                             ("b", matching.match_soft_numpy(scene[b].cpu().numpy().T, mh, x64, gamma))):
                worst[tag + "_lse"] = max(worst[tag + "_lse"], float(np.abs(g[0] - ref["lse"]).max()))
                worst[tag + "_conf"] = max(worst[tag + "_conf"], float((np.abs(g[1] - ref["conf"]) / ref["conf"]).max()))
                worst[tag + "_soft"] = max(worst[tag + "_soft"], float(np.abs(g[2] - ref["soft_xyz"]).max()))
        lines += ["best_idx / best_sim of the soft launch against ops.match_packed: %s." % ("bit-identical" if pairs_equal else "DIFFERENT"), "",
                  "| error (maximum over all %d rows) | measured | bound |" % (B * N), "|---|---|---|",
                  "| lse, against fp64 over the kernel's similarities | %.3g | c + 4u|lse| with c = (M + 8 gamma + 8) u = %.3g |" % (worst["a_lse"], c),
                  "| conf, relative, same reference | %.3g | 2c = %.3g (+ u absolute) |" % (worst["a_conf"], 2 * c),
                  "| soft_xyz, same reference | %.3g | 2c max|xyz| = %.3g |" % (worst["a_soft"], 2 * c * xmax),
                  "| lse, against the fp64 restatement from the descriptors | %.3g | gamma delta + 1e-5 = %.3g |" % (worst["b_lse"], gamma * delta + 1e-5),
                  "| conf, relative, same reference | %.3g | E = e^(2 gamma delta) - 1 = %.3g (+ 1e-6 absolute) |" % (worst["b_conf"], E),
                  "| soft_xyz, same reference | %.3g | E rho + 1e-6 = %.3g |" % (worst["b_soft"], E * rho + 1e-6), ""]

    if not args.no_step:
        torch.manual_seed(0)
        net = GeoMatch(make_model_cfg(n_mesh_node=M, num_points=N), 1, model_points=synthetic.make_model_points(1, M))
        tmpl = {k: v for k, v in net.state_dict().items()
                if not k.startswith("model_emb.mesh_graph") and k not in ("model_emb.xyz", "model_emb.const_one")}
        net.load_state_dict(synthetic.synthetic_state_dict(tmpl, seed=0), strict=False)
        net = net.to(dev).eval()
        batch = synthetic.make_batch(seed=100, batch=B, n_points=N)
        inputs = {k: torch.from_numpy(batch[k]).to(dev) for k in ("rgb", "cld_rgb_nrm", "choose", "dpt_xyz")}
        kinds = {"Kabsch (default)": dict(),
                 "soft matching, conf-weighted Kabsch on soft targets": dict(match_gamma=gamma, pose_opts=dict(weights="conf", targets="soft")),
                 "RANSAC, 20 hypotheses": dict(pose_fit="ransac", pose_opts=dict(ransac_iters=20))}
        with torch.no_grad():
            t = alternate({k: (lambda kw=kw: infer.pipeline_step(net, inputs, with_pose=True, **kw)) for k, kw in kinds.items()},
                          args.window, args.rounds, torch)
        lines += ["## pipeline_step(with_pose=True), eager, bf16x3", "", "| pose stage | us per step |", "|---|---|"]
        lines += ["| %s | %s |" % (k, fmt(v)) for k, v in t.items()]
        lines.append("")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
