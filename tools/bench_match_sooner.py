"""The two kernels that start matching sooner, each alone (profiles/match_sooner.md): event-timed, 30 launches back to back on a warm
chip, every form in one process.

  mesh layer   gdm_spline_direct3_hip at M = 8192, Cin = 9, C = 128, 4 in-edges per vertex: weights from LDS / from global memory
  heads        gdm_point_heads3_hip at B = 16, N = 2048 with and without the rows, and gdm_match_pack_hip of the same features

--parent-lib PATH: a libgdm_hip.so built from the parent commit.  Its kernels are timed in the same process, through ctypes with the
parent's prototypes (gdm_spline_direct3_hip without weights_in_lds, gdm_point_heads2_hip), so that each part is measured against the
kernel it replaces and not against this library's copy of it.  --only mesh|heads: one part (a counters run wants few kernels).
Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geometric_aware_dense_matching_amd import _lib, ops  # noqa: E402

VP, I = ctypes.c_void_p, ctypes.c_int
P = lambda t: VP(t.data_ptr()) if t is not None else VP(None)


def timed(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return round(s.elapsed_time(e) / n * 1e3, 2)          # us per launch


def must(rc, what):
    if rc != 0:
        raise RuntimeError("%s returned %d" % (what, rc))


def mesh_part(lib, parent, M, Cin):
    rs = np.random.RandomState(0)
    C, deg = 128, 4
    x = torch.from_numpy(rs.randn(M, Cin).astype(np.float32)).cuda()
    w = torch.from_numpy((rs.randn(125, Cin, C) / 3).astype(np.float32)).cuda()
    rowptr = torch.arange(0, deg * M + 1, deg, dtype=torch.int32).cuda()
    src = torch.from_numpy(rs.randint(0, M, deg * M).astype(np.int32)).cuda()
    attr = torch.from_numpy(rs.rand(deg * M, 3).astype(np.float32)).cuda()
    root = torch.from_numpy((rs.randn(Cin, C) / 3).astype(np.float32)).cuda()
    bias = torch.from_numpy(rs.randn(C).astype(np.float32)).cuda()
    pk_bytes = lib.gdm_conv3x3_act_bytes(1, C, 1, M)
    outs = {k: (torch.empty(C, M, device="cuda"), torch.zeros(pk_bytes, dtype=torch.uint8, device="cuda")) for k in ("lds", "global", "parent")}
    stream = VP(torch.cuda.current_stream().cuda_stream)
    head = (P(x), P(w), P(rowptr), P(src), P(attr), P(root), P(bias), I(M), I(Cin), I(C), I(5), I(1), VP(None))

    def run(l, key, *tail):
        return lambda: must(l.gdm_spline_direct3_hip(*head, P(outs[key][0]), P(outs[key][1]), *tail, stream), "gdm_spline_direct3_hip")
    res = {"M": M, "Cin": Cin, "lds_us": timed(run(lib, "lds", I(1))), "global_us": timed(run(lib, "global", I(0)))}
    if parent is not None:
        res["parent_us"] = timed(run(parent, "parent"))
        res["lds_us_again"] = timed(run(lib, "lds", I(1)))
        res["same_bits_as_parent"] = all(torch.equal(a, b) for a, b in zip(outs["lds"], outs["parent"]))
    res["same_bits_lds_global"] = all(torch.equal(a, b) for a, b in zip(outs["lds"], outs["global"]))
    return res


def heads_part(lib, parent, B, N):
    rs = np.random.RandomState(1)
    x0 = torch.from_numpy(rs.randn(B, 128, N).astype(np.float32)).cuda()
    a, b = x0[:, :64].contiguous(), x0[:, 64:].contiguous()
    Ws = [ops.gemm_pack_weight(torch.from_numpy((rs.randn(128, 128) / 11).astype(np.float32)).cuda()) for _ in range(8)]
    sc = [torch.from_numpy((rs.rand(128) + 0.5).astype(np.float32)).cuda() for _ in range(8)]
    sh = [torch.from_numpy((rs.randn(128) * 0.3).astype(np.float32)).cuda() for _ in range(8)]
    sc[3] = sh[3] = None
    w_last = ops.gemm_pack_weight(torch.from_numpy((rs.randn(2, 128) / 11).astype(np.float32)).cuda())
    b_last = torch.from_numpy(rs.randn(2).astype(np.float32)).cuda()
    w_arr = (VP * 8)(*[t.data_ptr() for t in Ws])
    sc_arr = (VP * 8)(*[t.data_ptr() if t is not None else None for t in sc])
    sh_arr = (VP * 8)(*[t.data_ptr() if t is not None else None for t in sh])
    act = (I * 8)(1, 1, 1, 0, 1, 1, 1, 1)
    arr = lambda v: ctypes.cast(v, VP)
    feat = {k: torch.empty(B, 128, N, device="cuda") for k in ("rows", "plain", "parent")}
    seg = {k: torch.empty(B, 2, N, device="cuda") for k in feat}
    rows = torch.empty(B * N * 512, dtype=torch.uint8, device="cuda")
    packed = {k: torch.empty_like(rows) for k in ("here", "parent")}
    stream = VP(torch.cuda.current_stream().cuda_stream)

    def head(k):
        return (P(a), P(b), I(64), VP(None), VP(None), I(0), I(B), I(N), I(8), arr(w_arr), arr(sc_arr), arr(sh_arr), arr(act), I(3), I(4),
                P(w_last), P(b_last), I(2), P(feat[k]), P(seg[k]))
    with_rows = lambda: must(lib.gdm_point_heads3_hip(*head("rows"), P(rows), stream), "gdm_point_heads3_hip")
    without = lambda: must(lib.gdm_point_heads3_hip(*head("plain"), VP(None), stream), "gdm_point_heads3_hip")
    pack = lambda l, k: (lambda: must(l.gdm_match_pack_hip(P(feat["plain"]), I(B), I(128), I(N), I(_lib.GDM_MATCH_BF16X3), P(packed[k]), stream),
                                      "gdm_match_pack_hip"))
    res = {"B": B, "N": N, "heads_rows_us": timed(with_rows), "heads_us": timed(without), "pack_us": timed(pack(lib, "here"))}
    if parent is not None:
        res["parent_heads_us"] = timed(lambda: must(parent.gdm_point_heads2_hip(*head("parent"), stream), "gdm_point_heads2_hip"))
        res["parent_pack_us"] = timed(pack(parent, "parent"))
        res["heads_rows_us_again"] = timed(with_rows)
        res["same_bits_as_parent"] = (torch.equal(feat["rows"], feat["parent"]) and torch.equal(seg["rows"], seg["parent"])
                                      and torch.equal(rows, packed["parent"]))
    res["rows_equal_pack"] = torch.equal(rows, packed["here"])
    res["feat_seg_equal_without_rows"] = torch.equal(feat["rows"], feat["plain"]) and torch.equal(seg["rows"], seg["plain"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--only", choices=("mesh", "heads"))
    ap.add_argument("--M", type=int, default=8192)
    ap.add_argument("--cin", type=int, default=9)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--N", type=int, default=2048)
    args = ap.parse_args()
    lib = _lib.lib()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("gdm_spline_direct3_hip", "gdm_point_heads2_hip", "gdm_match_pack_hip"):
            getattr(parent, name).restype = I
    # this library's entries through raw ctypes too (no argument conversion of the package between two launches)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gdm_spline_direct3_hip", "gdm_point_heads3_hip", "gdm_match_pack_hip"):
        getattr(raw, name).restype = I
    raw.gdm_conv3x3_act_bytes.restype = ctypes.c_size_t
    raw.gdm_conv3x3_act_bytes.argtypes = [I, I, I, I]
    out = {}
    if args.only in (None, "mesh"):
        out["mesh_layer"] = mesh_part(raw, parent, args.M, args.cin)
    if args.only in (None, "heads"):
        out["heads"] = heads_part(raw, parent, args.B, args.N)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
