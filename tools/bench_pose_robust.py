"""Timing of the pose stage's fits at the headline shape (B = 16 crops, N = 2048 points, M = 8192 model vertices): the Kabsch fit,
RANSAC at H = 20 / 256 / 1024 hypotheses, the consensus fit (seeds = 8), one ICP iteration of either metric (point-to-point,
point-to-plane), eager and as a graph-captured 10-iteration loop, and one depth-refinement iteration at the shape of
tools/pose_depth_refine_profile.py.  Correspondences: a known pose + 1 mm noise with 30 % of the points
in a background cluster.  Device-event timing of back-to-back calls after a warm-up; also checks that every RANSAC pose is within
1 % of the object diameter of the ground truth (ADD).
    python tools/bench_pose_robust.py [--reps 200] [--out profiles/pose_robust_bench.json]

--parent-lib PATH: a libgdm_hip.so built from the parent commit (same C ABI, so the package's binding serves both libraries in one
process).  First the check: every pose entry is called from both libraries on the same seeded inputs at B in {1, 3}, N in {1, 63, 64,
65, 257, 1024}, M = 777, masks empty / single / full / 60 %, and depth refinement on 130 x 130 windows (3 x 3 tiles of 64 pixels, the last ones 2 wide); every
output array is compared with torch.equal.  Then the rows above, `--rounds` alternating rounds, parent then this library: both medians,
both ranges, and for each row whether this library's median exceeds the parent's by more than the parent's own max - min."""
import argparse
import contextlib
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from geometric_aware_dense_matching_amd import _lib, evaluation, pose, render, synthetic  # noqa: E402


def make(B, N, M, frac, seed=0):
    rs = np.random.RandomState(seed)
    model = ((rs.rand(M, 3) - 0.5) * 0.2).astype(np.float32)
    idx = rs.randint(0, M, size=(B, N)).astype(np.int32)
    cld = np.zeros((B, 9, N), np.float32)
    RT = np.zeros((B, 3, 4), np.float32)
    for b in range(B):
        q, _ = np.linalg.qr(rs.randn(3, 3))
        q *= np.sign(np.linalg.det(q))
        t = np.array([0.01 * b, -0.02, 0.9])
        RT[b, :, :3], RT[b, :, 3] = q, t
        pts = model[idx[b]] @ q.T + t + 0.001 * rs.randn(N, 3)
        out = rs.rand(N) < frac
        pts[out] = t + np.array([0.3, 0.3, 0.0]) + (rs.rand(int(out.sum()), 3) - 0.5) * 0.3
        cld[b, :3] = pts.T
    dev = torch.device("cuda")
    res = dict(mask=torch.ones((B, N), dtype=torch.uint8, device=dev), best_idx=torch.from_numpy(idx).to(dev))
    return res, torch.from_numpy(cld).to(dev), torch.from_numpy(model).to(dev), torch.from_numpy(RT).to(dev)


def unit_normals(M, dev, seed=1):
    nrm = np.random.RandomState(seed).randn(M, 3)
    return torch.from_numpy((nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)).to(dev)


def rot(angle, axis):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx.dot(Kx)


def depth_case(n, C, win, dev, level=3):
    """The candidates, frame and windows of tools/pose_depth_refine_profile.py (480 x 640 frames) -> the arguments of refine_poses_depth."""
    H, W = 480, 640
    K = np.asarray(synthetic.LM_K, dtype=np.float64)
    m = render.demo_mesh(level=level, seed=1)
    rs = np.random.RandomState(0)
    RT = np.zeros((n, C, 3, 4))
    window = np.zeros((n, 4), dtype=np.int32)
    for i in range(n):
        z = 0.45 + 0.01 * i
        u, v = 100 + 22 * i, 100 + 12 * i
        t = np.array([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z])
        R = rot(0.3 + 0.4 * i, (1.0, 0.5, 0.2 * i))
        for c in range(C):
            RT[i, c] = np.hstack([rot(0.01 * c, rs.randn(3)).dot(R), (t + 0.0005 * c * rs.randn(3))[:, None]])
        window[i] = [u - win // 2, v - win // 2, u - win // 2 + win - 1, v - win // 2 + win - 1]
    verts = torch.from_numpy(m["verts"].astype(np.float32)).to(dev)
    faces = torch.from_numpy(m["faces"]).to(dev)
    RT_d, K_d = torch.from_numpy(RT).to(dev), torch.from_numpy(K).to(dev)
    depth = evaluation.render_depth(verts, faces, RT_d[:, 0].contiguous(), K_d, H, W, 0.01)
    depth = torch.where(depth > 0, depth, torch.full_like(depth, 1.5))
    return verts, faces, RT_d, depth, K_d, torch.from_numpy(window).to(dev)


def timeit(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def graphed(fn):
    """fn() captured once in a graph (after a warm-up on a side stream) -> its replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return lambda g=g, keep=keep: g.replay()                       # the captured outputs live as long as the replay does


def open_lib(path):
    """A second library under the package's prototypes."""
    l = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = res, args
    return l


@contextlib.contextmanager
def using(handle, entries):
    """Inside, every _lib.call of the package goes to `handle` (None: the package's own library); `entries` is its cache of bound entries."""
    if handle is None:
        yield
        return
    _lib.lib()
    saved = _lib._lib, _lib._entries
    _lib._lib, _lib._entries = handle, entries
    try:
        yield
    finally:
        _lib._lib, _lib._entries = saved


def flat(out):
    """The tensors of a result (a tensor, a tuple or a dict of them) as [(name, tensor)]."""
    if isinstance(out, dict):
        return sorted(out.items())
    if isinstance(out, torch.Tensor):
        return [("0", out)]
    return [(str(i), t) for i, t in enumerate(out)]


def masks(B, N, dev, seed):
    g = torch.Generator().manual_seed(seed)
    single = torch.zeros((B, N), dtype=torch.uint8)
    single[:, N // 2] = 1
    return {"empty": torch.zeros((B, N), dtype=torch.uint8, device=dev), "single": single.to(dev),
            "full": torch.ones((B, N), dtype=torch.uint8, device=dev),
            "60%": (torch.rand((B, N), generator=g) < 0.6).to(torch.uint8).to(dev)}


def check_cases(dev):
    """-> (label, fn) pairs: fn() calls one pose entry on seeded inputs and returns its outputs."""
    M = 777
    nrm = unit_normals(M, dev)
    for B in (1, 3):
        for N in (1, 63, 64, 65, 257, 1024):
            res0, cld, model, _ = make(B, N, M, 0.3, seed=B * 10000 + N)
            cld[:, 6:9] = torch.nn.functional.normalize(torch.randn((B, 3, N), generator=torch.Generator().manual_seed(N)), dim=1).to(dev)
            g = torch.Generator().manual_seed(7 * N + B)
            weight = torch.rand((B, N), generator=g).to(dev)
            target = (model[res0["best_idx"].long()] + 0.001 * torch.randn((B, N, 3), generator=g).to(dev)).contiguous()
            for kind, mask in masks(B, N, dev, N + B).items():
                res = dict(mask=mask, best_idx=res0["best_idx"])
                tag = "B=%d N=%d mask=%s" % (B, N, kind)

                def icp_inputs(res=res):
                    return pose.solve_poses(res, cld, model, min_points=1)

                yield "kabsch_stats " + tag, lambda res=res: pose.kabsch_stats(res, cld, model)
                yield "kabsch_stats_weighted " + tag, lambda res=res: pose.kabsch_stats_weighted(res, cld, model, weight)
                yield "kabsch_stats_weighted target " + tag, lambda res=res: pose.kabsch_stats_weighted(res, cld, model, weight, target)
                yield "solve_poses " + tag, lambda res=res: pose.solve_poses(res, cld, model)
                yield "solve_poses_weighted " + tag, lambda res=res: pose.solve_poses_weighted(res, cld, model, weight, target)
                yield "ransac_poses H=33 " + tag, lambda res=res: pose.ransac_poses(res, cld, model, iters=33, seed=3)
                yield "ransac_poses H=33 fix_percent=0.3 " + tag, lambda res=res: pose.ransac_poses(res, cld, model, iters=33, fix_percent=0.3)
                yield "consensus_poses " + tag, lambda res=res: pose.consensus_poses(res, cld, model, seeds=8)
                yield "refine_icp " + tag, lambda res=res, f=icp_inputs: pose.refine_icp(*f(), cld, res["mask"], model, iters=3, tolerance=0.0)
                yield "refine_icp reject " + tag, lambda res=res, f=icp_inputs: pose.refine_icp(*f(), cld, res["mask"], model, iters=3,
                                                                                                reject_dist=0.05, min_points=1)
                yield "refine_icp_plane " + tag, lambda res=res, f=icp_inputs: pose.refine_icp_plane(*f(), cld, res["mask"], model, nrm, iters=3,
                                                                                                     tolerance=0.0)
                yield "refine_icp_plane gated " + tag, lambda res=res, f=icp_inputs: pose.refine_icp_plane(
                    *f(), cld, res["mask"], model, nrm, iters=3, tolerance=0.0, reject_dist=0.5, normal_gate=-0.5, huber=0.01)
    for vf64 in (False, True):
        verts, faces, RT, depth, K, window = depth_case(2, 3, 130, dev)
        v = verts.double() if vf64 else verts
        yield "refine_poses_depth 130x130 verts=%s" % v.dtype, lambda v=v: pose.refine_poses_depth(v, faces, RT, depth, K, window=window, iters=3,
                                                                                                 reject=0.01, near=0.01)
        yield "refine_poses_depth 130x130 huber min_cos verts=%s" % v.dtype, lambda v=v: pose.refine_poses_depth(
            v, faces, RT, depth, K, window=window, iters=3, reject=0.01, huber=0.002, min_cos=0.2, near=0.01)


def check_against(parent, entries, dev):
    """Every case from both libraries -> {entry: [arrays compared, arrays equal]}, the labels of the unequal ones."""
    tally, unequal = {}, []
    for label, fn in check_cases(dev):
        with using(parent, entries):
            want = flat(fn())
        got = flat(fn())
        t = tally.setdefault(label.split(" B=")[0].split(" 130x130")[0].split()[0], [0, 0])
        for (name, a), (_, b) in zip(want, got):
            same = a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
            t[0] += 1
            t[1] += int(same)
            if not same:
                unequal.append("%s [%s]" % (label, name))
    return tally, unequal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--M", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4, help="with --parent-lib: alternating rounds, parent then this library")
    ap.add_argument("--parent-lib", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pose_robust needs the GPU"
    dev = torch.device("cuda")
    parent, entries = (open_lib(a.parent_lib), {}) if a.parent_lib else (None, None)
    check = None
    if parent is not None:
        tally, unequal = check_against(parent, entries, dev)
        check = dict(arrays_compared_equal=tally, unequal=unequal, all_equal=not unequal)
        print(json.dumps(dict(check=check)), flush=True)
    res, cld, model, gt = make(a.B, a.N, a.M, 0.3)
    diam = float(torch.cdist(model[::8], model[::8]).max())
    add = {}
    for H in (20, 256, 1024):
        RT, valid = pose.solve_poses(res, cld, model, method="ransac", ransac_iters=H)
        add["ransac_H%d" % H] = float(pose.add_metric(RT, gt, model).max()) / diam
    RTk, vk = pose.solve_poses(res, cld, model)
    # plane rows: the same cloud with random unit normals (timing only; tolerance 0 keeps every crop running, and the random normals
    # keep it well-conditioned, so no crop is frozen early) and every option on
    nrm = unit_normals(a.M, dev)
    cld[:, 6:9] = torch.nn.functional.normalize(torch.randn(a.B, 3, a.N, device=cld.device), dim=1)
    kw = dict(tolerance=0.0, reject_dist=0.5, normal_gate=-0.5, huber=0.01)
    mask = res["mask"]
    _, it_pl, _, st_pl = pose.refine_icp_plane(RTk, vk, cld, mask, model, nrm, iters=10, **kw)
    assert int(it_pl.min()) == 10 and int(st_pl.max()) == 0, "a plane crop stopped early: the timing would be of a frozen crop"
    dverts, dfaces, dRT, ddepth, dK, dwin = depth_case(16, 8, 128, dev)
    few = max(a.reps // 10, 5)
    # name -> (call, repetitions, what one repetition is divided by); the graphed rows are captured under the library they time
    rows = {"kabsch": (lambda: pose.solve_poses(res, cld, model), a.reps, 1)}
    for H in (20, 256, 1024):
        rows["ransac_H%d" % H] = (lambda H=H: pose.solve_poses(res, cld, model, method="ransac", ransac_iters=H), a.reps, 1)
    rows["consensus_seeds8"] = (lambda: pose.consensus_poses(res, cld, model, seeds=8), few, 1)
    rows["icp_1_iteration"] = (lambda: pose.refine_icp(RTk, vk, cld, mask, model, iters=1), a.reps, 1)
    rows["icp_10_iterations_per_iteration"] = (lambda: pose.refine_icp(RTk, vk, cld, mask, model, iters=10, tolerance=0.0), few, 10)
    rows["icp_plane_1_iteration"] = (lambda: pose.refine_icp_plane(RTk, vk, cld, mask, model, nrm, iters=1, **kw), a.reps, 1)
    rows["icp_plane_10_iterations_per_iteration"] = (lambda: pose.refine_icp_plane(RTk, vk, cld, mask, model, nrm, iters=10, **kw), few, 10)
    rows["depth_refine_1_iteration"] = (lambda: pose.refine_poses_depth(dverts, dfaces, dRT, ddepth, dK, window=dwin, iters=1, reject=0.01,
                                                                       near=0.01), few, 1)
    graph_rows = {"icp_graph_per_iteration": rows["icp_10_iterations_per_iteration"][0],
                  "icp_plane_graph_per_iteration": rows["icp_plane_10_iterations_per_iteration"][0]}
    sides = [("parent", parent), ("this", None)] if parent is not None else [("this", None)]
    rounds = a.rounds if parent is not None else 1
    replay = {}
    for side, handle in sides:
        with using(handle, entries):
            replay[side] = {k: graphed(fn) for k, fn in graph_rows.items()}
    us = {side: {k: [] for k in list(rows) + list(graph_rows)} for side, _ in sides}
    for _ in range(rounds):
        for side, handle in sides:
            with using(handle, entries):
                for k, (fn, reps, per) in rows.items():
                    us[side][k].append(timeit(fn, reps) / per)
                # captured 10-iteration loops, replayed: the two metrics alternate, three passes each, the median is kept
                passes = {k: [] for k in graph_rows}
                for _ in range(3):
                    for k in graph_rows:
                        passes[k].append(timeit(replay[side][k], a.reps) / 10)
                for k, v in passes.items():
                    us[side][k].append(sorted(v)[1])
    med = {side: {k: float(np.median(v)) for k, v in d.items()} for side, d in us.items()}
    out = dict(shape=dict(B=a.B, N=a.N, M=a.M), reps=a.reps, us_per_call={k: round(v, 1) for k, v in med["this"].items()},
               max_add_over_diameter=add, device=torch.cuda.get_device_name(0), torch=torch.__version__,
               plane_over_point_graphed=round(med["this"]["icp_plane_graph_per_iteration"] / med["this"]["icp_graph_per_iteration"], 3),
               note="device events around back-to-back calls (host enqueue included: the calls are not graph-captured), except the "
                    "*_graph_per_iteration rows: a captured 10-iteration loop, replayed, the median of three passes")
    if parent is not None:
        table = {}
        for k in us["this"]:
            p, t = us["parent"][k], us["this"][k]
            table[k] = dict(parent_median=round(med["parent"][k], 2), parent_min=round(min(p), 2), parent_max=round(max(p), 2),
                            parent_spread=round(max(p) - min(p), 2), this_median=round(med["this"][k], 2), this_min=round(min(t), 2),
                            this_max=round(max(t), 2), this_spread=round(max(t) - min(t), 2),
                            within_parent_spread=bool(med["this"][k] <= med["parent"][k] + (max(p) - min(p))))
        out.update(check=check, rounds=rounds, against_parent_us=table, all_within_parent_spread=all(r["within_parent_spread"] for r in table.values()))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
