"""Timing of the pose stage's fits at the headline shape (B = 16 crops, N = 2048 points, M = 8192 model vertices): the Kabsch fit,
RANSAC at H = 20 / 256 / 1024 hypotheses and one ICP iteration of either metric (point-to-point, point-to-plane), eager and as a
graph-captured 10-iteration loop.  Correspondences: a known pose + 1 mm noise with 30 % of the points
in a background cluster.  Device-event timing of back-to-back calls after a warm-up; also checks that every RANSAC pose is within
1 % of the object diameter of the ground truth (ADD).
    python tools/bench_pose_robust.py [--reps 200] [--out profiles/pose_robust_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from geometric_aware_dense_matching_amd import pose  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--M", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pose_robust needs the GPU"
    res, cld, model, gt = make(a.B, a.N, a.M, 0.3)
    diam = float(torch.cdist(model[::8], model[::8]).max())
    rows = {"kabsch": timeit(lambda: pose.solve_poses(res, cld, model), a.reps)}
    add = {}
    for H in (20, 256, 1024):
        rows["ransac_H%d" % H] = timeit(lambda: pose.solve_poses(res, cld, model, method="ransac", ransac_iters=H), a.reps)
        RT, valid = pose.solve_poses(res, cld, model, method="ransac", ransac_iters=H)
        add["ransac_H%d" % H] = float(pose.add_metric(RT, gt, model).max()) / diam
    RTk, vk = pose.solve_poses(res, cld, model)
    rows["icp_1_iteration"] = timeit(lambda: pose.refine_icp(RTk, vk, cld, res["mask"], model, iters=1), a.reps)
    rows["icp_10_iterations_per_iteration"] = timeit(lambda: pose.refine_icp(RTk, vk, cld, res["mask"], model, iters=10, tolerance=0.0),
                                                     max(a.reps // 10, 5)) / 10
    # plane rows: the same cloud with random unit normals (timing only; tolerance 0 keeps every crop running, and the random normals
    # keep it well-conditioned, so no crop is frozen early) and every option on
    rs = np.random.RandomState(1)
    nrm = rs.randn(a.M, 3)
    nrm = torch.from_numpy((nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)).to(model.device)
    cld[:, 6:9] = torch.nn.functional.normalize(torch.randn(a.B, 3, a.N, device=cld.device), dim=1)
    kw = dict(tolerance=0.0, reject_dist=0.5, normal_gate=-0.5, huber=0.01)
    mask = res["mask"]
    rows["icp_plane_1_iteration"] = timeit(lambda: pose.refine_icp_plane(RTk, vk, cld, mask, model, nrm, iters=1, **kw), a.reps)
    rows["icp_plane_10_iterations_per_iteration"] = timeit(lambda: pose.refine_icp_plane(RTk, vk, cld, mask, model, nrm, iters=10, **kw),
                                                           max(a.reps // 10, 5)) / 10
    _, it_pl, _, st_pl = pose.refine_icp_plane(RTk, vk, cld, mask, model, nrm, iters=10, **kw)
    assert int(it_pl.min()) == 10 and int(st_pl.max()) == 0, "a plane crop stopped early: the timing would be of a frozen crop"
    # captured 10-iteration loops, replayed: the two metrics alternate, three passes each, the median is reported and all are kept
    point_fn = graphed(lambda: pose.refine_icp(RTk, vk, cld, mask, model, iters=10, tolerance=0.0))
    plane_fn = graphed(lambda: pose.refine_icp_plane(RTk, vk, cld, mask, model, nrm, iters=10, **kw))
    passes = {"icp_graph_per_iteration": [], "icp_plane_graph_per_iteration": []}
    for _ in range(3):
        passes["icp_graph_per_iteration"].append(timeit(point_fn, a.reps) / 10)
        passes["icp_plane_graph_per_iteration"].append(timeit(plane_fn, a.reps) / 10)
    for k, v in passes.items():
        rows[k] = sorted(v)[1]
    out = dict(shape=dict(B=a.B, N=a.N, M=a.M), reps=a.reps, us_per_call={k: round(v, 1) for k, v in rows.items()},
               max_add_over_diameter=add, device=torch.cuda.get_device_name(0), torch=torch.__version__,
               graph_passes_us={k: [round(x, 1) for x in v] for k, v in passes.items()},
               plane_over_point_graphed=round(rows["icp_plane_graph_per_iteration"] / rows["icp_graph_per_iteration"], 3),
               note="device events around back-to-back calls (host enqueue included: the calls are not graph-captured), except the "
                    "*_graph_per_iteration rows: a captured 10-iteration loop, replayed")
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
