#!/usr/bin/env python3
"""Times the frame renderer (render.render_frames, gdm_render.hip) at the size training uses -- 16 frames of 480 x 640, S = 4 slots:
three render.demo_mesh(level=5) objects (20480 faces each) and the backdrop plane -- from device events after warm-up, beside the
depth-only pass of the same triangles and poses (ops.render_depth once per slot: the floor, since it walks the same coverage and
writes 4 bytes per covered pixel where the renderer writes 8 and then resolves), and as a share of the 43-46 ms training step.
Also timed: the same call with every slot empty (the clear and the resolve of empty layers alone), which says how much of the call
the visibility pass and the shading are.  Writes its section of profiles/render_frames.md and prints one JSON line.  Kernel times
come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/bench_render.py --iters 5 --no-write`."""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from geometric_aware_dense_matching_amd import ops, render, synthetic  # noqa: E402

H, W, N, S = 480, 640, 16, 4
STEP_MS = (43.0, 46.0)
OUT = os.path.join(ROOT, "profiles", "render_frames.md")
MARK = "bench_render"


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(3):                                                     # three windows: the spread is reported with the median
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / iters)
    return sorted(times)


def write_section(path, mark, text):
    """Replaces (or appends) the section between <!-- mark --> and <!-- /mark --> of a markdown file shared by two tools."""
    body = open(path).read() if os.path.exists(path) else "# Rendered training frames (DESIGN.md 6p)\n"
    block = "<!-- %s -->\n%s\n<!-- /%s -->\n" % (mark, text.rstrip(), mark)
    pat = re.compile(r"<!-- %s -->.*?<!-- /%s -->\n" % (mark, mark), flags=re.S)
    body = pat.sub(lambda _: block, body) if pat.search(body) else body.rstrip() + "\n\n" + block
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(body)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--level", type=int, default=5)
    p.add_argument("--no-write", action="store_true")
    p.add_argument("--out", type=str, default=OUT, help="the markdown file whose bench_render section is rewritten")
    args = p.parse_args()
    K = synthetic.LM_K.astype(np.float64)
    meshes = [render.demo_mesh(level=args.level, seed=s) for s in range(3)]
    meshes.append(render.backdrop_mesh(K, H, W, z=1.5))
    scene = render.SceneMeshes([render._as_mesh(m) for m in meshes])
    slot_obj, RT = render.sample_scene_poses(N, S, 0, K, H, W, (0.4, 1.0), 0, (1,), 3, 0.055)
    slot_obj[:, 2] = 2                                                     # one object per slot over the batch: the floor below needs it
    dev = scene.device
    so, RTd, Kd = torch.from_numpy(slot_obj).to(dev), torch.from_numpy(RT).to(dev), torch.from_numpy(K).to(dev)
    light = torch.tensor([[0.0, 0.0, -1.0]], dtype=torch.float64, device=dev).expand(N, 3).contiguous()
    empty = torch.full_like(so, -1)

    out = render.render_frames(scene, so, RTd, Kd, H, W, light=light)
    covered = int((out["inst"] > 0).sum())
    px_all = int(out["px_all"].sum())
    full = timed(lambda: render.render_frames(scene, so, RTd, Kd, H, W, light=light), args.iters)
    bare = timed(lambda: render.render_frames(scene, empty, RTd, Kd, H, W, light=light), args.iters)

    per_obj = []                                                           # the parent's depth pass on the same triangles and poses
    for s in range(S):
        o = int(slot_obj[0, s])
        f0, f1 = scene.obj_face0[o], scene.obj_face0[o + 1]
        per_obj.append((scene.verts, scene.faces[f0:f1].contiguous(), RTd[:, s].contiguous()))

    def depth_only():
        return [ops.render_depth(v, f, rt, Kd, H, W, render.NEAR) for v, f, rt in per_obj]

    layers = torch.stack(depth_only(), dim=1)                              # [N,S,H,W]: the renderer's depth is their minimum
    layers = torch.where(layers > 0, layers, torch.full_like(layers, float("inf"))).amin(dim=1)
    same_depth = bool(torch.equal(torch.where(torch.isinf(layers), torch.zeros_like(layers), layers), out["depth"]))
    floor = timed(depth_only, args.iters)

    med = lambda t: t[1]  # noqa: E731
    res = dict(frames=N, H=H, W=W, S=S, faces=int(scene.faces.shape[0]), covered_px=covered, layer_px=px_all,
               render_frames_ms=[round(t, 3) for t in full], empty_slots_ms=[round(t, 3) for t in bare],
               render_depth_floor_ms=[round(t, 3) for t in floor], ratio_to_floor=round(med(full) / med(floor), 2),
               share_of_step=[round(med(full) / s, 3) for s in STEP_MS[::-1]], depth_equals_min_of_layers=same_depth,
               keys_mib=round(N * S * H * W * 8 / 2 ** 20, 1), device=torch.cuda.get_device_name(0))
    print(json.dumps(res))
    if args.no_write:
        return
    dominant = ("the visibility pass and the shading of won pixels" if med(full) - med(bare) > med(bare)
                else "the clear and the resolve of the layers")
    text = """## tools/bench_render.py

%d frames of %d x %d, S = %d: three `demo_mesh(level=%d)` objects and the backdrop, %d faces in all; %d pixels covered in the
frames, %d in the slot layers (`px_all`); %s.  Device events after 5 warm-up calls, three windows of %d calls each (min / median /
max of the per-call mean); %.1f MiB of keys.

| what | ms per %d frames |
|---|---|
| `render.render_frames` (clear, visibility, resolve) | %.3f / %.3f / %.3f |
| the same call with every slot empty (clear + resolve of empty layers) | %.3f / %.3f / %.3f |
| `ops.render_depth` of the same triangles and poses, once per slot (the depth-only floor) | %.3f / %.3f / %.3f |

The renderer takes %.2f times the depth-only floor and %.1f-%.1f %% of a 43-46 ms training step.  The depth image equals the
minimum of the four depth-only layers bit for bit: %s.  The call with empty slots costs %.3f ms of the %.3f, so %s take(s) most of it.
There is no pass mark on time: nothing in the parent produces such frames.
""" % (N, H, W, S, args.level, res["faces"], covered, px_all, res["device"], args.iters, res["keys_mib"], N, *full, *bare, *floor,
       res["ratio_to_floor"], 100 * med(full) / STEP_MS[1], 100 * med(full) / STEP_MS[0], same_depth, med(bare), med(full), dominant)
    write_section(args.out, MARK, text)


if __name__ == "__main__":
    main()
