#!/usr/bin/env python3
"""Times the textured frame renderer (gdm_render_frames_tex_hip) at the size training uses -- 16 frames of 480 x 640,
S = 4 slots: three render.demo_mesh(level=5, textured=True) objects (20480 faces each), each with a 1024 x 1024 hash image as its
texture, and the backdrop plane -- beside the untextured entry on the same meshes and poses (the same scene packed without its
textures: grey objects), and the build of one 1024 x 1024 pyramid (gdm_texture_mips_hip).  Device events after warm-up; timing is
reported, not gated.  Prints one JSON line and writes its section of profiles/render_textured.md.  Kernel times come from a run of
their own under `rocprofv3 --kernel-trace --stats -- python tools/bench_render_textured.py --iters 5 --no-write`: there the textured
and the untextured resolve are two instances of one kernel and show as two rows."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_render import timed, write_section  # noqa: E402
from geometric_aware_dense_matching_amd import render, synthetic, texture  # noqa: E402

H, W, N, S, TEX = 480, 640, 16, 4, 1024
OUT = os.path.join(ROOT, "profiles", "render_textured.md")
MARK = "bench_render_textured"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--level", type=int, default=5)
    p.add_argument("--no-write", action="store_true")
    p.add_argument("--out", type=str, default=OUT)
    args = p.parse_args()
    K = synthetic.LM_K.astype(np.float64)
    meshes = []
    for s in range(3):
        m = render.demo_mesh(level=args.level, seed=s, textured=True, tex_size=16)
        m["texture"] = np.random.RandomState(s).randint(0, 256, size=(TEX, TEX, 3)).astype(np.uint8)
        meshes.append(m)
    meshes.append(render.backdrop_mesh(K, H, W, z=1.5))
    scene = render.SceneMeshes([render._as_mesh(m) for m in meshes])
    plain = render.SceneMeshes([render._as_mesh(m)[:4] for m in meshes])
    slot_obj, RT = render.sample_scene_poses(N, S, 0, K, H, W, (0.4, 1.0), 0, (1,), 3, 0.055)
    slot_obj[:, 2] = 2
    dev = scene.device
    so, RTd, Kd = torch.from_numpy(slot_obj).to(dev), torch.from_numpy(RT).to(dev), torch.from_numpy(K).to(dev)
    light = torch.tensor([[0.0, 0.0, -1.0]], dtype=torch.float64, device=dev).expand(N, 3).contiguous()

    out = render.render_frames(scene, so, RTd, Kd, H, W, light=light)
    ref = render.render_frames(plain, so, RTd, Kd, H, W, light=light)
    same_geometry = all(bool(torch.equal(out[k], ref[k])) for k in ("depth", "inst", "face", "px_all", "px_vis", "bbox_vis"))
    textured_px = int(((out["inst"] > 0) & (out["inst"] < S)).sum())
    image = torch.from_numpy(meshes[0]["texture"]).to(dev)
    tex = timed(lambda: render.render_frames(scene, so, RTd, Kd, H, W, light=light), args.iters)
    unt = timed(lambda: render.render_frames(plain, so, RTd, Kd, H, W, light=light), args.iters)
    mips = timed(lambda: texture.build_mips(image), args.iters)
    res = dict(frames=N, H=H, W=W, S=S, faces=int(scene.faces.shape[0]), texture=[TEX, TEX], tex_mib=round(scene.tex.numel() / 2 ** 20, 1),
               textured_px=textured_px, covered_px=int((out["inst"] > 0).sum()), same_geometry=same_geometry,
               textured_ms=[round(t, 3) for t in tex], untextured_ms=[round(t, 3) for t in unt], mips_ms=[round(t, 4) for t in mips],
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res))
    if args.no_write:
        return
    text = """## tools/bench_render_textured.py

%d frames of %d x %d, S = %d: three textured `demo_mesh(level=%d)` objects, a %d x %d image each (%.1f MiB of texels with the
mips), and the backdrop, %d faces in all; %d of the %d covered pixels show a textured object; %s.  Device events after 5 warm-up
calls, three windows of %d calls each (min / median / max of the per-call mean).  Depth, masks, faces and statistics of the two calls
are the same bytes: %s.

| what | ms |
|---|---|
| `render.render_frames`, textured (`gdm_render_frames_tex_hip`) | %.3f / %.3f / %.3f |
| `render.render_frames` of the same meshes and poses without textures (`gdm_render_frames_hip`) | %.3f / %.3f / %.3f |
| `texture.build_mips` of one %d x %d image (`gdm_texture_mips_hip`, %d launches) | %.4f / %.4f / %.4f |
""" % (N, H, W, S, args.level, TEX, TEX, res["tex_mib"], res["faces"], textured_px, res["covered_px"], res["device"], args.iters,
       same_geometry, *tex, *unt, TEX, TEX, texture.full_levels(TEX, TEX), *mips)
    write_section(args.out, MARK, text)


if __name__ == "__main__":
    main()
