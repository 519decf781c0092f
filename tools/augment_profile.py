#!/usr/bin/env python3
"""Times the crop augmentation (ops.augment_crops, csrc/gdm_augment.hip) on the GPU and prints the table of
profiles/augment.md: `augment_crops` for 16 crops at S = 256 against a bank of 480 x 640 frames, at the reference's stage probabilities
(the calls of a window walk through `--reps` seeds, so the mix of stages is that of 16 x reps crops) and with every stage forced on
(gdm_augment_force_all_stages, a measurement aid), and the YCB-V item (make_inputs_from_boxes, depth_fill="multiscale",
sampler="hash", jitter="hash", N = 2048, no pyramid) with and without augmentation.  Device events around `reps` calls, `rounds`
windows after a warm-up of every variant; the median window and the spread are printed.

    python tools/augment_profile.py [--reps 50] [--rounds 7] [--out profiles/augment.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geometric_aware_dense_matching_amd import _lib, frontend, ops, synthetic  # noqa: E402

B, H, W, S, N, NB = 16, 480, 640, 256, 2048, 8


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_profile.py needs the GPU: a time taken elsewhere says nothing")
    rs = np.random.RandomState(0)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    fr = [synthetic.make_frame(rs) for _ in range(B)]
    det = [synthetic.make_box_mask(rs) for _ in range(B)]
    K = np.stack([synthetic.LM_K for _ in range(B)]).astype(np.float32)
    f = dict(rgb_u8=cuda(np.stack([x[1] for x in fr])), depth=cuda(np.stack([x[0] for x in fr])), K=cuda(K),
             bbox_xyxy=cuda(np.stack([x[0] for x in det])), mask=cuda(np.stack([x[1] for x in det])))
    bank = (cuda(rs.randint(0, 256, size=(NB, H, W, 3)).astype(np.uint8)), cuda(rs.uniform(0.5, 1.5, size=(NB, H, W)).astype(np.float32)),
            cuda(rs.choice(np.array([0, 9, 255], np.uint8), size=(NB, H, W))))
    center, scale = frontend.dzi_boxes(f["bbox_xyxy"], (H, W))
    crop = frontend.crop_from_boxes(f["rgb_u8"], f["depth"], None, f["K"], center, scale, S, mask=f["mask"])
    lib = _lib.lib()
    pasted = ops.augment_crops(crop["rgb"], crop["depth"], crop["mask"], bank, None, 0)          # what the augmented item's fill reads
    filled = {"raw": frontend.fill_depth(crop["depth"]), "pasted": frontend.fill_depth(pasted[1])}
    normals = {k: frontend.depth_normals(v, f["K"]) for k, v in filled.items()}
    for k, v in filled.items():
        print("%s crop: %.1f %% of the pixels have depth, %.1f %% after the fill" %
              (k, 100 * float(((crop["depth"] if k == "raw" else pasted[1]) > 1e-6).float().mean()), 100 * float((v > 1e-6).float().mean())))

    def sample(k, i):
        return ops.sample_assemble(filled[k], crop["dpt_xyz"], crop["rgb"], normals[k], N, mask=crop["mask"], seed=i)

    def item(i, augment):
        return frontend.make_inputs_from_boxes(f["rgb_u8"], f["depth"], f["K"], f["bbox_xyxy"], S, N, mask=f["mask"], train=True,
                                               depth_fill="multiscale", sampler="hash", jitter="hash", seed=i, augment=augment,
                                               build_pyramid=False)

    variants = {
        "augment_crops, reference probabilities": lambda i: ops.augment_crops(crop["rgb"], crop["depth"], crop["mask"], bank, None, i),
        "augment_crops, no background": lambda i: ops.augment_crops(crop["rgb"], crop["depth"], None, None, None, i),
        "augment_crops, every stage forced on": lambda i: ops.augment_crops(crop["rgb"], crop["depth"], crop["mask"], bank, None, i),
        "fill_depth multiscale of the crop's depth": lambda i: frontend.fill_depth(crop["depth"]),
        "fill_depth multiscale of the pasted depth": lambda i: frontend.fill_depth(pasted[1]),
        "sample_assemble on the filled crop": lambda i: sample("raw", i),
        "sample_assemble on the filled pasted crop": lambda i: sample("pasted", i),
        "YCB-V item without augmentation": lambda i: item(i, None),
        "YCB-V item with augmentation": lambda i: item(i, dict(background=bank, enable=None)),
    }
    times = {k: [] for k in variants}
    for rnd in range(args.rounds + 1):                                        # round 0 is the warm-up of every variant
        for name, fn in variants.items():                                     # the variants alternate inside every round
            lib.gdm_augment_force_all_stages(1 if "forced" in name else 0)
            t = window(fn, args.reps if rnd else 5)
            lib.gdm_augment_force_all_stages(0)
            if rnd:
                times[name].append(t)
    draws = [d for s in range(args.reps) for d in frontend.augment_draws_numpy(B, s)]
    halos = [max(d["passes"][0]["halo"], d["passes"][1]["halo"] if d["second"] else 0) for d in draws]
    res = dict(shape=dict(B=B, S=S, N=N, bank=[NB, H, W]), reps=args.reps, rounds=args.rounds, device=torch.cuda.get_device_name(0),
               launches_per_augment_call=2, crops_with_a_halo=float(np.mean([h > 0 for h in halos])), mean_halo=float(np.mean(halos)),
               ms={k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in times.items()})
    print("| what | ms per call, median of %d windows of %d calls | min .. max |" % (args.rounds, args.reps))
    print("|---|---|---|")
    for k, v in res["ms"].items():
        print("| %s | %.3f | %.3f .. %.3f |" % (k, v["median"], v["min"], v["max"]))
    print("crops that draw a stencil stage in the pass that sets their halo: %.0f %%; mean halo %.1f pixels" %
          (100 * res["crops_with_a_halo"], res["mean_halo"]))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
