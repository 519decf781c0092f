#!/usr/bin/env python3
"""The end-to-end learnability record: trains the FFB6D variant on rendered frames of render.demo_mesh (`train_lm -data rendered`,
targets on the device) and evaluates `-state=test -data rendered` on 64 held-out rendered frames (another seed) before and after.
Reports the loss over the first and the last 50 steps and the ADD-0.1d recall (`ad_10` of the recall table: ADD below a tenth of
the object's diameter) with the mean ADD.  A record, not a test: whatever comes out is written down.  Run it under one `timeout`
of at most 15 minutes; it writes its section of profiles/render_frames.md and prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_render import OUT, write_section  # noqa: E402
from geometric_aware_dense_matching_amd import train_lm  # noqa: E402

MARK = "train_rendered_demo"


def evaluate(common, ckpt_dir, frames, batch):
    argv = ("-state=test -data rendered -checkpoint %s --batch-size %d --synthetic-items %d %s" % (ckpt_dir, batch, frames, common)).split()
    train_lm.test(train_lm.build_parser().parse_args(argv))
    table = train_lm.test.last_table
    (name, rec), = table.recalls.items()
    err = table.errors[name]
    return dict(frames=len(rec["ad_10"]), ad_10=float(np.mean(rec["ad_10"])), ad_5=float(np.mean(rec["ad_5"])),
                ad_2=float(np.mean(rec["ad_2"])), mean_ad_m=float(np.mean(err["ad"])), median_ad_m=float(np.median(err["ad"])))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=1500)
    p.add_argument("--batch-size", type=int, default=8)
    p.add_argument("--n-points", type=int, default=2048)
    p.add_argument("--n-mesh", type=int, default=1024)
    p.add_argument("--cls-id", type=int, default=1)
    p.add_argument("--out", type=str, default=OUT)
    args = p.parse_args()
    common = "-cls_id=%d --n-points %d --n-mesh %d" % (args.cls_id, args.n_points, args.n_mesh)
    with tempfile.TemporaryDirectory() as tmp:
        before = evaluate(common, os.path.join(tmp, "none"), 64, 16)
        argv = ("-state=train -data rendered --deterministic --batch-size %d --epochs 1 --save-every 1 --log-every 100 --synthetic-items %d "
                "--log-dir %s %s" % (args.batch_size, args.steps * args.batch_size, tmp, common)).split()
        t0 = time.time()
        trainer = train_lm.train(train_lm.build_parser().parse_args(argv))
        seconds = time.time() - t0
        after = evaluate(common, tmp, 64, 16)
        replaced = trainer._replaced_counter().tolist()
    hist = np.asarray(trainer.history, dtype=np.float64)
    k = min(50, len(hist))
    res = dict(steps=len(hist), batch=args.batch_size, n_points=args.n_points, n_mesh=args.n_mesh, seconds=round(seconds, 1),
               ms_per_step=round(1e3 * seconds / max(len(hist), 1), 1), first=dict(zip(("loss", "seg", "match"), hist[:k].mean(0).round(4).tolist())),
               last=dict(zip(("loss", "seg", "match"), hist[-k:].mean(0).round(4).tolist())), replaced=replaced, before=before, after=after)
    print(json.dumps(res))
    verdict = "rose" if after["ad_10"] > before["ad_10"] else "did NOT rise"
    text = """## tools/train_rendered_demo.py

FFB6D variant, `train_lm -state=train -data rendered` on `demo_mesh` frames: %d steps of batch %d (%d points, %d model vertices),
CyclicLR as `train_lm` sets it, %.1f s in all (%.1f ms per step with rendering, front end and targets); %d items replaced by their
batch's first valid one, %d in batches without a valid item.  Evaluation: `-state=test -data rendered`, 64 held-out frames (seed 1).

| | loss | seg | match |
|---|---|---|---|
| mean of the first %d steps | %.4f | %.4f | %.4f |
| mean of the last %d steps | %.4f | %.4f | %.4f |

| 64 held-out frames | ADD-0.1d recall | ADD-0.05d | ADD-0.02d | mean ADD (m) | median ADD (m) |
|---|---|---|---|---|---|
| before training (random weights) | %.3f | %.3f | %.3f | %.4f | %.4f |
| after training | %.3f | %.3f | %.3f | %.4f | %.4f |

The ADD-0.1d recall %s.  This is a record of one run, not a tuned result.
""" % (res["steps"], args.batch_size, args.n_points, args.n_mesh, seconds, res["ms_per_step"], replaced[0], replaced[1],
       k, *hist[:k].mean(0)[:3], k, *hist[-k:].mean(0)[:3],
       before["ad_10"], before["ad_5"], before["ad_2"], before["mean_ad_m"], before["median_ad_m"],
       after["ad_10"], after["ad_5"], after["ad_2"], after["mean_ad_m"], after["median_ad_m"], verdict)
    write_section(args.out, MARK, text)


if __name__ == "__main__":
    main()
