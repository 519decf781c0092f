"""Per-Function report of the training-step replay (tests/test_gpu_train_replay.py): records the steps once, compares every call with its
fp64 restatement and -- the reference-only yardstick -- the same restatement in fp32 torch with fp64, and prints the table of
profiles/train_replay.md (markdown) followed by every comparison that misses its tolerance.

    python tools/train_replay_report.py > table.md
"""
import collections
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_gpu_train_replay as steps_mod  # noqa: E402
import train_replay as tr  # noqa: E402

STEPS = steps_mod.STEPS + ("direct",)


def main():
    sink = steps_mod.record_steps()
    calls = collections.defaultdict(lambda: collections.defaultdict(int))
    info = collections.defaultdict(lambda: collections.defaultdict(int))
    worst = collections.defaultdict(lambda: [0.0, 0.0, 0.0])            # (class, kind) -> usual, scale-free, fp32 restatement (scale-free)
    raised, missed = {}, []
    for k, rec in enumerate(sink):
        ref, r32 = tr.reference(rec), tr.reference(rec, torch.float32)
        calls[rec.cls_name][rec.step] += 1
        for key in ("ties", "fragile"):
            info[rec.cls_name][key] += ref.info.get(key, 0)
        entry = tr.TABLE[rec.cls_name]
        for what, e1, e2, tol in tr.errors(rec, ref):
            kind, y = "buffers", 0.0
            if what.startswith("out"):
                kind, y = "forward", tr.scale_free_err(r32.outputs[int(what[3:])], ref.outputs[int(what[3:])])
            elif what.startswith("grad"):
                i = int(what[4:])
                kind, y = "gradients", 0.0 if i in entry.usual_only else tr.scale_free_err(r32.grads[i], ref.grads[i])
            w = worst[(rec.cls_name, kind)]
            w[0], w[1], w[2] = max(w[0], e1), max(w[1], e2), max(w[2], y)
            if not (e1 <= tol and e2 <= tol):
                missed.append("%s %s call %d %s: %.3e / %.3e > %.1e (fp32 restatement %.3e)" % (rec.cls_name, rec.step, k, what, e1, e2, tol, y))
        for i, t in entry.grad_tol.items():
            if t > entry.bwd and ref.grads[i] is not None and rec.grads is not None and rec.grads[i] is not None:
                r = raised.setdefault((rec.cls_name, i), [t, 0.0, 0.0])
                r[1] = max(r[1], tr.scale_free_err(rec.grads[i], ref.grads[i]) if i not in entry.usual_only else tr.rel_err(rec.grads[i], ref.grads[i]))
                r[2] = max(r[2], tr.scale_free_err(r32.grads[i], ref.grads[i]) if i not in entry.usual_only else tr.rel_err(r32.grads[i], ref.grads[i]))
        missed += ["%s %s call %d: %s" % (rec.cls_name, rec.step, k, f) for f in tr.structure_failures(rec, ref)]
        rec.cache.clear()
    fmt = lambda w: "%.1e / %.1e (%.1e)" % tuple(w) if w else "-"
    print("| Function | calls: %s | forward: usual / scale-free (fp32 restatement) | gradients | buffers | ties | tolerance fwd, bwd |" % " / ".join(STEPS))
    print("|---|---|---|---|---|---|---|")
    for name in sorted(tr.TABLE):
        e = tr.TABLE[name]
        print("| `%s` | %s | %s | %s | %s | %d | %.0e, %.0e |" % (
            name, " / ".join(str(calls[name][s]) for s in STEPS), fmt(worst.get((name, "forward"))), fmt(worst.get((name, "gradients"))),
            ("%.1e" % worst[(name, "buffers")][1]) if (name, "buffers") in worst else "-", info[name]["ties"], e.fwd, e.bwd))
    print()
    print("Fragile pre-activations inside `_EdgeBlockTrain` (|z| < 1e-6): %d" % info["_EdgeBlockTrain"]["fragile"])
    print()
    print("| gradient with its own tolerance | tolerance | kernel | fp32 restatement |")
    print("|---|---|---|---|")
    for (name, i), (t, e, y) in sorted(raised.items()):
        print("| `%s` argument %d | %.1e | %.1e | %.1e |" % (name, i, t, e, y))
    print()
    print("comparisons that miss their tolerance: %d" % len(missed))
    for m in missed:
        print("    " + m)


if __name__ == "__main__":
    main()
