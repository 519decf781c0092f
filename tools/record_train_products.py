#!/usr/bin/env python
"""Record which engine runs each product of every 1x1 training layer shape (tests/train_products.py) and write the golden files
tests/golden/train_products.json (needs the GPU; nothing is computed, it takes seconds) and tests/golden/train_products_fits.json
(--fits: the CPU is enough).  Run it on the commit whose decisions are to be pinned, BEFORE a change of ops.py's routing.

  python tools/record_train_products.py            # both files; the shapes of the recorded training steps are taken afresh
  python tools/record_train_products.py --fits     # the 2 GiB answers alone
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import train_products as tp  # noqa: E402


def replay_shapes():
    """[entry, B, Cin, Cout, n, bias] of every call the four recorded training steps of tests/test_gpu_train_replay.py make."""
    import test_gpu_train_replay as replay
    from geometric_aware_dense_matching_amd import ops
    with tp.noting_entries(ops) as calls:
        replay.record_steps()
    return [list(c) for c in sorted({tuple(c[:6]) for c in calls})]


def _dump(v, depth=0):
    """JSON with one row per line: dictionaries opened to two levels, lists of lists to one."""
    if isinstance(v, dict) and depth < 3:
        return "{\n" + ",\n".join("%s: %s" % (json.dumps(k), _dump(v[k], depth + 1)) for k in sorted(v)) + "\n}"
    if isinstance(v, list) and v and isinstance(v[0], list):
        return "[\n" + ",\n".join(json.dumps(i) for i in v) + "\n]"
    return json.dumps(v)


def write(name, doc):
    with open(os.path.join(tp.GOLDEN, name), "w") as f:
        f.write(_dump(doc) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fits", action="store_true", help="write train_products_fits.json only (no GPU)")
    args = ap.parse_args()
    from geometric_aware_dense_matching_amd import ops, settings
    if not args.fits:
        replay = replay_shapes()
        shapes = sorted(set(tp.synthetic_grid()) | set(tp.TEST_SHAPES) | {tuple(s[1:5]) for s in replay})
        write("train_products.json", {"letters": tp.__doc__.split("\n\n")[1], "columns": ["%s%s %s" % (e, "+bias" if b else "", lay) for e, b, lay in tp.columns()],
                                      "replay_calls": replay, "rows": tp.record_all(ops, settings, shapes)})
    else:
        shapes = sorted(tp.shape_of(k) for k in tp.load("train_products.json")["rows"][""])
    fits = {}
    for s in shapes + tp.LIMIT_SHAPES:
        row = ""
        for off in ("", "USE_MFMA_GEMM_TRAIN"):
            with tp.switched_off(settings, off):
                row += "FT"[tp.supported(ops, settings, s + (1, True))]
        fits[tp.key(s)] = row
    write("train_products_fits.json", {"what": "per B,Cin,Cout,n: do the operands of the three products fit (T/F), at the defaults and with "
                                               "USE_MFMA_GEMM_TRAIN off; supported: ops.conv1x1_train_supported per "
                                               "[B, Cin, Cout, n, kernel size, USE_GEMM_CONV1X1_TRAIN]",
                                       "fits": fits, "supported": [list(c) + [tp.supported(ops, settings, c)] for c in tp.supported_cases()]})


if __name__ == "__main__":
    main()
