#!/usr/bin/env python
"""The MEASURED part of profiles/step_compare.md, nothing more (its yardstick column and its text are written by hand): runs the
per-parameter whole-step tests (tests/step_compare.py) with their figures printed, ten minutes at the most, or reads a pytest log
that holds them (`-s`), and prints the fixtures' lines and one table row per comparison.

    python tools/step_compare_report.py [pytest.log] > measured.md
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = ["tests/test_gpu_step_compare.py",
         "tests/test_gpu_train_graph.py::test_graphed_training_iterations_equal_the_eager_loop_per_tensor",
         "tests/test_gpu_train.py::test_training_step_under_ddp_and_syncbn_in_an_rccl_group_of_one_per_parameter",
         "tests/test_gpu_train.py::test_training_step_on_two_ranks_with_half_the_batch_each_equals_one_process_per_parameter"]
KNOWN = re.compile(r"(FFB6D fixture|DGCNN fixture|loss per step|USE_\w+|grouped against|DGCNN fused|graphed against|RCCL group of one per|two ranks per|seeded stale|FFB6D most|DGCNN most).*")
ROW = re.compile(r"^(?P<what>.+?):? +worst distance / bound (?P<ratio>[0-9.e+-]+) at (?P<name>[\w.]+)(?P<rest>.*)$")


def main():
    if len(sys.argv) > 1:
        text = open(sys.argv[1]).read()
    else:
        text = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-p", "no:cacheprovider"] + TESTS, cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600).stdout
    rows = []
    for line in text.splitlines():
        m = KNOWN.search(line)                    # behind pytest's progress characters
        if not m:
            continue
        line = m.group(0)
        if "%s" in line or "%." in line:          # a failing test's source listing
            continue
        if line.startswith(("FFB6D fixture", "DGCNN fixture", "loss per step", "seeded stale", "FFB6D most", "DGCNN most")):
            print("* " + line)
        m = ROW.match(line)
        if m:
            rows.append((m["what"].strip(), float(m["ratio"]), m["name"], m["rest"].strip(" ;")))
    print("\n| comparison | worst distance / bound | at | |\n|---|---|---|---|")
    for r in rows:
        print("| %s | %.3f | `%s` | %s |" % r)
    return 0 if rows else 1


if __name__ == "__main__":
    sys.exit(main())
