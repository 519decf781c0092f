#!/usr/bin/env python3
"""knn_ref_cases.npz: the neighbour indices the compiled reference nanoflann (oracle/_ref/libknn_ref.so, `make -C oracle ref`)
returns for the inputs of tests/test_oracle_knn.py::test_oracle_equals_compiled_reference and
tests/test_gpu_ops.py::test_knn_reference_parity_tie_free, so that both tests run where the compiled reference is absent.
The inputs are not stored: each test regenerates them from its seed."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import knn as oknn  # noqa: E402

ORACLE_CASES = [(2048, 2048, 16), (512, 4096, 1), (4096, 512, 16), (32, 32, 16), (8, 1024, 1)]


def oracle_case_inputs(S, Q, K):
    """test_oracle_equals_compiled_reference's inputs."""
    rs = np.random.RandomState(S + Q + K)
    return rs.rand(2, S, 3).astype(np.float32), rs.rand(2, Q, 3).astype(np.float32)


def tie_free_inputs():
    """test_knn_reference_parity_tie_free's inputs (K = 16)."""
    rs = np.random.RandomState(11)
    return rs.rand(1, 2048, 3).astype(np.float32), rs.rand(1, 512, 3).astype(np.float32)


def main():
    assert oknn.have_ref(), "oracle/_ref/libknn_ref.so not built (make -C oracle ref)"
    out = {}
    for S, Q, K in ORACLE_CASES:
        sup, qry = oracle_case_inputs(S, Q, K)
        out["oracle_S%d_Q%d_K%d" % (S, Q, K)] = oknn.ref_knn_batch(sup, qry, K).astype(np.int16)
    sup, qry = tie_free_inputs()
    out["tie_free_K16"] = oknn.ref_knn_batch(sup, qry, 16).astype(np.int16)
    np.savez_compressed(os.path.join(HERE, "knn_ref_cases.npz"), **out)


if __name__ == "__main__":
    main()
