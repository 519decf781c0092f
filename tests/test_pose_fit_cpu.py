"""CPU: the pose-fit fragment (csrc/gdm_kabsch_fit.inc: Horn's quaternion by fp64 Jacobi, shared by the Kabsch solve, RANSAC and
ICP kernels), compiled unchanged for the host (oracle/kabsch_fit_host.cpp), against numpy's SVD with the reflection fix
(oracle/pose_ref.py best_fit_transform) on 17 input families of 2000 seeded cases each, and once more under AddressSanitizer + UBSan.

Bounds (derived, not measured): the fragment's R entries are fp32 roundings of an fp64 orthonormal matrix (error <= 2^-25 each), so
|R R^T - I| and |det - 1| <= 2e-7; the objective trace(R H) is within 2e-7 s1 of the SVD optimum; where that optimum is unique
((s2 + sign s3) / s1 > 1e-3) R agrees to 1e-7 and t to one fp32 ulp of max(1, |t|)."""
import numpy as np
import pytest

from oracle import kabsch_fit, pose_cases, pose_ref

CASES_PER_SIZE = 400                                 # x 5 sizes = 2000 cases per family
SEED = 20300


def _cases(fam):
    """-> the family's (A, B) stacks, one per size."""
    rs = np.random.RandomState(SEED + pose_cases.FAMILIES.index(fam))
    if fam.startswith("dup"):
        return [pose_cases.family(fam, rs, len(pose_cases.SIZES) * CASES_PER_SIZE, 4)]
    return [pose_cases.family(fam, rs, CASES_PER_SIZE, n) for n in pose_cases.SIZES]


@pytest.mark.parametrize("fam", pose_cases.FAMILIES)
def test_fit_fragment_vs_svd(fam):
    total = 0
    for A, B in _cases(fam):
        RT = kabsch_fit.fit(kabsch_fit.stats_of(A, B))
        pose_ref.check_fit(RT, A, B, fam in pose_cases.UNIQUE)
        total += len(A)
    assert total >= 2000


def test_fit_fragment_under_sanitizers():
    """Every family once more through the -fsanitize=address,undefined build: it must run clean and give the same bits."""
    stats = np.concatenate([kabsch_fit.stats_of(A, B) for fam in pose_cases.FAMILIES for A, B in _cases(fam)])
    assert len(stats) >= 17 * 2000
    got, rc, err = kabsch_fit.fit_sanitized(stats)
    assert rc == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-2000:]
    assert np.array_equal(got, kabsch_fit.fit(stats))
