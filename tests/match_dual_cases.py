"""Seeded inputs for the dual-softmax matching tests (CPU and GPU); the descriptors are tests/match_twoway_cases.py's.

  SHAPES / MASKS / GAMMAS   the launch shapes, mask kinds and temperatures of tests/test_gpu_match_dual.py
  mask(...)                 u8[B,N] of one of the MASKS
  model_xyz(...)            f32[M,3] vertices within a 10 cm cube
"""
import numpy as np

import match_twoway_cases as mc

# (2,70,200): one partial row block per crop, a partial panel; (1,256,256): exactly one of each; (3,128,8193): 33 panels, the last one
# column wide; (2,300,256): two row blocks per crop, the second 44 rows long, the crop boundary off every multiple of 256 rows;
# (5,20,300): more crops inside 256 rows than the two-way kernel has LDS slots for, crops shorter than a wave tile
SHAPES = [(2, 70, 200), (1, 256, 256), (3, 128, 8193), (2, 300, 256), (5, 20, 300)]
MASKS = ["ones", "empty_crop", "single_point", "half"]
GAMMAS = [16.0, 40.0]


def mask(B, N, kind):
    """ones: every point; half: a seeded half; empty_crop: a seeded half with the last crop all off; single_point: a seeded half with
    one point of the last crop on."""
    rs = mc.rng("match_dual mask %d %d %s" % (B, N, kind))
    if kind == "ones":
        return np.ones((B, N), np.uint8)
    m = (rs.rand(B, N) < 0.5).astype(np.uint8)
    if kind == "half":
        return m
    m[B - 1] = 0
    if kind == "single_point":
        m[B - 1, rs.randint(N)] = 1
    else:
        assert kind == "empty_crop", kind
    return m


def model_xyz(M):
    return mc.rng("match_dual xyz %d" % M).uniform(-0.05, 0.05, (M, 3)).astype(np.float32)
