"""The four generic point-to-pixel fusions of the step (batch 16), each form alone on an idle chip: the 1x1 GEMM followed by
ops.gather_add_affine_act (two launches, the fp32 map written and read back in between) against ops.conv1x1_packed_gather_add_act
(one launch: gather, add, BN and ReLU in the GEMM's epilogue).  30 launches back to back, event-timed.  Development aid; under
rocprofv3 --pmc it gives both forms' kernels in one process."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from geometric_aware_dense_matching_amd import ops


def tm(fn, n=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


B = 16
# site, channels (Cin = Cout), map side, gathered points, packed operand only
SITES = (("ds stage 1", 128, 32, 128, False), ("ds stage 2", 512, 32, 32, False), ("ds stage 3", 1024, 32, 8, True), ("up stage 0", 256, 64, 32, True))
for name, C, H, n, only in SITES:
    x = torch.randn(B, C, H, H, device="cuda")
    xp = ops.conv3x3_pack_act(x)
    xp = ops.PackedAct(xp.buf.clone(), xp.shape)                  # outside the pool: no output of either form lands on it
    wpk = ops.gemm_pack_weight(torch.randn(C, C, device="cuda") / C ** 0.5)
    t = torch.randn(B, C, n, device="cuda")
    idx = torch.randint(0, n, (B, H * H), device="cuda", dtype=torch.int32)
    sc, sh = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
    keep = {}

    def gemm():
        keep["x"] = ops.gemm_bf16x3_map(xp, wpk, C).view(B, C, H * H)

    def tail():
        ops.gather_add_affine_act(keep["x"], t, idx, sc, sh, 1, 0.0, hw=(H, H), f32_out=not only)

    def pair():
        gemm()
        tail()

    def fused():
        ops.conv1x1_packed_gather_add_act(xp, wpk, C, t, idx, sc, sh, 1, hw=(H, H), f32_out=not only)

    a, b = tm(gemm), tm(tail)
    p, f = tm(pair), tm(fused)
    print("%s %4d x %d x %d, %s: GEMM %.1f us + gather_add_affine_act %.1f us (back to back %.1f us); one launch %.1f us"
          % (name, C, H, H, "packed only" if only else "fp32 + packed", a, b, p, f), flush=True)
