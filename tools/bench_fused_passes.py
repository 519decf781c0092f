"""The three passes the image branch no longer makes, each form alone on an idle chip: the 64-channel fusion + `final` as two launches
vs ops.conv64_gather_add_final (128 x 128, batch 16), and ops.gather_add_affine_act with / without its fp32 store at
1024 x 32 x 32 and 256 x 64 x 64.  Development aid."""
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


B, n = 16, 128
m = 128 * 128
x = torch.randn(B, 64, m, device="cuda")
wpk = ops.pack_rows64(torch.randn(64, 64, device="cuda") * 0.2)
t = torch.randn(B, n, 64, device="cuda")
idx = torch.randint(0, n, (B, m), device="cuda", dtype=torch.int32)
sc, sh = torch.rand(64, device="cuda") + 0.5, torch.randn(64, device="cuda")
wf, bf = torch.randn(64, 64, 1, 1, device="cuda") * 0.3, torch.randn(64, device="cuda")
fuse = lambda: ops.conv64_gather_add_act_mfma(x, wpk, t, idx, sc, sh, 1, 0.0, t_point_major=True)
y = fuse().view(B, 64, 128, 128)
t_fuse, t_final = tm(fuse), tm(lambda: ops.conv1x1_logsoftmax(y, wf, bf))
t_one = tm(lambda: ops.conv64_gather_add_final(x, wpk, t, idx, sc, sh, 1, 0.0, wf, bf))
print("fusion %.1f us + final %.1f us = %.1f us; one launch %.1f us (201 MB -> 134 MB)" % (t_fuse, t_final, t_fuse + t_final, t_one))
for C, H in ((1024, 32), (256, 64)):
    xg = torch.randn(B, C, H * H, device="cuda")
    tg = torch.randn(B, C, n, device="cuda")
    ig = torch.randint(0, n, (B, H * H), device="cuda", dtype=torch.int32)
    s1, s2 = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
    a = tm(lambda: ops.gather_add_affine_act(xg, tg, ig, s1, s2, 1, 0.0, hw=(H, H)))
    b = tm(lambda: ops.gather_add_affine_act(xg, tg, ig, s1, s2, 1, 0.0, hw=(H, H), f32_out=False))
    print("gather_add_affine_act %4d x %d x %d: fp32 + packed %.1f us, packed only %.1f us (201 MB -> 134 MB)" % (C, H, H, a, b))
