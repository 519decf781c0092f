"""Shared by tests/test_soft_coord_cpu.py and tests/test_gpu_soft_coord.py: inputs, the analytic gradient of the soft assignment, the
per-item Python loop that restates loss.SoftAssignLoss, and the error bounds of DESIGN.md 6l.  Everything here is fp64 torch / numpy on
the CPU; nothing imports the HIP library."""
import math

import numpy as np
import torch

U = 2.0 ** -24
DELTA = 1e-4                 # the project's similarity tolerance


def unit_rows(rs, n, d=128):
    v = rs.randn(n, d)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def make_case(R, M, seed, family="random"):
    """x f32[R,128], y f32[M,128] unit rows (family "copy": every third x_r is a bit-copy of some y_c, so one column holds nearly all
    the mass at a large gamma), xyz f32[M,3] uniform in a +-0.1 m box, upstream a f32[R], b f32[R,3] standard normal."""
    rs = np.random.RandomState(seed)
    x, y = unit_rows(rs, R), unit_rows(rs, M)
    if family == "copy":
        x[::3] = y[rs.randint(0, M, size=len(x[::3]))]
    xyz = rs.uniform(-0.1, 0.1, (M, 3)).astype(np.float32)
    return x, y, xyz, rs.randn(R).astype(np.float32), rs.randn(R, 3).astype(np.float32)


def analytic(x, y, xyz, a, b, gamma):
    """fp64 tensors -> dict(lse, soft, p, G, gx, gy) by the formulas of include/gdm.h (no autograd)."""
    s = x @ y.t()
    lse = torch.logsumexp(gamma * s, dim=1)
    p = torch.exp(gamma * s - lse[:, None])
    soft = p @ xyz
    k = a - (b * soft).sum(1)
    G = gamma * p * (k[:, None] + b @ xyz.t())
    return dict(lse=lse, soft=soft, p=p, G=G, gx=G @ y, gy=G.t() @ x)


def bounds(ref, b, xyz, gamma, R, M):
    """The derived bounds of DESIGN.md 6l on the kernel's outputs against fp64 (torch f64 tensors in, numpy out)."""
    E = math.exp(2 * gamma * DELTA) - 1
    rho = float((xyz - xyz.mean(0)).abs().max())
    b1 = b.abs().sum(1)
    A_r = ref["G"].abs().sum(1)
    A_c = ref["G"].abs().sum(0)
    gx = (E + 2.0 ** -14 + (M + 128) * U) * A_r + 2 * gamma * E * rho * b1 + 1e-7
    gy = (E + 2.0 ** -14 + (R + 128) * U) * A_c + 2 * gamma * E * rho * (ref["p"] * b1[:, None]).sum(0) + 1e-7
    return dict(lse=gamma * DELTA + 1e-5, soft=E * rho + 1e-6, gx=gx.numpy(), gy=gy.numpy(), E=E, rho=rho)


def loop_loss(f, m, xyz, labels, match, gamma, beta, RT=None, cld=None, sym_idx=None, want=("xyz", "nll")):
    """The soft-assignment losses restated as the reference writes its matching loss: a Python loop over the items.  f [B,D,N] raw
    scene features, m [D,M] raw vertex features (both may require grad), xyz [M,3], labels int[B,N], match int[B,N] (M = none);
    target of the coordinate term: R^T (p - t) from RT [B,3,4] and cld [B,3,N] when given, else xyz[match]; sym_idx int[M]: the
    symmetric form (columns match[n] and match[sym_idx[n]]).  Items with fewer than 3 selected points are skipped; the mean over the
    remaining items of the mean over their selected rows; a row without a vertex weighs 0 but counts.  -> (xyz loss, nll loss)."""
    B, D, N = f.shape
    M = m.shape[1]
    y = m / m.norm(dim=0, keepdim=True)
    tot_xyz, tot_nll, n_items = 0.0, 0.0, 0
    for bb in range(B):
        idx = torch.nonzero(labels[bb] == 1).squeeze(1)
        if idx.numel() < 3:
            continue
        n_items += 1
        sx, sn = 0.0, 0.0
        for n in idx.tolist():
            g = int(match[bb, n])
            g2 = int(match[bb, int(sym_idx[n])]) if sym_idx is not None else None
            if g >= M or (g2 is not None and g2 >= M):
                continue
            x = f[bb, :, n] / f[bb, :, n].norm()
            s = gamma * (x @ y)                                   # [M]
            lse = torch.logsumexp(s, dim=0)
            if "nll" in want:
                sn = sn + (lse - s[g] if g2 is None else lse - torch.logaddexp(s[g], s[g2]))
            if "xyz" in want:
                soft = torch.exp(s - lse) @ xyz
                t = xyz[g] if RT is None else RT[bb, :, :3].t() @ (cld[bb, :, n] - RT[bb, :, 3])
                d = (soft - t).abs()
                sx = sx + torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta).sum()
        tot_xyz = tot_xyz + sx / idx.numel()
        tot_nll = tot_nll + sn / idx.numel()
    n_items = max(n_items, 1)
    return tot_xyz / n_items, tot_nll / n_items
