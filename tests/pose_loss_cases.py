"""Shared by tests/test_pose_loss_cpu.py and tests/test_gpu_pose_loss.py: seeded families of weighted correspondences for the pose-fit
loss (include/gdm.h THE POSE LOSS RULE), the host build of the shared fit / adjoint math (tests/pose_adjoint_host.cpp) and the fp64
autograd reference.  Everything here is fp64 numpy / torch on the CPU; nothing needs a GPU."""
import os
import subprocess

import numpy as np
import torch

from geometric_aware_dense_matching_amd import pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "geometric_aware_dense_matching_amd", "csrc")
HOST_SRC = os.path.join(ROOT, "tests", "pose_adjoint_host.cpp")

WELL = ("generic", "noisy", "planar", "weights")          # the families that are meant to be well conditioned
FAMILIES = WELL + ("collinear", "few")


def rot(rs, angle=None):
    """A random rotation (of `angle` radians about a random axis when given)."""
    ax = rs.randn(3)
    ax /= np.linalg.norm(ax)
    a = rs.uniform(0.3, 2.5) if angle is None else angle
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def sym_z(S):
    """S rotations about z by 2 pi j / S as [S,3,4] (j = 0 the identity), with a small translation on the others."""
    out = np.zeros((S, 3, 4))
    for j in range(S):
        a = 2 * np.pi * j / S
        out[j, :, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        out[j, :, 3] = [0.0, 0.0, 0.002 * (j % 2)]
    return out


def make_case(family, seed, n=40, K=32, S=1, winner=0):
    """One crop in fp64: A (model side) [n,3], B (scene) [n,3], w [n], RT_gt [3,4], X [K,3], sym [S,3,4], up (the upstream gradient).
    The ground truth is the true pose moved by a few degrees and millimetres, composed with the inverse of sym[winner], so that
    transform `winner` is the clear minimum of D_s."""
    rs = np.random.RandomState(seed)
    if family == "few":
        n = 4
    A = rs.uniform(-0.1, 0.1, (n, 3))
    if family == "planar":
        A[:, 2] *= 0.02
    if family == "collinear":
        A = np.outer(rs.uniform(-0.1, 0.1, n), rs.randn(3) / 2) + rs.uniform(-0.05, 0.05, 3)
    R, t = rot(rs), rs.uniform(-0.3, 0.3, 3) + np.array([0, 0, 0.8])
    noise = 2e-2 if family == "noisy" else 1e-3
    B = A @ R.T + t + (0.0 if family == "collinear" else noise) * rs.randn(n, 3)
    w = 10.0 ** rs.uniform(-6, 0, n) if family == "weights" else rs.uniform(0.2, 1.0, n)
    sym = sym_z(S)
    Rg = rot(rs, 0.05) @ R
    tg = t + rs.uniform(-0.01, 0.01, 3)
    Rs, ts = sym[winner, :, :3], sym[winner, :, 3]
    gt = np.concatenate([Rg @ Rs.T, (tg - Rg @ Rs.T @ ts)[:, None]], axis=1)          # gt o sym[winner] = (Rg | tg)
    X = rs.uniform(-0.1, 0.1, (K, 3))
    return dict(A=A, B=B, w=w, gt=gt, X=X, sym=sym, up=float(rs.uniform(0.5, 2.0)), family=family, seed=seed, winner=winner)


def build_host(out_dir, sanitize=False):
    """g++ build of tests/pose_adjoint_host.cpp against the package's csrc (the fragment and the adjoint header, unchanged); with
    sanitize, under -fsanitize=address,undefined.  A stand-alone program: nothing of it is loaded into Python."""
    exe = os.path.join(str(out_dir), "pose_adjoint_host" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-ffp-contract=off", "-Wall"] + flags + ["-I", CSRC, HOST_SRC, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=300)
    return exe


def host_input(cases, min_points=5, cond_min=1e-3):
    lines = ["%d" % len(cases)]
    for c in cases:
        n, K, S = len(c["A"]), len(c["X"]), len(c["sym"])
        lines.append("%d %d %d %d %r %r" % (n, K, S, min_points, float(cond_min), c["up"]))
        rows = np.concatenate([c["A"], c["B"], c["w"][:, None]], axis=1)
        for block in (rows, c["gt"], c["X"], c["sym"].reshape(-1, 12)):
            lines += [" ".join(repr(float(v)) for v in row) for row in np.asarray(block, np.float64).reshape(-1, np.asarray(block).shape[-1])]
    return "\n".join(lines) + "\n"


def run_host(exe, cases, min_points=5, cond_min=1e-3):
    """-> (raw stdout, [dict(state, sym_idx, loss, dA [n,3], dw [n])]) of the host program on the cases."""
    out = subprocess.run([exe], input=host_input(cases, min_points, cond_min), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    assert out.stderr == "", out.stderr[-2000:]
    tok = iter(out.stdout.split())
    res = []
    for c in cases:
        state, win, loss = int(next(tok)), int(next(tok)), float.fromhex(next(tok))
        g = np.array([float.fromhex(next(tok)) for _ in range(4 * len(c["A"]))]).reshape(-1, 4)
        res.append(dict(state=state, sym_idx=win, loss=loss, dA=g[:, :3], dw=g[:, 3]))
    return out.stdout, res


def reference(c, min_points=5, cond_min=1e-3, dtype=torch.float64, mask=None):
    """pose.kabsch_pose_loss_reference on one case with fp64 autograd: dict(state, sym_idx, loss, dA, dw, RT) (gradients of up * loss)."""
    A = torch.tensor(c["A"], dtype=dtype)[None].requires_grad_(True)
    w = torch.tensor(c["w"], dtype=dtype)[None].requires_grad_(True)
    loss, RT, state, sym_idx = pose.kabsch_pose_loss_reference(
        torch.tensor(c["B"], dtype=dtype)[None], A, w, torch.tensor(c["gt"], dtype=dtype)[None], torch.tensor(c["X"], dtype=dtype),
        torch.tensor(c["sym"], dtype=dtype), mask, min_points, cond_min)
    dA, dw = np.zeros(c["A"].shape), np.zeros(c["w"].shape)
    if loss.requires_grad:
        ga, gw = torch.autograd.grad((loss * c["up"]).sum(), (A, w), allow_unused=True)
        dA = dA if ga is None else ga[0].numpy()
        dw = dw if gw is None else gw[0].numpy()
    return dict(state=int(state[0]), sym_idx=int(sym_idx[0]), loss=float(loss[0]), dA=dA, dw=dw, RT=RT[0].numpy())
