"""ORACLE -- test infrastructure only; never imported by the product package.

ctypes face of oracle/_build/libkabsch_fit_host.so: the product's pose-fit fragment (csrc/gdm_kabsch_fit.inc) compiled for the host
(oracle/kabsch_fit_host.cpp), and the runner of its sanitizer build (make -C oracle san)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libkabsch_fit_host.so")
_SAN = os.path.join(_HERE, "_build", "kabsch_fit_host_san")
_SRC = [os.path.join(_HERE, "kabsch_fit_host.cpp"),
        os.path.join(_HERE, "..", "geometric_aware_dense_matching_amd", "csrc", "gdm_kabsch_fit.inc")]

_lib = None


def _stale(path):
    return not os.path.exists(path) or any(os.path.getmtime(s) > os.path.getmtime(path) for s in _SRC)


def _load():
    global _lib
    if _lib is None:
        if _stale(_SO):
            subprocess.check_call(["make", "-s", "-C", _HERE, "_build/libkabsch_fit_host.so"])
        lib = ctypes.CDLL(_SO)
        lib.kabsch_fit_host_batch.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
        lib.kabsch_fit_host_batch.restype = None
        _lib = lib
    return _lib


def stats_of(A, B):
    """The 16 statistics of gdm_kabsch_stats_hip in fp64: A (model), B (scene) [..., n, 3] -> f64[..., 16]."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    n = np.full(A.shape[:-2] + (1,), float(A.shape[-2]))
    ab = np.swapaxes(A, -1, -2) @ B
    return np.concatenate([n, A.sum(-2), B.sum(-2), ab.reshape(ab.shape[:-2] + (9,))], axis=-1)


def fit(stats):
    """stats f64[K,16] -> [R | t] f32[K,3,4], by the fragment."""
    stats = np.ascontiguousarray(stats, np.float64).reshape(-1, 16)
    out = np.full((stats.shape[0], 3, 4), np.nan, np.float32)
    _load().kabsch_fit_host_batch(stats.ctypes.data, stats.shape[0], out.ctypes.data)
    return out


def fit_sanitized(stats):
    """The same through the AddressSanitizer + UBSan build, in a process of its own -> (f32[K,3,4], return code, stderr)."""
    if _stale(_SAN):
        subprocess.check_call(["make", "-s", "-C", _HERE, "san"])
    stats = np.ascontiguousarray(stats, np.float64).reshape(-1, 16)
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "stats.bin"), os.path.join(d, "RT.bin")
        stats.tofile(src)
        p = subprocess.run([_SAN, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        out = np.fromfile(dst, np.float32).reshape(-1, 3, 4) if p.returncode == 0 else None
    return out, p.returncode, p.stderr.decode(errors="replace")
