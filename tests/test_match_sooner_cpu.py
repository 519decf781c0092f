"""CPU: the host side of the two entries that start matching sooner -- gdm_point_heads3_hip (the heads kernel with the scene's matching
rows as an output) and the weights_in_lds argument of gdm_spline_direct3_hip.  Refusals come before any HIP call, so they need no GPU;
the switches are plain module attributes read at call time."""
import ctypes
import os

import pytest

from geometric_aware_dense_matching_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_prototypes_as_the_header_declares_them():
    assert _lib.PARAMS["gdm_point_heads3_hip"] == _lib.PARAMS["gdm_point_heads2_hip"][:-1] + ("out_rows", "stream")
    assert _lib.PARAMS["gdm_spline_direct3_hip"][-3:] == ("out_packed", "weights_in_lds", "stream")
    res, args = _lib.SIGNATURES["gdm_spline_direct3_hip"]
    assert res is ctypes.c_int and args[-2] is ctypes.c_int and args[-1] is ctypes.c_void_p


def _heads_args(p, feat_layer, out_rows):
    w = (ctypes.c_void_p * 2)(p, p)
    none = (ctypes.c_void_p * 2)(None, None)
    act = (ctypes.c_int * 2)(0, 1)
    arr = lambda a: ctypes.cast(a, ctypes.c_void_p)
    return (p, None, 128, None, None, 0, 1, 16, 2, arr(w), arr(none), arr(none), arr(act), feat_layer, -1, None, None, 0,
            p if feat_layer >= 0 else None, None, out_rows, None), (w, none, act)


def test_heads_rows_are_refused_without_a_feature_layer_or_off_a_16_byte_boundary(lib):
    buf = (ctypes.c_char * 65536)()
    p = (ctypes.addressof(buf) + 15) & ~15
    args, keep = _heads_args(p, -1, p)
    assert lib.gdm_point_heads3_hip(*args) != 0 and b"out_rows" in lib.gdm_last_error()
    args, keep = _heads_args(p, 1, p + 4)
    assert lib.gdm_point_heads3_hip(*args) != 0 and b"16-byte" in lib.gdm_last_error()


def test_switches_default_on_and_follow_the_environment():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("from geometric_aware_dense_matching_amd import settings as s; print(int(s.SPLINE_LDS_WEIGHTS), int(s.HEADS_MATCH_ROWS))")
    for env, want in (({}, "1 1"), ({"GDM_SPLINE_LDS_WEIGHTS": "0"}, "0 1"), ({"GDM_HEADS_MATCH_ROWS": "0"}, "1 0")):
        e = {k: v for k, v in os.environ.items() if k not in ("GDM_SPLINE_LDS_WEIGHTS", "GDM_HEADS_MATCH_ROWS")}
        e.update(env)
        out = subprocess.run([sys.executable, "-c", code], cwd=root, env=e, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.split() == want.split(), (env, out.stdout, out.stderr[-300:])
