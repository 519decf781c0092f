"""CPU: the C-ABI shared library builds for gfx950, loads, and exports every symbol include/gdm.h
declares (no compute calls without a GPU); host-side argument checking fails loudly."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from geometric_aware_dense_matching_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _header():
    txt = open(os.path.join(ROOT, "include", "gdm.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(gdm_[a-z0-9_]+)\s*\(", _header())))


def _int_entries_with_pointers():
    """Names of the int-returning declarations of gdm.h that take at least one pointer."""
    decls = re.findall(r"^\s*int\s+(gdm_[a-z0-9_]+)\s*\(([^)]*)\)", _header(), flags=re.M)
    return sorted(name for name, params in decls if "*" in params)


def test_every_declared_symbol_is_exported_and_bound(lib):
    from geometric_aware_dense_matching_amd import _lib
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(_lib.SIGNATURES) == names          # the ctypes table covers the header exactly


def test_version_and_error_string(lib):
    assert lib.gdm_version() == 1
    assert isinstance(lib.gdm_last_error(), bytes)


def test_argument_validation_needs_no_gpu(lib):
    rc = lib.gdm_knn_batch_hip(None, None, 1, 4, 4, 1, None, None, None)
    assert rc == -1 and b"NULL" in lib.gdm_last_error()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    assert lib.gdm_knn_batch_hip(p, p, 1, 4, 4, 99, p, None, None) == -1
    assert b"K=99" in lib.gdm_last_error()
    assert lib.gdm_match_hip(p, p, 1, 64, 4, 4, 0, p, p, None, p, 1 << 20, None) == -1
    assert b"D=64" in lib.gdm_last_error()
    assert lib.gdm_match_workspace_bytes(16, 2048, 8192) > 16 * 2048 * 512


def test_code_object_is_gfx950():
    from geometric_aware_dense_matching_amd import _lib
    data = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in data


def test_ops_refuse_cpu_tensors():
    from geometric_aware_dense_matching_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_max(torch.zeros(1, 2, 3), torch.zeros(1, 1, 1, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.match(torch.zeros(1, 128, 32), torch.zeros(128, 64))


def _is_ptr(a):
    return a is ctypes.c_void_p or hasattr(a, "contents") or (hasattr(a, "_type_") and not isinstance(a._type_, str))


@pytest.mark.parametrize("mode", ["null", "zero", "negative"])
def test_every_entry_point_refuses_degenerate_arguments(lib, mode):
    """Every int-returning entry point with pointer arguments, called with (a) all pointers NULL, (b) valid host pointers and every
    size 0, (c) every size -1: a nonzero return code and a message, no launch, no crash -- host-side validation comes before any HIP
    call (which is also why this runs without a GPU)."""
    from geometric_aware_dense_matching_amd import _lib
    buf = (ctypes.c_char * 65536)()
    p = ctypes.addressof(buf)
    called = []
    for name, (res, args) in sorted(_lib.SIGNATURES.items()):
        if res is not ctypes.c_int or not any(_is_ptr(a) for a in args):
            continue
        vals = []
        for a in args:
            if _is_ptr(a):
                vals.append(None if mode == "null" else (p if a is ctypes.c_void_p else ctypes.cast(p, a)))
            elif a in (ctypes.c_float, ctypes.c_double):
                vals.append(0.0)
            else:
                vals.append(-1 if mode == "negative" else 0)
        rc = getattr(lib, name)(*vals)
        assert rc != 0, "%s accepted %s arguments" % (name, mode)
        assert len(lib.gdm_last_error()) > 0
        called.append(name)
    assert called == _int_entries_with_pointers()          # the ctypes filter above skips no entry point of the header


def test_library_loads_behind_torch_hip_runtime():
    """A process must hold ONE HIP runtime: torch's.  _lib.lib() imports torch before it loads libgdm_hip.so, so that a process which
    reaches the library first (__graft_entry__.build() followed by smoke()) does not pull in /opt/rocm's runtime beside torch's --
    which ended in "no ROCm-capable device is detected" at the first launch."""
    import subprocess
    import sys
    code = ("import sys; from geometric_aware_dense_matching_amd import _lib; before = 'torch' in sys.modules; _lib.lib(); "
            "print(before, 'torch' in sys.modules)")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    assert out.stdout.split()[-2:] == ["False", "True"]
