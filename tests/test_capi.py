"""CPU: the C-ABI shared library builds for gfx950, loads, and exports every symbol include/gdm.h
declares (no compute calls without a GPU); host-side argument checking fails loudly; the ctypes binding
derived from the header has the types the C++ compiler sees in it."""
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


# ------------------------------------------------------------------------------------------
# the binding is derived from include/gdm.h: the compiler, not a hand-typed table, says what the header's types are
# ------------------------------------------------------------------------------------------
_STRUCT_NAMES = {"gdm_knn_job": "KnnJob", "gdm_pw_seg": "PwSeg", "gdm_pw_job": "PwJob", "gdm_copy_job": "CopyJob"}

_CXX_PRELUDE = """
#include "gdm.h"
#include <cstddef>
#include <tuple>
#include <type_traits>
template <class F> struct sig;
template <class R, class... A> struct sig<R (*)(A...)> {
    using ret = R;
    static constexpr int arity = sizeof...(A);
    template <int i> using arg = std::tuple_element_t<i, std::tuple<A...>>;
};
template <class T> constexpr bool is_void = std::is_void_v<T>;
template <class T> constexpr bool is_ptr = std::is_pointer_v<T>;
template <class T, int size, bool sgn> constexpr bool is_int = std::is_integral_v<T> && sizeof(T) == size && std::is_signed_v<T> == sgn;
template <class T, int size> constexpr bool is_flt = std::is_floating_point_v<T> && sizeof(T) == size;
"""


def _cxx_category(c):
    """The C++ predicate (a template of the prelude, still missing its type argument) that a ctypes class stands for."""
    if c is None:
        return "is_void<%s>"
    if c in (ctypes.c_void_p, ctypes.c_char_p) or _is_ptr(c):
        return "is_ptr<%s>"
    if c in (ctypes.c_float, ctypes.c_double):
        return "is_flt<%%s, %d>" % ctypes.sizeof(c)
    assert isinstance(c(0).value, int), c
    return "is_int<%%s, %d, %s>" % (ctypes.sizeof(c), "true" if c(-1).value < 0 else "false")


def test_compiler_agrees_with_the_parsed_header(tmp_path):
    """Every return type, parameter type and arity of SIGNATURES, and the size and every field offset / type of the four job
    structures, as static_asserts against decltype(&gdm_x) and offsetof in a C++ file that includes gdm.h: pointer, integer of a
    size and signedness, floating type of a size.  A row that says int where the header says long does not compile."""
    import subprocess
    from geometric_aware_dense_matching_amd import _lib
    lines = [_CXX_PRELUDE]
    for name, (res, args) in _lib.SIGNATURES.items():
        s = "sig<decltype(&%s)>" % name
        lines.append('static_assert(%s::arity == %d, "%s: arity");' % (s, len(args), name))
        lines.append('static_assert(%s, "%s: return type");' % (_cxx_category(res) % (s + "::ret"), name))
        for i, a in enumerate(args):
            lines.append('static_assert(%s, "%s: parameter %d (%s)");' % (_cxx_category(a) % ("%s::arg<%d>" % (s, i)), name, i,
                                                                          _lib.PARAMS[name][i]))
    for cname, pyname in _STRUCT_NAMES.items():
        cls = getattr(_lib, pyname)
        lines.append('static_assert(sizeof(%s) == %d, "%s: size");' % (cname, ctypes.sizeof(cls), cname))
        for field, ftype in cls._fields_:
            lines.append('static_assert(offsetof(%s, %s) == %d, "%s.%s: offset");' % (cname, field, getattr(cls, field).offset, cname, field))
            lines.append('static_assert(%s, "%s.%s: type");' % (_cxx_category(ftype) % ("decltype(%s::%s)" % (cname, field)), cname, field))
    assert len(_lib.SIGNATURES) >= 149 and len(lines) > 1500
    src = tmp_path / "gdm_types.cpp"
    src.write_text("\n".join(lines) + "\n")
    out = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def test_header_constants_and_their_aliases():
    from geometric_aware_dense_matching_amd import _lib, frontend, ops
    defines = re.findall(r"^#define\s+(GDM_\w+)\s+\(?(-?[0-9.]+)f?\)?\s*(?:/\*.*)?$", open(os.path.join(ROOT, "include", "gdm.h")).read(),
                         flags=re.M)
    assert len(defines) == 20
    for name, text in defines:
        val = getattr(_lib, name)
        assert type(val) is (float if "." in text else int) and val == float(text), name
    for mod, alias, name in ((ops, "MATCH_BF16X3", "GDM_MATCH_BF16X3"), (ops, "MATCH_F32", "GDM_MATCH_F32"),
                             (ops, "MATCH_SOFT_MAX_GAMMA", "GDM_MATCH_SOFT_MAX_GAMMA"), (ops, "MATCH_SOFT_MAX_M", "GDM_MATCH_SOFT_MAX_M"),
                             (ops, "SOFT_COORD_MAX_GAMMA", "GDM_SOFT_COORD_MAX_GAMMA"), (frontend, "NORMALS_MAX_K", "GDM_NORMALS_MAX_K"),
                             (frontend, "FILL_STAGES", "GDM_FILL_STAGES")):
        assert getattr(mod, alias) is getattr(_lib, name), alias
    assert frontend.FILL_MODES == {"multiscale": _lib.GDM_FILL_MULTISCALE, "fast": _lib.GDM_FILL_FAST}


def test_parser_refuses_an_unknown_type():
    from geometric_aware_dense_matching_amd import _lib
    with pytest.raises(RuntimeError, match="short.*gdm_made_up_hip"):
        _lib._parse("int gdm_made_up_hip(const float* x, short n, void* stream);")
    with pytest.raises(RuntimeError, match="gdm_made_up_hip"):
        _lib._parse("int gdm_made_up_hip(const short* x, int n, void* stream);")
    consts, sigs, names = _lib._parse("#define GDM_MADE_UP 3\nlong gdm_made_up(const float* x, size_t n);")
    assert consts == {"GDM_MADE_UP": 3} and names == {"gdm_made_up": ("x", "n")}
    assert sigs == {"gdm_made_up": (ctypes.c_long, [ctypes.c_void_p, ctypes.c_size_t])}


def test_call_needs_no_gpu_for_host_side_refusals(lib, monkeypatch):
    """_lib.call: tensors go as pointers, the stream is appended where the header's last parameter is the stream, a status raises
    GdmError in check()'s format, a value comes back as it is.  The library refuses these arguments before any HIP call."""
    from geometric_aware_dense_matching_amd import _lib
    monkeypatch.setattr(_lib, "_stream", lambda: None)
    conf, mask, score = torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.uint8), torch.nn.Parameter(torch.zeros(2))
    with pytest.raises(_lib.GdmError, match=r"^gdm_match_score_hip failed \(rc=-1\): .*bad shape"):
        _lib.call("gdm_match_score_hip", conf, mask, 0, 0, score)
    with pytest.raises(_lib.GdmError, match=r"gdm_match_score_hip.*NULL"):
        _lib.call("gdm_match_score_hip", None, None, 0, 0, None)
    n = _lib.call("gdm_match_rows_bytes", 3)
    assert type(n) is int and n == lib.gdm_match_rows_bytes(3) > 0
    with pytest.raises(TypeError):
        _lib.call("gdm_match_score_hip", conf, mask, 0, 0)
    with pytest.raises(TypeError):
        _lib.call("gdm_match_rows_bytes", 3, 4)


_KNN_WS_TABLES = {                                     # entries: (support id, S, K, grid_w); Q = 33, dense strides
    "cloud": [(1, 2048, 16, 0), (2, 512, 16, 0), (3, 128, 16, 0), (4, 32, 16, 0)],
    "k1": [(1, 2048, 1, 0), (2, 512, 1, 0)],
    "one": [(1, 77, 16, 0)],
    "mixed": [(1, 16384, 16, 128), (1, 16384, 16, 0), (1, 16384, 1, 0), (1, 16384, 16, 128), (2, 960, 5, 40), (2, 960, 5, 0),
              (3, 64, 16, 4), (3, 64, 16, 0), (4, 1023, 2, 0), (5, 1024, 2, 0), (6, 8192, 32, 0)],
}
_KNN_WS_BYTES = {"cloud": (48176, 144528, 770816), "k1": (0, 0, 0), "one": (2048, 6144, 32768), "mixed": (458464, 1375392, 7335424)}


def _knn_ws_table(entries):
    """A job table over fake, distinct, 16-byte-aligned addresses per support id (nothing is dereferenced by the size function)."""
    from geometric_aware_dense_matching_amd import _lib
    Q = 33
    arr = (_lib.KnnJob * max(len(entries), 1))()
    for a, (sid, S, K, grid_w) in zip(arr, entries):
        a.support = 0x10000000 * sid
        a.query = 0x7000000000 + 0x10000 * sid
        a.idx = 0x7100000000
        a.d2 = None
        a.support_bstride, a.query_bstride = S * 3, Q * 3
        a.S, a.Q, a.K, a.grid_w = S, Q, K, grid_w
    return arr


@pytest.mark.parametrize("name", sorted(_KNN_WS_TABLES))
def test_knn_workspace_bytes(lib, name):
    """gdm_knn_jobs_workspace_bytes is what the launch's own plan reserves.  Per distinct (support, layout), each rounded up to 16 bytes:
    organised (grid_w >= 8, S / grid_w >= 8, both <= 256): B * (2 W + 2 H + 2 ceil(H / 16)) * 4; unorganised with S >= 1024: B * (16 S +
    4144) (sorted float4 points + KC_META = 1036 words per crop); else hashed tiles B * ntiles * npad * 16 with ntiles = ceil(S / 1024),
    npad = the power of two >= max(64, ceil(S / ntiles)); K = 1 jobs take nothing.  E.g. "cloud", B = 1: 36912 + 8192 + 2048 + 1024;
    "mixed", B = 1: 2112 + 266288 + 528 + 16384 + 1024 (support 3 once: grid_w = 4 is no grid) + 16384 + 20528 + 135216."""
    entries = _KNN_WS_TABLES[name]
    arr = _knn_ws_table(entries)
    for B, want in zip((1, 3, 16), _KNN_WS_BYTES[name]):
        assert lib.gdm_knn_jobs_workspace_bytes(arr, len(entries), B) == want, (name, B)


def test_knn_workspace_bytes_ignores_the_order_of_the_table_and_refuses_bad_tables(lib):
    import random
    rng = random.Random(7)
    entries = list(_KNN_WS_TABLES["mixed"])
    for _ in range(200):
        rng.shuffle(entries)
        assert lib.gdm_knn_jobs_workspace_bytes(_knn_ws_table(entries), len(entries), 3) == _KNN_WS_BYTES["mixed"][1], entries
    arr = _knn_ws_table(_KNN_WS_TABLES["cloud"])
    assert lib.gdm_knn_jobs_workspace_bytes(arr, 33, 1) == 0
    assert lib.gdm_knn_jobs_workspace_bytes(arr, 4, 0) == 0
    assert lib.gdm_knn_jobs_workspace_bytes(None, 4, 1) == 0
