"""ctypes binding of libgdm_hip.so, derived from the C ABI's own declaration: include/gdm.h is parsed at import into SIGNATURES,
the job structures and the GDM_* constants, so an entry point is declared once, in the header.  `call()` is how the package calls one.

The product path has no CPU fallback: if the shared library is missing or a call fails,
this module raises.  `build()` compiles it in-tree with hipcc for gfx950.
"""
import ctypes
import os
import re
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libgdm_hip.so")
CSRC = os.path.join(_PKG, "csrc")

HEADER = os.path.join(_PKG, "..", "include", "gdm.h")

_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double,
            "uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
_STRUCTS = {}          # C name -> ctypes.Structure of every `typedef struct` of the header


def _ctype(ctype, where):
    """The ctypes class of one C type of the header; a data pointer is c_void_p whatever it points to.  An unknown word raises."""
    t = re.sub(r"\bconst\b|\s", "", ctype)
    if t in _SCALARS:
        return _SCALARS[t]
    if t == "void":
        return None
    if t == "char*":
        return ctypes.c_char_p
    if t[-1:] == "*" and t[:-1] in _STRUCTS:
        return ctypes.POINTER(_STRUCTS[t[:-1]])
    if t[-1:] == "*" and (t.rstrip("*") in _SCALARS or t.rstrip("*") in ("void", "uint8_t")):
        return ctypes.c_void_p
    raise RuntimeError("include/gdm.h: unknown type %r in `%s`" % (ctype.strip(), where))


def _parse(text):
    """(constants, signatures, parameter names) of the text of gdm.h.  It defines the job structures into _STRUCTS on the way."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    consts = {}
    for name, val in re.findall(r"^#define\s+(GDM_\w+)\s+\(?(-?[\d.]+)f?\)?\s*$", text, flags=re.M):
        consts[name] = float(val) if "." in val else int(val)
    text = re.sub(r"^\s*#[^\n]*", "", text, flags=re.M)
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            ctype, first, rest = re.fullmatch(r"(.*?)(\w+)((?:\s*,\s*\w+)*)", decl, flags=re.S).groups()
            fields += [(f, _ctype(ctype, "%s: %s" % (name, decl))) for f in [first] + re.findall(r"\w+", rest)]
        cls = "".join(w.capitalize() for w in name.split("_")[1:])          # gdm_knn_job -> KnnJob
        _STRUCTS[name] = type(cls, (ctypes.Structure,), {"_fields_": fields, "__doc__": "%s (include/gdm.h)." % name})
    sigs, names = {}, {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(gdm_\w+)\s*\(([^)]*)\)\s*;", text):
        where = "%s %s(%s)" % (ret.strip(), name, " ".join(params.split()))
        params = [] if params.strip() == "void" else [re.fullmatch(r"(.*?)(\w+)", p.strip(), flags=re.S).groups() for p in params.split(",")]
        sigs[name] = (_ctype(ret, where), [_ctype(t, where) for t, _ in params])
        names[name] = tuple(n for _, n in params)
    return consts, sigs, names


try:
    with open(HEADER) as _header:
        _consts, SIGNATURES, PARAMS = _parse(_header.read())
except OSError as e:
    raise RuntimeError("the package binds libgdm_hip.so from include/gdm.h and cannot read it (%s): %s" % (HEADER, e))
# SIGNATURES: name -> (restype, argtypes) of every symbol the header declares, in its order; PARAMS: name -> parameter names
globals().update(_consts)          # every numeric #define GDM_* of the header
KnnJob, PwSeg, PwJob, CopyJob = (_STRUCTS["gdm_" + n] for n in ("knn_job", "pw_seg", "pw_job", "copy_job"))

_lib = None
_torch = None          # the torch module, once lib() has imported it: torch must not be loaded before lib() decides to


def _objects_state():
    st = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".o"):
            st[f] = os.stat(os.path.join(CSRC, f)).st_mtime_ns
    return st


def build(verbose=False):
    """hipcc --offload-arch=gfx950 build of libgdm_hip.so (cross-compiles without a GPU).  Writes csrc/build_record.json: which
    translation units this call recompiled (`make` decides by time stamps) and the library's size / SHA-256 -- the evidence of what
    was built, read back by `build_record()` (bench.py prints it with its line)."""
    import hashlib
    import json
    import time
    before = _objects_state()
    out = None if verbose else subprocess.DEVNULL
    t0 = time.time()
    subprocess.check_call(["make", "-C", CSRC, "-j4"], stdout=out)
    after = _objects_state()
    rebuilt = sorted(f for f, m in after.items() if before.get(f) != m)
    with open(LIB_PATH, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()[:16]
    rec = {"mode": "hipcc --offload-arch=gfx950 via csrc/Makefile (in-tree, ahead of time)", "recompiled": rebuilt,
           "up_to_date": sorted(set(after) - set(rebuilt)), "lib": os.path.basename(LIB_PATH), "lib_bytes": os.path.getsize(LIB_PATH),
           "lib_sha256_16": digest, "seconds": round(time.time() - t0, 1), "when": time.strftime("%Y-%m-%dT%H:%M:%S")}
    try:
        with open(os.path.join(CSRC, "build_record.json"), "w") as f:
            json.dump(rec, f, indent=1)
    except OSError:
        pass
    print("[gdm build] recompiled %d of %d translation units%s; %s %d bytes sha256 %s" %
          (len(rebuilt), len(after), (": " + " ".join(rebuilt)) if rebuilt else "", rec["lib"], rec["lib_bytes"], digest))
    return LIB_PATH


def build_record():
    """What `build()` last recorded, plus the SHA-256 of the library that is actually loaded (they must agree)."""
    import hashlib
    import json
    rec = {}
    try:
        with open(os.path.join(CSRC, "build_record.json")) as f:
            rec = json.load(f)
    except (OSError, ValueError):
        rec = {"mode": "prebuilt library (no build record travelled)"}
    try:
        with open(LIB_PATH, "rb") as f:
            rec["loaded_lib_sha256_16"] = hashlib.sha256(f.read()).hexdigest()[:16]
    except OSError:
        rec["loaded_lib_sha256_16"] = None
    rec.pop("up_to_date", None)
    if rec.get("lib_sha256_16") is not None:                    # the record describes ANOTHER build (e.g. `make` run by hand afterwards)
        rec["record_matches_loaded_lib"] = rec["lib_sha256_16"] == rec["loaded_lib_sha256_16"]
    return rec


def lib():
    global _lib, _torch
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libgdm_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C geometric_aware_dense_matching_amd/csrc`. There is no CPU fallback." % LIB_PATH)
        # torch FIRST: PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so) and the process must hold exactly one.  Loaded
        # before torch, this library pulls in /opt/rocm's runtime instead, torch then brings its own, and the first launch from here
        # fails with "no ROCm-capable device is detected" (build() followed by smoke() in one process did exactly that).
        import torch
        _torch = torch
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)          # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


class GdmError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        msg = lib().gdm_last_error()
        raise GdmError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else "?"))


def _stream():
    return _torch.cuda.current_stream().cuda_stream


_PLAIN = frozenset((int, float, type(None)))
_entries = {}          # name -> (bound function, whether its last parameter is the stream, how many arguments the caller gives)


def call(name, *args):
    """Call entry point `name` of the library: tensors go as their data_ptr(), everything else (None, addresses, sizes, floats, job
    arrays) as it is.  Every `*_hip` entry takes the HIP stream last and returns a status (the header's convention): torch's current
    stream is appended for it at call time, and a status other than 0 raises GdmError.  The other entries return their value."""
    try:
        fn, hip, n = _entries[name]
    except KeyError:
        hip = PARAMS[name][-1:] == ("stream",)
        fn, hip, n = _entries[name] = getattr(lib(), name), hip, len(PARAMS[name]) - hip
    if len(args) != n:          # ctypes itself lets surplus arguments through, and the stream would follow them
        raise TypeError("%s takes %d arguments%s, got %d" % (name, n, " and the stream" if hip else "", len(args)))
    Tensor = _torch.Tensor          # (isinstance against it is slow for an int or a float: those are told by their type first)
    argv = [a if type(a) in _PLAIN else a.data_ptr() if isinstance(a, Tensor) else a for a in args]
    if not hip:
        return fn(*argv)
    rc = fn(*argv, _stream())
    if rc != 0:
        check(rc, name)
