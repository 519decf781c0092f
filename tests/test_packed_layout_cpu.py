"""CPU: the packed activation layout.  csrc/gdm_packed_act.h is the one definition eight kernels write through and the convolution
kernel reads by; here it is compiled for the host as a stand-alone program (tests/packed_layout_host.cpp, plain and under
AddressSanitizer + UBSan) and held to the documented formula, restated independently in numpy (tests/packed_layout.py)."""
import os
import subprocess

import numpy as np
import pytest

import packed_layout as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "packed_layout_host.cpp")


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("packed_layout_host")
    cxx = os.environ.get("CXX", "g++")
    plain, san = str(d / "layout_plain"), str(d / "layout_san")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-o", plain, SRC])
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", san, SRC])
    return plain, san


def _run(prog, *args):
    p = subprocess.run([prog] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.returncode, p.stderr[-2000:])
    return p.stdout.splitlines()


@pytest.fixture(scope="module")
def tables(host_programs):
    """shape -> (header values, int64[B, C/8, H, W, 2] offsets) as the plain program prints them; the sanitised build printed the same."""
    plain, san = host_programs
    out = {}
    for shape in P.SHAPES:
        lines = _run(plain, *shape)
        assert _run(san, *shape) == lines
        B, C, H, W = shape
        head = lines[0].split()
        assert head[0] == "map"
        rows = np.array([[int(v) for v in ln.split()] for ln in lines[1:]], np.int64)
        assert rows.shape == (B * (C // 8) * H * W, 6)
        want_idx = np.stack(np.meshgrid(np.arange(B), np.arange(C // 8), np.arange(H), np.arange(W), indexing="ij"), -1).reshape(-1, 4)
        assert np.array_equal(rows[:, :4], want_idx)                         # every (b, group, y, x), once, in order
        out[shape] = ([int(v) for v in head[1:]], rows[:, 4:].reshape(B, C // 8, H, W, 2))
    return out


@pytest.mark.parametrize("shape", P.SHAPES)
def test_offsets_equal_the_documented_formula(tables, shape):
    B, C, H, W = shape
    (nbytes, nchunk, plane, lo), off = tables[shape]
    assert np.array_equal(off, P.granule_offsets(B, C, H, W))
    assert (nchunk, plane, lo) == (P.nchunk(C), (H + 2) * (W + 2), 16 * (H + 2) * (W + 2) * 16)
    assert np.array_equal(off[..., 1] - off[..., 0], np.full(off.shape[:-1], lo))


@pytest.mark.parametrize("shape", P.SHAPES)
def test_bytes_equal_the_size_function(tables, shape):
    """gdm_conv3x3_act_bytes' formula, restated: B * (H + 2) * (W + 2) * ceil(C / 128) * 512."""
    B, C, H, W = shape
    assert tables[shape][0][0] == B * (H + 2) * (W + 2) * ((C + 127) // 128) * 512 == P.packed_bytes(B, C, H, W)


@pytest.mark.parametrize("shape", P.SHAPES)
def test_granules_are_distinct_aligned_and_inside_the_buffer(tables, shape):
    (nbytes, _, _, _), off = tables[shape]
    flat = off.ravel()
    assert len(np.unique(flat)) == flat.size
    assert (flat % 16 == 0).all() and flat.min() >= 0 and flat.max() + 16 <= nbytes


@pytest.mark.parametrize("shape", P.SHAPES)
def test_untouched_granules_are_exactly_the_border_and_the_missing_channels(tables, shape):
    """No interior pixel lands on a border granule: what the writers leave alone is the one-pixel border of every plane, and all of
    the planes of the channels beyond C in a trailing partial chunk -- nothing else, and nothing less."""
    B, C, H, W = shape
    (nbytes, nchunk, plane, _), off = tables[shape]
    touched = np.zeros(nbytes // 16, bool)
    touched[off.ravel() // 16] = True
    grid = touched.reshape(B, nchunk, 32, H + 2, W + 2)                      # the layout's own nesting: image, chunk, plane, row, column
    want = np.zeros_like(grid)
    for chunk in range(nchunk):
        groups = min(16, C // 8 - 16 * chunk)                               # live 8-channel groups of this chunk
        want[:, chunk, :groups, 1:-1, 1:-1] = True                           # hi planes
        want[:, chunk, 16:16 + groups, 1:-1, 1:-1] = True                    # lo planes
    assert np.array_equal(grid, want)


def test_launcher_predicate(host_programs):
    """gdm_packed_out_ok: C a whole number of 8-channel groups, 64 or a multiple of 128, and a 16-byte aligned buffer."""
    for prog in host_programs:
        rows = np.array([[int(v) for v in ln.split()] for ln in _run(prog, "ok", 700)])
        C = rows[:, 0]
        ok = (C % 8 == 0) & ((C == 64) | ((C >= 128) & (C % 128 == 0)))
        assert np.array_equal(rows[:, 1], ok.astype(int)) and not rows[:, 2].any()


def test_numpy_pack_writes_what_the_offsets_say():
    """The restatement's pack (the reference of the GPU pack-kernel test) against its own offsets: channel c of a pixel is bf16
    element c % 8 of the granule, hi + lo reproduce the value to 2^-16 relative, and everything else stays zero."""
    rs = np.random.RandomState(7)
    B, C, H, W = 2, 136, 3, 2
    x = rs.randn(B, C, H, W).astype(np.float32)
    buf = P.pack(x).view(np.uint16)
    off = P.granule_offsets(B, C, H, W) // 2
    hi = (buf[off[..., 0, None] + np.arange(8)].astype(np.uint32) << 16).view(np.float32)    # [B, C/8, H, W, 8]
    lo = (buf[off[..., 1, None] + np.arange(8)].astype(np.uint32) << 16).view(np.float32)
    xs = x.reshape(B, C // 8, 8, H, W).transpose(0, 1, 3, 4, 2)
    assert np.array_equal(hi, (P.bf16_rne(xs).astype(np.uint32) << 16).view(np.float32))
    assert (np.abs(hi + lo - xs) <= 2.0 ** -16 * np.abs(xs)).all()
    rest = np.ones(buf.size, bool)
    rest[(off[..., None] + np.arange(8)).ravel()] = False
    assert not buf[rest].any()
    # round to nearest EVEN: 1 + 2^-8 is a tie between bf16 1.0 and 1 + 2^-7 and goes to the even one; 1 + 3 * 2^-8 goes up
    assert list(P.bf16_rne(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], np.float32))) == [0x3F80, 0x3F82]
