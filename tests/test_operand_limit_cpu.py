"""CPU: every entry point that launches the convolution / GEMM kernel (csrc/gdm_conv.hip conv_mfma16_kernel) refuses packed operands of
2 GiB or more on the host, before any HIP call -- the kernel addresses both operands with 32-bit byte offsets -- and admits the
neighbouring shape just under the limit; the Python predicate of ops.py draws the same line.

Nothing is launched here, with or without a GPU: the shape just under the limit is called with a packed operand that is not 16-byte
aligned, which the launcher refuses BEHIND the limit check.  "aligned" in the message therefore says that the shape passed the limit,
and the over-limit calls, made with the same misaligned pointer, show that the limit is checked first."""
import ctypes

import pytest

LIMIT = 2 ** 31


@pytest.fixture(scope="module")
def lib():
    from geometric_aware_dense_matching_amd import _lib
    return _lib.lib()


_BUF = (ctypes.c_char * 4096)()


@pytest.fixture(scope="module")
def p():
    """A valid, 16-byte aligned host address: every refusal comes before the first HIP call, nothing is read through it."""
    return (ctypes.addressof(_BUF) + 15) & ~15


def map_bytes(B, Cin, H, W):
    """Packed activations of a [B, Cin, H, W] map: a one-pixel zero border, 512 bytes per pixel and 128-channel chunk."""
    return B * (H + 2) * (W + 2) * -(-Cin // 128) * 512


def weight_bytes(taps, Cin, Cout):
    return taps * -(-Cin // 128) * (-(-Cout // 128) * 128) * 512


def _call(lib, p, name, shape):
    """The entry point `name` on `shape`, with a misaligned xpk (see the module's docstring): (return code, message)."""
    q = p + 4
    s = shape
    if name == "gdm_conv3x3_packed_hip":
        rc = lib.gdm_conv3x3_packed_hip(q, p, None, None, None, s["B"], s["Cin"], s["Cout"], s["H"], s["W"], 0, p, None)
    elif name == "gdm_conv3x3_strided_hip":
        rc = lib.gdm_conv3x3_strided_hip(q, p, None, None, None, s["B"], s["Cin"], s["Cout"], s["H"], s["W"], s["stride"], 0, p, None, None)
    elif name == "gdm_conv1x1_packed_hip":
        rc = lib.gdm_conv1x1_packed_hip(q, p, None, None, s["B"], s["Cin"], s["Cout"], s["H"], s["W"], 0, 0, p, None)
    elif name == "gdm_conv1x1_strided_hip":
        rc = lib.gdm_conv1x1_strided_hip(q, p, None, None, s["B"], s["Cin"], s["Cout"], s["H"], s["W"], s["stride"], 0, p, None)
    elif name == "gdm_gemm_grouped_hip":
        rc = lib.gdm_gemm_grouped_hip(q, p, p, p, s["R"], s["M"], s["Cin"], s["Cout"], p, None)
    elif name == "gdm_conv1x1_packed_wb_hip":
        rc = lib.gdm_conv1x1_packed_wb_hip(q, p, s["wbstride"], s["B"], s["Cin"], s["Cout"], s["H"], s["W"], p, None)
    else:
        raise KeyError(name)
    return rc, lib.gdm_last_error()


def _refused_for_the_limit(lib, p, name, shape):
    rc, msg = _call(lib, p, name, shape)
    assert rc != 0, (name, shape)
    assert b"2 GiB" in msg and name.encode() in msg, (name, shape, msg)


def _passes_the_limit(lib, p, name, shape):
    rc, msg = _call(lib, p, name, shape)
    assert rc != 0, (name, shape)                               # (the misaligned operand)
    assert b"2 GiB" not in msg and b"aligned" in msg, (name, shape, msg)


def _wb(x_shape, Cout, parts, taps):
    """The launch conv3x3_wgrad (taps 9, x [B, Cin, H, W]) / gemm_wgrad (taps 1, x [B, Cin, 1, P]) makes of gdm_conv1x1_packed_wb_hip."""
    B, Cin, H, W = x_shape
    n = B * H * W // 128 // parts
    return dict(wbstride=n * (-(-Cout // 128) * 128) * 512, B=parts, Cin=128 * n, Cout=Cout, H=taps, W=Cin)


# (entry point, what varies, first value AT OR PAST the limit, its neighbour under it, shape as a function of that value, bytes as one)
ACT_SIDE = [
    ("gdm_conv3x3_packed_hip", 3629, 3628, lambda B: dict(B=B, Cin=128, Cout=128, H=32, W=32), lambda B: map_bytes(B, 128, 32, 32)),
    ("gdm_conv3x3_strided_hip", 963, 962, lambda B: dict(B=B, Cin=64, Cout=64, H=64, W=64, stride=1), lambda B: map_bytes(B, 64, 64, 64)),
    # stride 2: H, W are the OUTPUT size, the operand is the 128 x 128 input
    ("gdm_conv3x3_strided_hip", 249, 248, lambda B: dict(B=B, Cin=64, Cout=64, H=64, W=64, stride=2), lambda B: map_bytes(B, 64, 128, 128)),
    # a [B, 64, 43680] product packed as a map of one row per image
    ("gdm_conv1x1_packed_hip", 33, 32, lambda B: dict(B=B, Cin=64, Cout=128, H=1, W=43680), lambda B: map_bytes(B, 64, 1, 43680)),
    ("gdm_conv1x1_packed_hip", 699072, 699040, lambda n: dict(B=2, Cin=128, Cout=128, H=1, W=n), lambda n: map_bytes(2, 128, 1, n)),
    ("gdm_conv1x1_strided_hip", 249, 248, lambda B: dict(B=B, Cin=64, Cout=64, H=64, W=64, stride=2), lambda B: map_bytes(B, 64, 128, 128)),
    ("gdm_conv1x1_strided_hip", 3629, 3628, lambda B: dict(B=B, Cin=128, Cout=128, H=32, W=32, stride=1), lambda B: map_bytes(B, 128, 32, 32)),
    # the grouped form: ONE 1 x M map whatever the number of gathered rows
    ("gdm_gemm_grouped_hip", 1398100, 1398099, lambda M: dict(R=256, M=M, Cin=128, Cout=128), lambda M: map_bytes(1, 128, 1, M)),
    ("gdm_gemm_grouped_hip", 1398100, 1398080, lambda M: dict(R=1 << 20, M=M, Cin=128, Cout=128), lambda M: map_bytes(1, 128, 1, M)),
    # the weight-gradient GEMMs: "images" = parts of the contraction, "map" = taps x Cin; B * H*W * (Cin + 2) * 44 (3x3) or * 12 (1x1) bytes
    ("gdm_conv1x1_packed_wb_hip", 47, 46, lambda B: _wb((B, 256, 64, 64), 8, 1, 9), lambda B: B * 64 * 64 * (256 + 2) * 44),
    ("gdm_conv1x1_packed_wb_hip", 47, 46, lambda B: _wb((B, 256, 64, 64), 8, 32, 9), lambda B: B * 64 * 64 * (256 + 2) * 44),
    ("gdm_conv1x1_packed_wb_hip", 43, 42, lambda B: _wb((B, 256, 1, 16384), 64, 1, 1), lambda B: B * 16384 * (256 + 2) * 12),
]


@pytest.mark.parametrize("name,over,under,shape,nbytes", ACT_SIDE, ids=["%s-%d" % (c[0], i) for i, c in enumerate(ACT_SIDE)])
def test_refuses_activations_of_2_gib_or_more_and_admits_the_shape_below(lib, p, name, over, under, shape, nbytes):
    assert nbytes(under) < LIMIT <= nbytes(over), (nbytes(under), nbytes(over))
    _refused_for_the_limit(lib, p, name, shape(over))
    _passes_the_limit(lib, p, name, shape(under))


def test_the_wb_shapes_are_the_operands_the_size_functions_count(lib):
    """The "map" of a weight-gradient launch has the bytes of gdm_wgrad_x_bytes / gdm_wgrad_x1_bytes, its weights those of gdm_wgrad_go_bytes."""
    for parts in (1, 32):
        s = _wb((46, 256, 64, 64), 8, parts, 9)
        assert map_bytes(s["B"], s["Cin"], s["H"], s["W"]) == lib.gdm_wgrad_x_bytes(46, 256, 64, 64) == 2138898432
        assert s["B"] * s["wbstride"] == lib.gdm_wgrad_go_bytes(46, 8, 64, 64)
    s = _wb((42, 256, 1, 16384), 64, 1, 1)
    assert map_bytes(s["B"], s["Cin"], s["H"], s["W"]) == lib.gdm_wgrad_x1_bytes(42, 256, 16384) == 2130444288
    assert s["B"] * s["wbstride"] == lib.gdm_wgrad_go_bytes(42, 64, 16384 // 32, 32)


# weights: taps * Cin / 128 * roundup(Cout, 128) * 512 bytes; with per-image weights, (B - 1) * w_bstride bytes in front of the last set
WEIGHT_SIDE = [
    ("gdm_conv3x3_packed_hip", 7296, 7168, lambda co: dict(B=1, Cin=8192, Cout=co, H=1, W=32), lambda co: weight_bytes(9, 8192, co)),
    ("gdm_conv3x3_strided_hip", 7296, 7168, lambda co: dict(B=1, Cin=8192, Cout=co, H=1, W=32, stride=2), lambda co: weight_bytes(9, 8192, co)),
    ("gdm_conv1x1_packed_hip", 65409, 65408, lambda co: dict(B=1, Cin=8192, Cout=co, H=1, W=32), lambda co: weight_bytes(1, 8192, co)),
    ("gdm_conv1x1_strided_hip", 65409, 65408, lambda co: dict(B=1, Cin=8192, Cout=co, H=1, W=32, stride=1), lambda co: weight_bytes(1, 8192, co)),
    ("gdm_gemm_grouped_hip", 65536, 65408, lambda co: dict(R=256, M=32, Cin=8192, Cout=co), lambda co: weight_bytes(1, 8192, co)),
    # one weight set: as the 1x1 GEMM
    ("gdm_conv1x1_packed_wb_hip", 4096, 3968, lambda co: dict(wbstride=0, B=1, Cin=128 * 1024, Cout=co, H=8, W=32),
     lambda co: weight_bytes(1, 128 * 1024, co)),
    # two images, two weight sets of 1 GiB: the varied value is the first set's size
    ("gdm_conv1x1_packed_wb_hip", 2 ** 30, 2 ** 30 - 16, lambda st: dict(wbstride=st, B=2, Cin=128 * 512, Cout=4096, H=8, W=32),
     lambda st: st + weight_bytes(1, 128 * 512, 4096)),
]


@pytest.mark.parametrize("name,over,under,shape,nbytes", WEIGHT_SIDE, ids=["%s-%d" % (c[0], i) for i, c in enumerate(WEIGHT_SIDE)])
def test_refuses_weights_of_2_gib_or_more_and_admits_the_shape_below(lib, p, name, over, under, shape, nbytes):
    assert nbytes(under) < LIMIT <= nbytes(over), (nbytes(under), nbytes(over))
    _refused_for_the_limit(lib, p, name, shape(over))
    _passes_the_limit(lib, p, name, shape(under))


def test_the_refusal_names_the_entry_point_and_both_byte_counts(lib, p):
    rc, msg = _call(lib, p, "gdm_conv3x3_strided_hip", dict(B=963, Cin=64, Cout=64, H=64, W=64, stride=1))
    assert rc != 0
    assert msg.startswith(b"gdm_conv3x3_strided_hip:"), msg
    assert str(map_bytes(963, 64, 64, 64)).encode() in msg and str(weight_bytes(9, 64, 64)).encode() in msg, msg


def test_a_byte_count_that_overflows_64_bits_is_refused_too(lib, p):
    _refused_for_the_limit(lib, p, "gdm_conv1x1_packed_wb_hip", dict(wbstride=2 ** 62, B=2 ** 31 - 1, Cin=128, Cout=128, H=8, W=32))
    _refused_for_the_limit(lib, p, "gdm_conv1x1_packed_hip", dict(B=2 ** 31 - 1, Cin=2 ** 31 - 128, Cout=128, H=1, W=2 ** 31 - 32))


# The GPU tests' shapes (tests/test_gpu_operand_limit.py), one side each: (what ops.py's predicate is asked, bytes in plain arithmetic)
def _predicate_cases(lib):
    from geometric_aware_dense_matching_amd import ops
    return [
        ("gemm, many images", lambda B: ops.gemm_supported(64, 128, 43680, B), 32, 33, lambda B: B * 3 * (43680 + 2) * 512, 2147057664),
        ("gemm, two long images", lambda n: ops.gemm_supported(128, 128, n, 2), 699040, 699072, lambda n: 2 * 3 * (n + 2) * 512, 2147457024),
        ("conv3x3", lambda B: ops.operands_fit(ops._map_bytes(B, 64, 64, 64)), 962, 963, lambda B: B * 66 * 66 * 512, 2145521664),
        ("stride 2", lambda B: ops.operands_fit(ops._map_bytes(B, 64, 128, 128)), 248, 249, lambda B: B * 130 * 130 * 512, 2145894400),
        ("grouped", lambda M: ops.gemm_supported(128, 128, M, 1), 1398080, 1398112, lambda M: 3 * (M + 2) * 512, 2147453952),
        ("conv3x3_wgrad", lambda B: ops.operands_fit(lib.gdm_wgrad_x_bytes(B, 256, 64, 64), lib.gdm_wgrad_go_bytes(B, 8, 64, 64)), 46, 47,
         lambda B: B * 64 * 64 * (256 + 2) * 44, 2138898432),
        ("gemm_wgrad", lambda B: ops.operands_fit(lib.gdm_wgrad_x1_bytes(B, 256, 16384), lib.gdm_wgrad_go_bytes(B, 64, 512, 32)), 42, 43,
         lambda B: B * 16384 * (256 + 2) * 12, 2130444288),
    ]


def test_the_python_predicate_draws_the_same_line(lib):
    for what, fits, under, over, nbytes, stated in _predicate_cases(lib):
        assert nbytes(under) == stated < LIMIT <= nbytes(over), what
        assert fits(under), what
        assert not fits(over), what


def test_the_wrappers_refuse_before_they_touch_a_tensor(lib):
    """ValueError with the shape and the byte count, raised from the shape alone: a meta tensor has no storage to pack."""
    import torch
    from geometric_aware_dense_matching_amd import ops
    wpk = torch.empty(65536, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"gemm_bf16x3.*33, 64, 43680.*2214153216"):
        ops.gemm_bf16x3(torch.empty(33, 64, 43680, device="meta"), wpk, 128)
    with pytest.raises(ValueError, match=r"conv3x3_bf16x3.*963, 64, 64, 64.*2147751936"):
        ops.conv3x3_bf16x3(torch.empty(963, 64, 64, 64, device="meta"), wpk, 64)
    with pytest.raises(ValueError, match=r"conv3x3_pack_act.*249, 64, 128, 128.*2154547200"):
        ops.conv3x3_pack_act(torch.empty(249, 64, 128, 128, device="meta"))
    with pytest.raises(ValueError, match=r"conv1x1_packed2d.*249, 64, 128, 128.*2154547200"):
        ops.conv1x1_packed2d(ops.PackedAct(None, (249, 64, 128, 128)), wpk, 64, stride=2)
    with pytest.raises(ValueError, match=r"gemm_grouped.*1, 128, 1398100.*2147484672"):
        ops.gemm_grouped(torch.empty(1, 128, 1398100, device="meta"), wpk, torch.zeros(256, dtype=torch.int32), None, 128)
    with pytest.raises(ValueError, match=r"conv3x3_wgrad.*47, 256, 64, 64.*2185396224"):
        ops.conv3x3_wgrad(torch.empty(47, 256, 64, 64, device="meta"), torch.empty(47, 8, 64, 64, device="meta"))
    with pytest.raises(ValueError, match=r"gemm_wgrad.*43, 256, 16384.*2181169152"):
        ops.gemm_wgrad(torch.empty(43, 256, 16384, device="meta"), torch.empty(43, 64, 16384, device="meta"))
