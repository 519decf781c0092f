"""CPU: gdm_conv1x1_gather_add_hip (the 1x1 GEMM with the point-to-pixel fusion tail as its epilogue) refuses what it is not built for
on the host, before any HIP call: null pointers, an empty gathered term, the leaky activation, packed operands of 2 GiB or more."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from geometric_aware_dense_matching_amd import _lib
    return _lib.lib()


_BUF = (ctypes.c_char * 4096)()


@pytest.fixture(scope="module")
def p():
    """A valid, 16-byte aligned host address: every refusal comes before the first HIP call, nothing is read through it."""
    return (ctypes.addressof(_BUF) + 15) & ~15


def _args(p, **over):
    a = dict(xpk=p, wpk=p, gidx=p, gt=p, gn=4, scale=p, shift=p, B=1, Cin=128, Cout=128, H=8, W=32, act=1, out=p, outpk=p, stream=None)
    a.update(over)
    return [a[k] for k in ("xpk", "wpk", "gidx", "gt", "gn", "scale", "shift", "B", "Cin", "Cout", "H", "W", "act", "out", "outpk", "stream")]


def _refused(lib, p, word, **over):
    rc = lib.gdm_conv1x1_gather_add_hip(*_args(p, **over))
    assert rc != 0, over
    assert word in lib.gdm_last_error(), (over, lib.gdm_last_error())


@pytest.mark.parametrize("name", ["xpk", "wpk", "gidx", "gt", "scale", "shift"])
def test_refuses_a_null_pointer(lib, p, name):
    _refused(lib, p, b"NULL", **{name: None})


def test_refuses_a_call_without_an_output(lib, p):
    _refused(lib, p, b"NULL", out=None, outpk=None)


@pytest.mark.parametrize("gn", [0, -1])
def test_refuses_an_empty_gathered_term(lib, p, gn):
    _refused(lib, p, b"gn=", gn=gn)


@pytest.mark.parametrize("act", [2, -1])
def test_refuses_activations_other_than_none_and_relu(lib, p, act):
    _refused(lib, p, b"act=", act=act)


def test_refuses_shapes_the_kernel_is_not_built_for(lib, p):
    _refused(lib, p, b"Cin=", Cin=64)
    _refused(lib, p, b"Cin=", Cin=100)
    _refused(lib, p, b"W=", W=24)
    _refused(lib, p, b"packed output", Cout=12)                   # Cout % 8 with a packed output
    _refused(lib, p, b"packed output", H=1, out=p)                # B*H*W % 256 with a packed output
    _refused(lib, p, b"aligned", gidx=p + 4)


def test_refuses_packed_operands_of_2_gib_or_more(lib, p):
    """The kernel addresses both packed operands through buffer descriptors with 32-bit byte offsets."""
    # activations: B * (H + 2) * (W + 2) * Cin / 128 * 512 bytes
    assert 4096 * 34 * 34 * 512 >= 2 ** 31
    _refused(lib, p, b"2 GiB", B=4096, H=32, W=32)
    assert 2048 * 34 * 34 * 512 * 2 >= 2 ** 31
    _refused(lib, p, b"2 GiB", B=2048, Cin=256, H=32, W=32)
    # weights: Cin / 128 * roundup(Cout, 128) * 512 bytes
    assert (8192 // 128) * 65536 * 512 >= 2 ** 31
    _refused(lib, p, b"2 GiB", Cin=8192, Cout=65536)
