"""Test infrastructure only: the packed activation layout (csrc/gdm_packed_act.h) restated in numpy from its documented formula,
independently of the header's code.  Shared by tests/test_packed_layout_cpu.py (the header as a host program) and the pack-kernel
test in tests/test_gpu_ops.py.

A map [B, C, H, W]: for every (image b, 128-channel chunk) 32 planes of the zero-bordered (H + 2) x (W + 2) grid; plane q < 16 holds
the bf16 hi parts of channels [8q, 8q + 8) of the chunk, plane 16 + q their lo parts; one pixel of one plane is 16 bytes at
    (((b * nchunk + chunk) * 32 + plane) * (H + 2) * (W + 2) + (y + 1) * (W + 2) + (x + 1)) * 16."""
import numpy as np

# (B, C, H, W) of the CPU test: one granule; 64 channels (half a chunk); one chunk; a partial second chunk; two chunks; the mesh
# branch's [1, C, 1, M] map
SHAPES = [(1, 8, 1, 1), (2, 64, 2, 3), (2, 128, 1, 5), (3, 136, 3, 2), (2, 256, 2, 2), (1, 128, 1, 7)]


def nchunk(C):
    return (C + 127) // 128


def packed_bytes(B, C, H, W):
    """What gdm_conv3x3_act_bytes computes (its shape gate aside): B images x padded grid x chunks x 512 bytes."""
    return B * (H + 2) * (W + 2) * nchunk(C) * 512


def granule_offsets(B, C, H, W):
    """int64[B, C // 8, H, W, 2]: byte offset of the hi ([..., 0]) and lo ([..., 1]) granule of channel group g = c // 8 of every pixel."""
    b, g, y, x = np.meshgrid(np.arange(B), np.arange(C // 8), np.arange(H), np.arange(W), indexing="ij")
    chunk, q = g // 16, g % 16
    out = np.empty(b.shape + (2,), np.int64)
    for k, plane in enumerate((q, 16 + q)):
        out[..., k] = ((((b * nchunk(C) + chunk) * 32 + plane) * (H + 2) * (W + 2)) + (y + 1) * (W + 2) + (x + 1)) * 16
    return out


def bf16_rne(v):
    """fp32 -> bf16 bits (uint16), round to nearest even: what v_cvt_pk_bf16_f32 gives for finite values."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def split(v):
    """gdm_split2's definition (csrc/gdm_common.h): hi = bf16(v), lo = bf16(v - hi), both round to nearest even."""
    v = np.ascontiguousarray(v, np.float32)
    hi = bf16_rne(v)
    hif = (hi.astype(np.uint32) << 16).view(np.float32)
    return hi, bf16_rne(v - hif)


def pack(x):
    """x f32[B, C, H, W] (C % 8 == 0) -> the packed buffer, uint8[packed_bytes]."""
    B, C, H, W = x.shape
    buf = np.zeros(packed_bytes(B, C, H, W) // 2, np.uint16)
    off = granule_offsets(B, C, H, W) // 2                                # in bf16 elements
    parts = split(x)
    for k in range(2):
        p = parts[k].reshape(B, C // 8, 8, H, W)
        for j in range(8):                                               # channel 8g + j is element j of the granule
            buf[off[..., k] + j] = p[:, :, j]
    return buf.view(np.uint8)
