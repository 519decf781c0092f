// The packed activation: the one operand format conv_mfma16_kernel (gdm_conv.hip) reads, and everything that writes it.
//
// A map f32[B, C, H, W] (C = 64 or a multiple of 128) is stored PLANAR by 16-byte MFMA fragment: for every (image b, 128-channel chunk)
// 32 planes of the zero-bordered (H + 2) x (W + 2) pixel grid; plane q < 16 holds the bf16 "hi" parts of channels [8q, 8q + 8) of the
// chunk, plane 16 + q their "lo" parts (gdm_split2, gdm_common.h).  One pixel of one plane is a 16-byte granule at byte
//
//     (((b * nchunk + chunk) * 32 + plane) * (H + 2)(W + 2) + (y + 1) * (W + 2) + (x + 1)) * 16,      nchunk = ceil(C / 128)
//
// A wave's operand load (lane = pixel, one fragment) is then two contiguous 512-byte runs for ANY tap shift, instead of 32 scattered
// 32-byte pieces of pixel-major rows; a tap is just a pixel offset and the zero padding is real zeros.  Writers never touch the border
// or, in a trailing partial chunk (C = 64), the planes of the channels that do not exist: the buffer comes zero-filled.
//
// The layout part of this header is plain C++ (tests/packed_layout_host.cpp includes it without HIP); the stores need hipcc.
//
// How the members are written is part of what the kernels compile to (measured on the ISA of all eight writers):
//   * the plane size is a MEMBER, computed once.  Computed inside each member function, every copy is folded into its own
//     expression before the copies can be merged, and the kernels lose the one register pair the hand-written code kept;
//   * granule() is pixel() + group() as ONE expression, the form the single-granule writers had;
//   * gdm_split8 is four gdm_split2 (the cast-based form of gdm_owner_stream.h costs every writer here instructions, and
//     gdm_split2 costs the kernels there registers: that header keeps its own).
#pragma once
#include <stddef.h>
#include <stdint.h>
#ifdef __HIPCC__
#include "gdm_common.h"
#define GDM_HD __host__ __device__ __forceinline__
#else
#define GDM_HD
#endif

constexpr int GDM_PK_GRANULE = 16;      // bytes of a granule: 8 bf16 of one pixel
constexpr int GDM_PK_PLANES = 32;       // planes per (image, chunk): 16 hi, 16 lo
constexpr int GDM_PK_LO = 16;           // planes from a hi plane to its lo plane
constexpr int GDM_PK_CHUNK = 128;       // channels per chunk

struct gdm_packed_map {
    int C, H, W;
    long np;                            // granules per plane
    GDM_HD gdm_packed_map(int C_, int H_, int W_) : C(C_), H(H_), W(W_), np((long)(H_ + 2) * (W_ + 2)) {}
    GDM_HD int nchunk() const { return (C + GDM_PK_CHUNK - 1) / GDM_PK_CHUNK; }
    GDM_HD long plane() const { return np; }
    GDM_HD size_t bytes(int B) const { return (size_t)B * (H + 2) * (W + 2) * nchunk() * (GDM_PK_PLANES * GDM_PK_GRANULE); }
    // byte offset of plane 0's granule of pixel (y, x): what a writer of several channel groups hoists out of its loop ...
    GDM_HD long pixel(int b, int chunk, int y, int x) const { return (((long)(b * nchunk() + chunk) * GDM_PK_PLANES) * np + (long)(y + 1) * (W + 2) + x + 1) * GDM_PK_GRANULE; }
    // ... what it adds for plane q, and from a hi granule to its lo granule
    GDM_HD long group(int q) const { return (long)q * np * GDM_PK_GRANULE; }
    GDM_HD long lo() const { return GDM_PK_LO * np * GDM_PK_GRANULE; }
    // pixel(b, chunk, y, x) + group(q), for a writer of one granule
    GDM_HD long granule(int b, int chunk, int q, int y, int x) const { return ((((long)b * nchunk() + chunk) * GDM_PK_PLANES + q) * np + (long)(y + 1) * (W + 2) + x + 1) * GDM_PK_GRANULE; }
};

// channel counts the format exists for (a 64-channel map is one half-empty chunk)
static inline bool gdm_packed_channels_ok(int C) { return C == 64 || (C >= GDM_PK_CHUNK && C % GDM_PK_CHUNK == 0); }
// what a producer's launcher checks about its packed output: whole 8-channel groups, a channel count of the format, 16-byte stores
static inline bool gdm_packed_out_ok(int C, const void* buf) { return C % 8 == 0 && gdm_packed_channels_ok(C) && ((uintptr_t)buf & (GDM_PK_GRANULE - 1)) == 0; }

#ifdef __HIPCC__
// eight channels of one pixel -> its hi granule at base + hi_offset and its lo granule at base + lo_offset
__device__ __forceinline__ void gdm_packed_store8(unsigned char* base, long hi_offset, long lo_offset, const float (&v)[8])
{
    gdm_u32x4 hi, lo;
    gdm_split8(v, hi, lo);
    *reinterpret_cast<uint4*>(base + hi_offset) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    *reinterpret_cast<uint4*>(base + lo_offset) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}
// four channels: half (0 / 1) of both granules
__device__ __forceinline__ void gdm_packed_store4(unsigned char* base, long hi_offset, long lo_offset, int half, const float (&v)[4])
{
    unsigned hi0, lo0, hi1, lo1;
    gdm_split2(v[0], v[1], hi0, lo0);
    gdm_split2(v[2], v[3], hi1, lo1);
    unsigned char* p = base + hi_offset + half * (GDM_PK_GRANULE / 2);
    *reinterpret_cast<uint2*>(p) = make_uint2(hi0, hi1);
    *reinterpret_cast<uint2*>(p + (lo_offset - hi_offset)) = make_uint2(lo0, lo1);
}
#endif
