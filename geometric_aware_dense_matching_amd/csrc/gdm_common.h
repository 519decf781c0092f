// Shared helpers for libgdm_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/gdm.h"

void gdm_set_error(const char* fmt, ...);

#define GDM_CHECK_ARG(cond, ...)                   \
    do {                                           \
        if (!(cond)) {                             \
            gdm_set_error(__VA_ARGS__);            \
            return GDM_EINVAL;                     \
        }                                          \
    } while (0)

#define GDM_HIP(call)                                                              \
    do {                                                                           \
        hipError_t _e = (call);                                                    \
        if (_e != hipSuccess) {                                                    \
            gdm_set_error("%s failed: %s", #call, hipGetErrorString(_e));          \
            return (int)_e;                                                        \
        }                                                                          \
    } while (0)

static inline int gdm_launch_status(const char* what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        gdm_set_error("launch of %s failed: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

static inline int gdm_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

#ifdef __cplusplus
#include <type_traits>
// A run-time value as a compile-time constant: f(std::integral_constant<int, v>) for v in [0, N) -- the last arm takes every other value,
// like the `else` of the ladder this replaces -- and f(std::true_type / std::false_type).  Inside f, `decltype(A)::value` is a constant
// expression (a template argument).  Every arm instantiates f, so f must name only instances that are meant to exist.
template <int N, int I = 0, class F>
static inline void gdm_dispatch_int(int v, F&& f)
{
    if constexpr (I + 1 < N) {
        if (v != I) return gdm_dispatch_int<N, I + 1>(v, f);
    }
    f(std::integral_constant<int, I>{});
}
template <class F>
static inline void gdm_dispatch_bool(bool v, F&& f)
{
    if (v) f(std::true_type{});
    else f(std::false_type{});
}

// Allows `Kernel` up to `bytes` of dynamic LDS (more than the 64 KiB a kernel may ask for by default).  Once per instantiation and
// process: the function-local static is initialised once, thread-safely; the result is ignored (a launch that asks for more than it
// may reports the error itself).
template <auto Kernel>
static inline void gdm_allow_lds(int bytes)
{
    static const hipError_t once = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    (void)once;
}
#endif

#ifdef __HIPCC__
// Split-bf16 operands (the matching, convolution, up-convolution and circle-loss kernels): |v - hi - lo| <= 2^-16 |v| (a bf16 half-ulp
// is 2^-8 relative: |lo| <= 2^-8 |v|, and lo's own rounding is 2^-8 of that), both parts
// rounded to nearest even by the hardware conversion (v_cvt_pk_bf16_f32): a NaN stays a NaN in hi (so it reaches the output, as it
// would through an fp32 product) and an overflow rounds to infinity.  hi / lo come back packed two to a dword (element 0 low).
typedef __attribute__((ext_vector_type(2))) float gdm_f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 gdm_bf16x2;
// MFMA operand / accumulator vectors
typedef __attribute__((ext_vector_type(16))) float gdm_f32x16;
typedef __attribute__((ext_vector_type(4))) float gdm_f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 gdm_bf16x8;
typedef __attribute__((ext_vector_type(4))) unsigned gdm_u32x4;
// Byte offset of 16-byte chunk `ch` (0..31: hi | lo halves of 16) of row `row` in an LDS image of ROWB-byte rows, XOR-swizzled inside
// each half by the row so that the 16 rows of an MFMA fragment hit different banks (an involution in ch)
template <int ROWB>
__device__ __forceinline__ int gdm_swz(int row, int ch) { return row * ROWB + (((ch & 16) | ((ch ^ row) & 15)) << 4); }
__device__ __forceinline__ unsigned gdm_bf16_pk(float a, float b)
{
    const gdm_f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, gdm_bf16x2));
}
__device__ __forceinline__ void gdm_split2(float a, float b, unsigned& hi, unsigned& lo)
{
    hi = gdm_bf16_pk(a, b);
    lo = gdm_bf16_pk(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}
// eight values -> one 16-byte operand granule of hi parts and one of lo parts
__device__ __forceinline__ void gdm_split8(const float (&v)[8], gdm_u32x4& hi, gdm_u32x4& lo)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned h, l;                                           // (a vector element does not bind to a reference)
        gdm_split2(v[2 * j], v[2 * j + 1], h, l);
        hi[j] = h, lo[j] = l;
    }
}
__device__ __forceinline__ unsigned short gdm_bf16_1(float a) { return (unsigned short)(gdm_bf16_pk(a, 0.f) & 0xffffu); }
// Packed fp32 arithmetic must not read a register in the two wait states behind the wait that retires its LDS read (ADVICE.md
// item 1, tools/scan_lds_pk_hazard.py): GDM_SETTLE_LDS("+v"(x), ...) retires the reads and spends the two states, once for all the
// registers it names (values read from LDS or shuffled, whose consumers the compiler may pack)
#define GDM_SETTLE_LDS(...) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 1" : __VA_ARGS__)
#endif
