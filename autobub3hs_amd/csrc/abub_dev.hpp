// abub_dev.hpp -- what every translation unit of the gfx950 library shares: the error plumbing and the small packed-math
// device helpers.  Everything here is static / inline and there is no kernel in it: a unit that includes it gets no code it
// does not call.  The bound-and-verify machinery of K2 / K3 lives in abub_scan.hpp, what the frame readers share in
// abub_frames.hpp, what the encoders share in abub_enc.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/abub_hip.h"

// ------------------------------------------------------------------------------------------------
// error plumbing (the thread-local message buffer lives in abub_misc.hip)
// ------------------------------------------------------------------------------------------------
int abub_set_err_(int code, const char *what, hipError_t e);
static int set_err(int code, const char *what, hipError_t e = hipSuccess) { return abub_set_err_(code, what, e); }
#define HIPCHK(x)                                   \
    do {                                            \
        hipError_t e_ = (x);                        \
        if (e_ != hipSuccess)                       \
            return set_err(ABUB_E_HIP, #x, e_);     \
    } while (0)

// ------------------------------------------------------------------------------------------------
// small device helpers
// ------------------------------------------------------------------------------------------------
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

// cv::borderInterpolate(BORDER_REFLECT_101)
__device__ __forceinline__ int reflect101(int p, int len)
{
    if (len == 1)
        return 0;
    while (p < 0 || p >= len)
        p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

// two u16 lanes, saturating unsigned subtract  (v_pk_sub_u16 ... clamp)
__device__ __forceinline__ uint32_t pk_subsat(uint32_t a, uint32_t b)
{
    u16x2 x = __builtin_bit_cast(u16x2, a), y = __builtin_bit_cast(u16x2, b);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(x, y));
}
// two i16 lanes, |a-b|  (2x v_pk_sub_i16 + v_pk_max_i16)
__device__ __forceinline__ uint32_t pk_absdiff(uint32_t a, uint32_t b)
{
    s16x2 x = __builtin_bit_cast(s16x2, a), y = __builtin_bit_cast(s16x2, b);
    s16x2 d = x - y, e = y - x;
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(d, e));
}
// two u16 lanes: a*K + b  (v_pk_mad_u16 with an inline constant)
template <int K>
__device__ __forceinline__ uint32_t pk_madk(uint32_t a, uint32_t b)
{
    u16x2 x = __builtin_bit_cast(u16x2, a), y = __builtin_bit_cast(u16x2, b);
    u16x2 k = {K, K};
    return __builtin_bit_cast(uint32_t, (u16x2)(x * k + y));
}
// two u16 lanes: min(a, 1)  (v_pk_min_u16)
__device__ __forceinline__ uint32_t pk_min1(uint32_t a)
{
    const u16x2 one = {1, 1};
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), one));
}

// (a << 2) + b in one VALU op.  Written as asm because the compiler would CSE the shift of two such
// expressions sharing `a` into shift + 2 adds (3 ops instead of 2).  No u16 lane overflows into its
// neighbour here (all lanes <= 65408 after the add), so the 32-bit form is exact for both lanes.
__device__ __forceinline__ uint32_t lshl2_add(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// bytes (b0,b1) / (b2,b3) of a dword widened to two u16 lanes  (v_perm_b32)
__device__ __forceinline__ uint32_t widen_lo(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0c010c00u); }
__device__ __forceinline__ uint32_t widen_hi(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0c030c02u); }

// ---- packed-byte thresholds for the v_sad_u8 bound scans (K2: k2_sad_chain, K3: k3_bound_scan) ------------------------
__device__ __forceinline__ uint32_t pk_addsat(uint32_t a, uint32_t b)
{
    u16x2 x = __builtin_bit_cast(u16x2, a), y = __builtin_bit_cast(u16x2, b);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_add_sat(x, y));
}
// bytes (b0,b1) / (b2,b3) of a dword into the HIGH bytes of two u16 lanes: a saturating u16 add / sub of two such
// values leaves min(x + y, 255) / max(x - y, 0) in the high byte
__device__ __forceinline__ uint32_t widen8_lo(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x010c000cu); }
__device__ __forceinline__ uint32_t widen8_hi(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x030c020cu); }
// the high bytes of the lanes of (a: pixels 0,1; b: pixels 2,3) packed back into one dword
__device__ __forceinline__ uint32_t pack8(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07050301u); }

#define DPP_WAVE_SHL1 0x130 /* lane i <- lane i+1 */
#define DPP_WAVE_SHR1 0x138 /* lane i <- lane i-1 */

// wave-level ordering of LDS traffic (a list belongs to one wave; LDS executes a wave's instructions in order)
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
