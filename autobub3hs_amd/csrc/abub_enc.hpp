// abub_enc.hpp -- what the two GPU encoders (abub_abf_enc.hip, abub_png_enc.hip) share: the scan of their place kernels, the load
// of a pixel's left neighbour, the kernel that places the files of a batch, and the argument check of their entries.  The source
// check (a frame of P bytes at s lies inside the pixels: frame_in_range, found alike by every kernel of an entry) and the wave
// sum come from abub_frames.hpp.  Included by those two translation units only.
#ifndef ABUB_ENC_HPP
#define ABUB_ENC_HPP

#include "abub_frames.hpp"

namespace {

#define ENC_SCAN 256 /* threads of the place kernels */

inline size_t align16z(size_t v) { return (v + 15) & ~(size_t)15; }

// v of the lane to the left (0 in lane 0)
__device__ __forceinline__ uint32_t enc_left_neighbour(uint32_t v)
{
    uint32_t prev = __builtin_amdgcn_update_dpp(0u, v, DPP_WAVE_SHR1, 0xf, 0xf, false);
    // (the shift stays a v_mov_b32_dpp of its own: folded into the subtraction that follows it -- v_subrev_u32_dpp with v as
    // both operands -- the difference came out negated on gfx950)
    asm volatile("" : "+v"(prev));
    return prev;
}

// inclusive scan over the ENC_SCAN threads of a block (sh: one word per wave); every thread calls it
template <class T>
__device__ __forceinline__ T enc_block_scan(T v, T *sh, T &blockTotal)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o);
        if (lane >= o)
            v += t;
    }
    __syncthreads(); // (sh may still be read by the round before)
    if (lane == 63)
        sh[wv] = v;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < ENC_SCAN / 64; ++w) {
        const T t = sh[w];
        before += w < wv ? t : (T)0;
        all += t;
    }
    blockTotal = all;
    return v + before;
}

// files[f] = {off, len, status} with off[0] = 0, off[f + 1] = align16(off[f] + len[f]); *total = the end of the last file.
// A frame is P bytes; frame f's length is the word at flen + f * stride bytes (0 for a frame that is not read).  One workgroup.
__global__ __launch_bounds__(ENC_SCAN) void k_enc_place_files(uint64_t pixels_bytes, const uint64_t *__restrict__ src, int nframes,
                                                               uint64_t P, const uint32_t *__restrict__ flen, uint32_t stride,
                                                               uint64_t out_cap, abub_abf_file *__restrict__ files,
                                                               uint64_t *__restrict__ total)
{
    __shared__ unsigned long long sh[ENC_SCAN / 64];
    unsigned long long base = 0;
    for (int f0 = 0; f0 < nframes; f0 += ENC_SCAN) {
        const int f = f0 + (int)threadIdx.x;
        const uint32_t len = f < nframes ? *(const uint32_t *)((const uint8_t *)flen + (uint64_t)f * stride) : 0u;
        const unsigned long long room = ((unsigned long long)len + 15ull) & ~15ull;
        unsigned long long all;
        const unsigned long long incl = enc_block_scan(room, sh, all);
        if (f < nframes) {
            const uint64_t off = base + incl - room;
            abub_abf_file r;
            r.off = off;
            r.len = len;
            r.status = !frame_in_range(src[f], pixels_bytes, P) ? ABUB_ABF_ENC_E_SRC : off + len > out_cap ? ABUB_ABF_ENC_E_CAP : 0;
            files[f] = r;
            if (f == nframes - 1)
                *total = off + len;
        }
        base += all;
    }
}

// The refusals of an encoder's entry, the same for both and in this order.  `stem` names the entry (<stem>_dev, as it stands
// in abub_last_error()) and its scratch function (<stem>_scratch_bytes).  ABUB_OK: the arguments can be used
inline int enc_check_args(const char *stem, size_t (*fileBound)(int, int), size_t (*scratchBytes)(int, int, int), const void *pixels,
                          const uint64_t *src, int nframes, int W, int H, const void *out, const abub_abf_file *files,
                          const uint64_t *total, const void *scratch, size_t scratch_bytes)
{
    char msg[160];
    if (!pixels || !src || !out || !files || !total || !scratch || nframes < 0)
        snprintf(msg, sizeof msg, "%s_dev: null pointer or negative count", stem);
    else if (W < 1 || W > 65535 || H < 1 || H > 65535)
        snprintf(msg, sizeof msg, "%s_dev: width and height must be in [1, 65535]", stem);
    else if (!fileBound(W, H))
        snprintf(msg, sizeof msg, "%s_dev: a W x H frame whose file may reach 4 GB", stem);
    else if (scratch_bytes < scratchBytes(nframes, W, H))
        snprintf(msg, sizeof msg, "%s_dev: scratch smaller than %s_scratch_bytes", stem, stem);
    else if (((uintptr_t)scratch | (uintptr_t)src | (uintptr_t)files | (uintptr_t)total) & 7)
        snprintf(msg, sizeof msg, "%s_dev: src, files, total and scratch must be 8-byte aligned", stem);
    else
        return ABUB_OK;
    return set_err(ABUB_E_INVALID, msg);
}

} // namespace
#endif
