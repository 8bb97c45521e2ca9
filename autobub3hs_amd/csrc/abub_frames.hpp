// abub_frames.hpp -- what the kernels that walk resident frames byte by byte share (abub_compare.hip, abub_stats.hip,
// abub_peek.hip; abub_enc.hpp takes the range test and the wave sum): the range test, the walk of a frame in 16 KiB tiles
// with the widest loads the addresses allow, the wave reduction, and the entries' common checks and grid shape.
//
// The walk.  The grid is jobs x contiguous FR_TILE-byte tiles of the frame; a block of four waves owns a tile.  A frame is
// `head` single bytes, then nunits = (frame_bytes - head) / U units of U = sizeof(T) bytes, then tail < U single bytes.
// frame_width picks T and head so that every stream in play is a multiple of U at its byte `head`.  A tile is walked in
// steps of FR_THREADS * FR_UNR units; in a step a lane loads FR_UNR units of every stream before it uses any.  The head
// and tail bytes (fewer than 16 each) go to wave 0 of tile 0, one per lane: lane l < 16 takes head byte l, lane 16 + k
// tail byte k.
//
// Bounds.  A stream is read only where frame_in_range(off, bytes, frame_bytes) holds, which cannot overflow.  Within it
// every load lies in [0, frame_bytes): a step hands out unit indices base + u * FR_THREADS + threadIdx.x, and
// frame_loads reads unit i at head + i * U only where i < end <= nunits (FULL: the step's last index is below end); an
// edge byte is at index < head, or at head + nunits * U + k with k < tail, which is below frame_bytes.  With
// frame_bytes <= 2^32 - 2 (frame_bytes_ok) every index fits u32 and none equals FR_NONE.
//
// k_stat (abub_stats.hip) walks through frame_walk.  k_cmp (abub_compare.hip) and k_peek_copy (abub_peek.hip) take the
// range test, the types, constants, reduction and grid from here but keep their own copies of the walk (cmp_tile / cmp_step,
// peek_tile / peek_step): through frame_walk k_cmp's path for a wave that found a difference ran a tenth slower and
// k_peek_copy up to 1.4 % slower (profiles/r22/frames_ab.json), with the same instructions in another allocation.
#ifndef ABUB_FRAMES_HPP
#define ABUB_FRAMES_HPP

#include "abub_dev.hpp"
#include <stddef.h>
#include <type_traits>

namespace {

#define FR_THREADS 256         /* four waves per tile */
#define FR_UNR 4               /* loads of each stream a lane has in flight */
#define FR_TILE 16384u         /* bytes of a frame per block: FR_THREADS * FR_UNR * 16 */
#define FR_NONE 0xffffffffu    /* a lane of wave 0 that has no head or tail byte */

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// [off, off + n) lies inside a buffer of `bytes` bytes
__device__ __forceinline__ bool frame_in_range(uint64_t off, uint64_t bytes, uint64_t n) { return off <= bytes && bytes - off >= n; }

// how many of the four bytes of x are nonzero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x)
{
    uint32_t nz = x | (x >> 4); // bit 8 k set iff byte k of x is nonzero
    nz |= nz >> 2;
    nz |= nz >> 1;
    return (uint32_t)__popc(nz & 0x01010101u);
}

// the three load widths; a kernel derives its own trait from this one and adds its arithmetic
template <class T>
struct FrameUnit {
    static __device__ __forceinline__ T zero() { return T{}; } // (u32x4{}: four zeros)
};

// unit i of a stream; zero where i is not below `end` (FULL: it is) or the stream is not in play
template <bool FULL, class T>
__device__ __forceinline__ T frame_unit(const T *s, uint32_t i, uint32_t end, bool on = true)
{
    return on && (FULL || i < end) ? s[i] : FrameUnit<T>::zero();
}
// one stream's loads of the step that starts at unit `base`
template <bool FULL, class T>
__device__ __forceinline__ void frame_loads(T (&v)[FR_UNR], const T *s, uint32_t base, uint32_t end, bool on = true)
{
#pragma unroll
    for (int u = 0; u < FR_UNR; ++u)
        v[u] = frame_unit<FULL>(s, base + (uint32_t)u * FR_THREADS + threadIdx.x, end, on);
}

// Tile `tile` of a frame in units of T after `head` bytes: step(base, end, full) for every step of the tile that has units
// (full: std::true_type where all FR_THREADS * FR_UNR units from `base` on lie below `end`, the same in every thread of
// the block), then in wave 0 of tile 0 of a frame that has head or tail bytes edge(at): the lane's byte index, or FR_NONE.
template <class T, class Step, class Edge>
__device__ __forceinline__ void frame_walk(uint32_t frame_bytes, uint32_t head, uint32_t tile, Step step, Edge edge)
{
    constexpr uint32_t U = (uint32_t)sizeof(T), PER_TILE = FR_TILE / U, STEP = FR_THREADS * FR_UNR;
    const uint32_t nunits = (frame_bytes - head) / U, tail = frame_bytes - head - nunits * U; // (tail < U <= 16)
    // (tile < 2^18 and PER_TILE <= 2^14: the tile's last unit index stays below 2^32, its end need not)
    const uint32_t end = (uint32_t)min((uint64_t)nunits, (uint64_t)(tile + 1u) * PER_TILE);
    for (uint32_t s = 0; s < PER_TILE / STEP; ++s) {
        const uint32_t base = tile * PER_TILE + s * STEP;
        if (base >= end)
            break;
        if (end - base >= STEP)
            step(base, end, std::true_type());
        else
            step(base, end, std::false_type());
    }
    if (tile == 0 && threadIdx.x < 64 && (head | tail)) { // (the whole wave 0, or none of it)
        const uint32_t l = threadIdx.x;
        edge(l < head ? l : l >= 16u && l - 16u < tail ? head + nunits * U + (l - 16u) : FR_NONE);
    }
}

// The widest unit the streams allow, from the low address bits of the first (`low`) and the bits in which the other
// streams in play differ from it (`apart`): body(T(), head) with T the 16-, 4- or 1-byte unit
template <class Body>
__device__ __forceinline__ void frame_width(uint32_t low, uint32_t apart, uint32_t frame_bytes, Body body)
{
    if ((apart & 15u) == 0u)
        body(u32x4(), min((16u - (low & 15u)) & 15u, frame_bytes));
    else if ((apart & 3u) == 0u)
        body(uint32_t(), min((4u - (low & 3u)) & 3u, frame_bytes));
    else
        body(uint8_t(), 0u);
}

// The xor butterfly over the 64 lanes of a wave for several values at once, value k under operation Op k; every lane calls
// it and gets the results.  (One loop for all values: their shuffles interleave.  One value after the other measured slower.)
struct WaveSum { static __device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b) { return a + b; } };
struct WaveMin { static __device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b) { return min(a, b); } };
struct WaveMax { static __device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b) { return max(a, b); } };
template <class... Op, class... V>
__device__ __forceinline__ void wave_reduce(V &...v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        ((v = Op::op(v, (uint32_t)__shfl_xor(v, o))), ...);
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return wave_reduce<WaveSum>(v), v; }
// the same butterfly for an array of uint32_t or int32_t under one operation (an int32_t sum wraps as the uint32_t sum does)
template <class Op, class T, size_t N>
__device__ __forceinline__ void wave_reduce_all(T (&v)[N])
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (size_t k = 0; k < N; ++k)
            v[k] = (T)Op::op((uint32_t)v[k], (uint32_t)__shfl_xor(v[k], o));
}

// the entries' side: what a frame size and a job list must satisfy, and the grid of a walk over n jobs
inline bool frame_bytes_ok(size_t frame_bytes) { return frame_bytes >= 1 && frame_bytes <= (size_t)0xfffffffeu; }
inline bool frame_lists_aligned(const void *jobs, const void *results) { return (((uintptr_t)jobs | (uintptr_t)results) & 7) == 0; }
inline dim3 frame_grid(size_t frame_bytes, int n) { return dim3((unsigned)((frame_bytes + FR_TILE - 1) / FR_TILE), (unsigned)(n < 65535 ? n : 65535)); }

} // namespace
#endif
