// abub_compare.hip -- resident frames compared byte for byte: abub_frames_compare_dev (include/abub_hip.h, DESIGN section 3,
// "Verifying a repacked run").  What memcmp of two decoded frames plus a byte loop does on a host thread: per pair the
// number of differing bytes, the lowest differing index and the largest |a[i] - b[i]|.
//
// The grid is pairs x contiguous 16 KiB tiles of the frame; a block of four waves owns a tile.  A lane issues FR_UNR
// independent loads of each side before it uses any (the shape of read_guide in tools/rowload_bench), ORs the XORs
// together, and one ballot decides for the whole wave that its part of the tile is clean: a clean wave issues no atomic,
// so identical frames touch their record only through k_cmp_init.  A wave that saw a difference counts the nonzero bytes
// of the XOR, reduces (sum, min, max) over its lanes and issues one atomicAdd, one atomicMin and one atomicMax: all three
// commute, so a record does not depend on the order the waves arrive in.  No workgroup waits for another.
//
// The loads are as wide as the two frame addresses allow: 16 bytes where they are congruent mod 16, 4 where congruent mod
// 4, else single bytes; the bytes in front of the first and behind the last whole unit (fewer than 16 each) go to wave 0
// of tile 0, one per lane.
//
// Bounds.  A pair is read only when a + frame_bytes <= a_bytes and b + frame_bytes <= b_bytes (frame_in_range; E_RANGE
// otherwise, found alike by k_cmp_init, which writes the status, and by every block of k_cmp, which then returns).  Within
// a pair every load lies in [0, frame_bytes) of its frame, by the reasoning of abub_frames.hpp: cmp_tile and cmp_step are
// this kernel's own copy of frame_walk and frame_loads (see there: with the shared walk the path of a wave that found a
// difference measured a tenth slower, so this one kernel keeps its walker).  Only results[pair] is written, pair < npairs.
#include "abub_frames.hpp"

namespace {

// what one lane found: bytes that differ, the lowest index among them, the largest difference
struct CmpAcc {
    uint32_t n = 0, first = 0xffffffffu, mx = 0;
    // the four bytes of a dword that starts at index `at`
    __device__ __forceinline__ void dword(uint32_t wa, uint32_t wb, uint32_t at)
    {
        const uint32_t x = wa ^ wb;
        if (!x)
            return;
        n += nonzero_bytes(x);
        first = min(first, at + (((uint32_t)__ffs((int)x) - 1u) >> 3)); // (little endian: the lowest byte has the lowest index)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d = (int)((wa >> (8 * k)) & 0xffu) - (int)((wb >> (8 * k)) & 0xffu);
            mx = max(mx, (uint32_t)(d < 0 ? -d : d));
        }
    }
    __device__ __forceinline__ void byte(uint32_t ba, uint32_t bb, uint32_t at)
    {
        if (ba == bb)
            return;
        ++n;
        first = min(first, at);
        mx = max(mx, ba > bb ? ba - bb : bb - ba);
    }
};

// The lanes' findings into the pair's record: one atomic of each kind per wave.  Every lane of the wave calls it.
__device__ __forceinline__ void cmp_commit(CmpAcc c, abub_cmp_result *__restrict__ r)
{
    wave_reduce<WaveSum, WaveMin, WaveMax>(c.n, c.first, c.mx);
    if ((threadIdx.x & 63) == 0 && c.n) {
        atomicAdd(&r->ndiff, c.n);
        atomicMin(&r->first, c.first);
        atomicMax(&r->max_abs, c.mx);
    }
}

template <class T>
struct CmpUnit;
template <>
struct CmpUnit<u32x4> : FrameUnit<u32x4> {
    static __device__ __forceinline__ uint32_t any(u32x4 a, u32x4 b)
    {
        const u32x4 x = a ^ b;
        return x.x | x.y | x.z | x.w;
    }
    static __device__ __forceinline__ void slow(CmpAcc &c, u32x4 a, u32x4 b, uint32_t at)
    {
        c.dword(a.x, b.x, at);
        c.dword(a.y, b.y, at + 4u);
        c.dword(a.z, b.z, at + 8u);
        c.dword(a.w, b.w, at + 12u);
    }
};
template <>
struct CmpUnit<uint32_t> : FrameUnit<uint32_t> {
    static __device__ __forceinline__ uint32_t any(uint32_t a, uint32_t b) { return a ^ b; }
    static __device__ __forceinline__ void slow(CmpAcc &c, uint32_t a, uint32_t b, uint32_t at) { c.dword(a, b, at); }
};
template <>
struct CmpUnit<uint8_t> : FrameUnit<uint8_t> {
    static __device__ __forceinline__ uint32_t any(uint8_t a, uint8_t b) { return (uint32_t)(a ^ b); }
    static __device__ __forceinline__ void slow(CmpAcc &c, uint8_t a, uint8_t b, uint32_t at) { c.byte(a, b, at); }
};

// FR_THREADS * FR_UNR units from `base` on; FULL: all of them lie below `end` (the loads need no guard)
template <class T, bool FULL>
__device__ __forceinline__ void cmp_step(const T *ua, const T *ub, uint32_t base, uint32_t end, uint32_t head,
                                         abub_cmp_result *__restrict__ r)
{
    constexpr uint32_t U = (uint32_t)sizeof(T);
    T va[FR_UNR], vb[FR_UNR];
#pragma unroll
    for (int u = 0; u < FR_UNR; ++u) {
        const uint32_t i = base + (uint32_t)u * FR_THREADS + threadIdx.x;
        va[u] = FULL || i < end ? ua[i] : CmpUnit<T>::zero();
    }
#pragma unroll
    for (int u = 0; u < FR_UNR; ++u) {
        const uint32_t i = base + (uint32_t)u * FR_THREADS + threadIdx.x;
        vb[u] = FULL || i < end ? ub[i] : CmpUnit<T>::zero();
    }
    uint32_t x = 0;
#pragma unroll
    for (int u = 0; u < FR_UNR; ++u)
        x |= CmpUnit<T>::any(va[u], vb[u]);
    if (__ballot(x != 0u) == 0ull)
        return; // (the same in every lane of the wave)
    CmpAcc c;
#pragma unroll
    for (int u = 0; u < FR_UNR; ++u) {
        const uint32_t i = base + (uint32_t)u * FR_THREADS + threadIdx.x;
        CmpUnit<T>::slow(c, va[u], vb[u], head + i * U); // (equal where i >= end: both are zero)
    }
    cmp_commit(c, r);
}

// Tile `tile` of a pair whose frames start at pa and pb, both multiples of sizeof(T) after `head` bytes
template <class T>
__device__ __forceinline__ void cmp_tile(const uint8_t *pa, const uint8_t *pb, uint32_t frame_bytes, uint32_t head, uint32_t tile,
                                         abub_cmp_result *__restrict__ r)
{
    constexpr uint32_t U = (uint32_t)sizeof(T), PER_TILE = FR_TILE / U, STEP = FR_THREADS * FR_UNR;
    const uint32_t nunits = (frame_bytes - head) / U, tail = frame_bytes - head - nunits * U; // (tail < U <= 16)
    const T *ua = reinterpret_cast<const T *>(pa + head), *ub = reinterpret_cast<const T *>(pb + head);
    // (tile < 2^18 and PER_TILE <= 2^14: the tile's last unit index stays below 2^32, its end need not)
    const uint32_t end = (uint32_t)min((uint64_t)nunits, (uint64_t)(tile + 1u) * PER_TILE);
    for (uint32_t s = 0; s < PER_TILE / STEP; ++s) {
        const uint32_t base = tile * PER_TILE + s * STEP;
        if (base >= end)
            break;
        if (end - base >= STEP) // (the same in every thread of the block)
            cmp_step<T, true>(ua, ub, base, end, head, r);
        else
            cmp_step<T, false>(ua, ub, base, end, head, r);
    }
    if (tile == 0 && threadIdx.x < 64 && (head | tail)) { // (the whole wave 0, or none of it)
        const uint32_t l = threadIdx.x;
        CmpAcc c;
        if (l < head)
            c.byte(pa[l], pb[l], l);
        else if (l >= 16u && l - 16u < tail) {
            const uint32_t at = head + nunits * U + (l - 16u);
            c.byte(pa[at], pb[at], at);
        }
        cmp_commit(c, r);
    }
}

// results[p] = {0 or E_RANGE, 0, 0xffffffff, 0}: the state k_cmp's atomics start from, and the whole answer for a pair that
// is not read
__global__ __launch_bounds__(FR_THREADS) void k_cmp_init(uint64_t a_bytes, uint64_t b_bytes, const abub_cmp_pair *__restrict__ pairs,
                                                          int npairs, uint64_t frame_bytes, abub_cmp_result *__restrict__ results)
{
    const uint64_t p = (uint64_t)blockIdx.x * FR_THREADS + threadIdx.x;
    if (p >= (uint64_t)npairs)
        return;
    const abub_cmp_pair pr = pairs[p];
    abub_cmp_result r;
    r.status = frame_in_range(pr.a, a_bytes, frame_bytes) && frame_in_range(pr.b, b_bytes, frame_bytes) ? 0u : (uint32_t)ABUB_CMP_E_RANGE;
    r.ndiff = 0;
    r.first = 0xffffffffu;
    r.max_abs = 0;
    results[p] = r;
}

__global__ __launch_bounds__(FR_THREADS) void k_cmp(const uint8_t *a, uint64_t a_bytes, const uint8_t *b, uint64_t b_bytes,
                                                     const abub_cmp_pair *__restrict__ pairs, int npairs, uint32_t frame_bytes,
                                                     abub_cmp_result *__restrict__ results)
{
    for (uint32_t p = blockIdx.y; p < (uint32_t)npairs; p += gridDim.y) {
        const abub_cmp_pair pr = pairs[p];
        if (!frame_in_range(pr.a, a_bytes, frame_bytes) || !frame_in_range(pr.b, b_bytes, frame_bytes))
            continue; // (the same in every thread of every block of the pair)
        const uint8_t *pa = a + pr.a, *pb = b + pr.b;
        const uint32_t la = (uint32_t)(uintptr_t)pa, lb = (uint32_t)(uintptr_t)pb;
        abub_cmp_result *r = results + p;
        if (((la ^ lb) & 15u) == 0u)
            cmp_tile<u32x4>(pa, pb, frame_bytes, min((16u - (la & 15u)) & 15u, frame_bytes), blockIdx.x, r);
        else if (((la ^ lb) & 3u) == 0u)
            cmp_tile<uint32_t>(pa, pb, frame_bytes, min((4u - (la & 3u)) & 3u, frame_bytes), blockIdx.x, r);
        else
            cmp_tile<uint8_t>(pa, pb, frame_bytes, 0u, blockIdx.x, r);
    }
}

} // namespace

extern "C" int abub_frames_compare_dev(const uint8_t *a, size_t a_bytes, const uint8_t *b, size_t b_bytes, const abub_cmp_pair *pairs,
                                       int npairs, size_t frame_bytes, abub_cmp_result *results, void *stream)
{
    if (!a || !b || !pairs || !results || npairs < 0)
        return set_err(ABUB_E_INVALID, "abub_frames_compare_dev: null pointer or negative count");
    if (!frame_bytes_ok(frame_bytes))
        return set_err(ABUB_E_INVALID, "abub_frames_compare_dev: frame_bytes must be in [1, 2^32 - 2]");
    if (!frame_lists_aligned(pairs, results))
        return set_err(ABUB_E_INVALID, "abub_frames_compare_dev: pairs and results must be 8-byte aligned");
    if (npairs == 0)
        return ABUB_OK;
    hipStream_t st = (hipStream_t)stream;
    k_cmp_init<<<(unsigned)(((size_t)npairs + FR_THREADS - 1) / FR_THREADS), FR_THREADS, 0, st>>>(
        (uint64_t)a_bytes, (uint64_t)b_bytes, pairs, npairs, (uint64_t)frame_bytes, results);
    HIPCHK(hipGetLastError());
    k_cmp<<<frame_grid(frame_bytes, npairs), FR_THREADS, 0, st>>>(a, (uint64_t)a_bytes, b, (uint64_t)b_bytes, pairs, npairs,
                                                                  (uint32_t)frame_bytes, results);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}
