// abub_stats.hip -- per-frame statistics of resident frames: abub_frame_stats_dev (include/abub_hip.h, DESIGN section 3,
// "Surveying a run").  What a byte loop over a decoded frame does on a host thread (host/survey.cpp frameStatsHost, the
// definition): per job the grey-level range, sum, sum of squares, black and saturated pixels of the frame, and against a
// model (mu, sigma6) and a reference frame the count and sum of sat(|p - m| - s) and of sat(|p - r| - s).
//
// The grid is jobs x contiguous 16 KiB tiles of the frame; a block of four waves owns a tile, as in abub_compare.hip.  A
// lane issues ST_UNR independent loads of every stream in play (the frame; with a model mu and sigma6; with a reference
// frame that too) before it uses any.  Sums come from packed-byte instructions (v_sad_u8 against 0, v_dot4_u32_u8 of a
// dword with itself), the clamped differences from u16 pairs (v_pk_sub_i16 / v_pk_max_i16 / v_pk_sub_u16 clamp, as
// k3_bound_scan forms them).  A lane sees at most 64 + 1 bytes of a tile and a block 16 KiB + 30: 16414 * 255^2 < 2^32, so
// every partial sum of a block fits u32.  The lanes' findings are summed over the wave with shuffles, over the four waves
// through LDS, and thread 0 issues one atomic of each kind per block into the job's record: u32 add / min / max and u64
// add (an add of 0 is left out).  All of them commute and every value is an integer, so a record does not depend on the
// order the blocks arrive in, and no workgroup waits for another.
//
// The loads are as wide as the addresses in play allow: 16 bytes where all are congruent mod 16, 4 where congruent mod 4,
// else single bytes; the bytes in front of the first and behind the last whole unit (fewer than 16 each) go to wave 0 of
// tile 0, one per lane.
//
// Bounds.  A job is read only when every stream it names lies inside its buffer: cur + frame_bytes <= frames_bytes; with
// ref != UINT64_MAX, ref + frame_bytes <= frames_bytes; with a model, model + frame_bytes <= model_bytes (each tested as
// off <= bytes && bytes - off >= frame_bytes, which cannot overflow).  Otherwise E_RANGE, found alike by k_stat_init,
// which writes the status and zeroes the rest, and by every block of k_stat, which then goes on to its next job.  Within a
// job every load lies in [0, frame_bytes) of its stream: unit i at head + i * U with i < nunits = (frame_bytes - head) / U,
// head and tail bytes by their own index.  Only results[j] is written, j < njobs.
#include "abub_dev.hpp"
#include <stddef.h>

namespace {

#define ST_THREADS 256 /* four waves per tile */
#define ST_UNR 4       /* loads of each stream a lane has in flight */
#define ST_TILE 16384u /* bytes of a frame per block: ST_THREADS * ST_UNR * 16 */
#define ST_NONE 0xffffffffffffffffull

typedef uint32_t st_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool st_in_range(uint64_t off, uint64_t bytes, uint64_t frame_bytes)
{
    return off <= bytes && bytes - off >= frame_bytes;
}

// which streams a job has, and whether all of them lie inside their buffers
struct StatPlan {
    bool model, ref, ok;
};
__device__ __forceinline__ StatPlan st_plan(const abub_stat_job &jb, bool have_mu, uint64_t frames_bytes, uint64_t model_bytes,
                                            uint64_t frame_bytes)
{
    StatPlan pl;
    pl.model = have_mu && jb.model != ST_NONE;
    pl.ref = jb.ref != ST_NONE;
    pl.ok = st_in_range(jb.cur, frames_bytes, frame_bytes) && (!pl.ref || st_in_range(jb.ref, frames_bytes, frame_bytes)) &&
            (!pl.model || st_in_range(jb.model, model_bytes, frame_bytes));
    return pl;
}

// bytes of x that are zero
__device__ __forceinline__ uint32_t st_zero_bytes(uint32_t x)
{
    uint32_t nz = x | (x >> 4); // bit 8 k set iff byte k of x is nonzero
    nz |= nz >> 2;
    nz |= nz >> 1;
    return 4u - (uint32_t)__popc(nz & 0x01010101u);
}

// two u16 lanes: min(a, 1)  (v_pk_min_u16)
__device__ __forceinline__ uint32_t st_pk_min1(uint32_t a)
{
    const u16x2 one = {1, 1};
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), one));
}

// what one lane found in its (at most 65) bytes of a tile; every field fits u32 for a whole block (header comment)
struct StatAcc {
    uint32_t mn = 255u, mx = 0, n_zero = 0, n_sat = 0, n_out = 0, n_moved = 0, sum = 0, sumsq = 0, sum_out = 0, sum_moved = 0;

    // sat(|p - q| - s) of the four bytes of a dword: how many are nonzero, and their sum
    static __device__ __forceinline__ void clamped(uint32_t p, uint32_t q, uint32_t s, uint32_t &n, uint32_t &total)
    {
        const uint32_t lo = pk_subsat(pk_absdiff(widen_lo(p), widen_lo(q)), widen_lo(s));
        const uint32_t hi = pk_subsat(pk_absdiff(widen_hi(p), widen_hi(q)), widen_hi(s));
        const uint32_t o = lo + hi, c = st_pk_min1(lo) + st_pk_min1(hi); // (lanes <= 510 and <= 2: no carry between them)
        total += (o & 0xffffu) + (o >> 16);
        n += (c & 0xffffu) + (c >> 16);
    }
    template <bool MODEL, bool REF>
    __device__ __forceinline__ void dword(uint32_t p, uint32_t r, uint32_t m, uint32_t s)
    {
        sum = __builtin_amdgcn_sad_u8(p, 0u, sum);
        sumsq = __builtin_amdgcn_udot4(p, p, sumsq, false);
        const uint32_t b0 = p & 0xffu, b1 = (p >> 8) & 0xffu, b2 = (p >> 16) & 0xffu, b3 = p >> 24;
        mn = min(mn, min(min(b0, b1), min(b2, b3)));
        mx = max(mx, max(max(b0, b1), max(b2, b3)));
        n_zero += st_zero_bytes(p);
        n_sat += st_zero_bytes(~p);
        if (MODEL)
            clamped(p, m, s, n_out, sum_out);
        if (REF)
            clamped(p, r, s, n_moved, sum_moved);
    }
    template <bool MODEL, bool REF>
    __device__ __forceinline__ void byte(uint32_t p, uint32_t r, uint32_t m, uint32_t s)
    {
        sum += p;
        sumsq += p * p;
        mn = min(mn, p);
        mx = max(mx, p);
        n_zero += p == 0u;
        n_sat += p == 255u;
        if (MODEL) {
            const uint32_t d = p > m ? p - m : m - p, o = d > s ? d - s : 0u;
            n_out += o != 0u;
            sum_out += o;
        }
        if (REF) {
            const uint32_t d = p > r ? p - r : r - p, o = d > s ? d - s : 0u;
            n_moved += o != 0u;
            sum_moved += o;
        }
    }
};

template <class T>
struct StatUnit;
template <>
struct StatUnit<st_u32x4> {
    static __device__ __forceinline__ st_u32x4 zero() { return st_u32x4{0u, 0u, 0u, 0u}; }
    template <bool MODEL, bool REF>
    static __device__ __forceinline__ void add(StatAcc &c, st_u32x4 p, st_u32x4 r, st_u32x4 m, st_u32x4 s)
    {
        c.dword<MODEL, REF>(p.x, r.x, m.x, s.x);
        c.dword<MODEL, REF>(p.y, r.y, m.y, s.y);
        c.dword<MODEL, REF>(p.z, r.z, m.z, s.z);
        c.dword<MODEL, REF>(p.w, r.w, m.w, s.w);
    }
};
template <>
struct StatUnit<uint32_t> {
    static __device__ __forceinline__ uint32_t zero() { return 0u; }
    template <bool MODEL, bool REF>
    static __device__ __forceinline__ void add(StatAcc &c, uint32_t p, uint32_t r, uint32_t m, uint32_t s)
    {
        c.dword<MODEL, REF>(p, r, m, s);
    }
};
template <>
struct StatUnit<uint8_t> {
    static __device__ __forceinline__ uint8_t zero() { return 0; }
    template <bool MODEL, bool REF>
    static __device__ __forceinline__ void add(StatAcc &c, uint8_t p, uint8_t r, uint8_t m, uint8_t s)
    {
        c.byte<MODEL, REF>(p, r, m, s);
    }
};

// the four streams of a job: the frame, the reference frame, mu and sigma6 (the last three only where the job has them)
struct StatSrc {
    const uint8_t *p, *r, *m, *s;
};

// ST_THREADS * ST_UNR units from `base` on; FULL: all of them lie below `end` (the loads need no guard)
template <class T, bool MODEL, bool REF, bool FULL>
__device__ __forceinline__ void st_step(StatAcc &c, const T *up, const T *ur, const T *um, const T *us, uint32_t base, uint32_t end)
{
    T vp[ST_UNR], vr[ST_UNR], vm[ST_UNR], vs[ST_UNR];
#pragma unroll
    for (int u = 0; u < ST_UNR; ++u) {
        const uint32_t i = base + (uint32_t)u * ST_THREADS + threadIdx.x;
        vp[u] = FULL || i < end ? up[i] : StatUnit<T>::zero();
    }
#pragma unroll
    for (int u = 0; u < ST_UNR; ++u) {
        const uint32_t i = base + (uint32_t)u * ST_THREADS + threadIdx.x;
        vm[u] = MODEL && (FULL || i < end) ? um[i] : StatUnit<T>::zero();
        vs[u] = MODEL && (FULL || i < end) ? us[i] : StatUnit<T>::zero();
    }
#pragma unroll
    for (int u = 0; u < ST_UNR; ++u) {
        const uint32_t i = base + (uint32_t)u * ST_THREADS + threadIdx.x;
        vr[u] = REF && (FULL || i < end) ? ur[i] : StatUnit<T>::zero();
    }
#pragma unroll
    for (int u = 0; u < ST_UNR; ++u) {
        const uint32_t i = base + (uint32_t)u * ST_THREADS + threadIdx.x;
        if (FULL || i < end)
            StatUnit<T>::template add<MODEL, REF>(c, vp[u], vr[u], vm[u], vs[u]);
    }
}

// Tile `tile` of a job whose streams are all multiples of sizeof(T) after `head` bytes -> what this lane found
template <class T, bool MODEL, bool REF>
__device__ __forceinline__ StatAcc st_tile(const StatSrc &src, uint32_t frame_bytes, uint32_t head, uint32_t tile)
{
    constexpr uint32_t U = (uint32_t)sizeof(T), PER_TILE = ST_TILE / U, STEP = ST_THREADS * ST_UNR;
    const uint32_t nunits = (frame_bytes - head) / U, tail = frame_bytes - head - nunits * U; // (tail < U <= 16)
    const T *up = reinterpret_cast<const T *>(src.p + head), *ur = reinterpret_cast<const T *>(src.r + head);
    const T *um = reinterpret_cast<const T *>(src.m + head), *us = reinterpret_cast<const T *>(src.s + head);
    // (tile < 2^18 and PER_TILE <= 2^14: the tile's last unit index stays below 2^32, its end need not)
    const uint32_t end = (uint32_t)min((uint64_t)nunits, (uint64_t)(tile + 1u) * PER_TILE);
    StatAcc c;
    for (uint32_t st = 0; st < PER_TILE / STEP; ++st) {
        const uint32_t base = tile * PER_TILE + st * STEP;
        if (base >= end)
            break;
        if (end - base >= STEP) // (the same in every thread of the block)
            st_step<T, MODEL, REF, true>(c, up, ur, um, us, base, end);
        else
            st_step<T, MODEL, REF, false>(c, up, ur, um, us, base, end);
    }
    if (tile == 0 && threadIdx.x < 64) { // head and tail bytes: wave 0 of tile 0, one per lane
        const uint32_t l = threadIdx.x;
        uint32_t at = 0xffffffffu;
        if (l < head)
            at = l;
        else if (l >= 16u && l - 16u < tail)
            at = head + nunits * U + (l - 16u);
        if (at != 0xffffffffu)
            c.byte<MODEL, REF>(src.p[at], REF ? src.r[at] : 0u, MODEL ? src.m[at] : 0u, MODEL ? src.s[at] : 0u);
    }
    return c;
}

template <bool MODEL, bool REF>
__device__ __forceinline__ StatAcc st_job(const StatSrc &src, uint32_t frame_bytes, uint32_t tile)
{
    const uint32_t lp = (uint32_t)(uintptr_t)src.p;
    uint32_t apart = 0; // the low address bits in which the streams in play differ
    if (MODEL)
        apart |= (lp ^ (uint32_t)(uintptr_t)src.m) | (lp ^ (uint32_t)(uintptr_t)src.s);
    if (REF)
        apart |= lp ^ (uint32_t)(uintptr_t)src.r;
    if ((apart & 15u) == 0u)
        return st_tile<st_u32x4, MODEL, REF>(src, frame_bytes, min((16u - (lp & 15u)) & 15u, frame_bytes), tile);
    if ((apart & 3u) == 0u)
        return st_tile<uint32_t, MODEL, REF>(src, frame_bytes, min((4u - (lp & 3u)) & 3u, frame_bytes), tile);
    return st_tile<uint8_t, MODEL, REF>(src, frame_bytes, 0u, tile);
}

// results[j]: the state k_stat's atomics start from (min 255, the flags of the streams the job has, all else 0), or
// {E_RANGE, all else 0}, the whole answer for a job that is not read
__global__ __launch_bounds__(ST_THREADS) void k_stat_init(uint64_t frames_bytes, bool have_mu, uint64_t model_bytes,
                                                          const abub_stat_job *__restrict__ jobs, int njobs, uint64_t frame_bytes,
                                                          abub_stat_result *__restrict__ results)
{
    const uint64_t j = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (j >= (uint64_t)njobs)
        return;
    const StatPlan pl = st_plan(jobs[j], have_mu, frames_bytes, model_bytes, frame_bytes);
    abub_stat_result r = {};
    if (pl.ok) {
        r.min = 255u;
        r.flags = (pl.model ? ABUB_STAT_F_MODEL : 0u) | (pl.model && pl.ref ? ABUB_STAT_F_REF : 0u);
    } else
        r.status = (uint32_t)ABUB_STAT_E_RANGE;
    results[j] = r;
}

#define ST_NVALS 10
__global__ __launch_bounds__(ST_THREADS) void k_stat(const uint8_t *frames, uint64_t frames_bytes, const uint8_t *mu,
                                                     const uint8_t *sigma6, uint64_t model_bytes,
                                                     const abub_stat_job *__restrict__ jobs, int njobs, uint32_t frame_bytes,
                                                     abub_stat_result *__restrict__ results)
{
    __shared__ uint32_t part[ST_THREADS / 64][ST_NVALS];
    for (uint32_t j = blockIdx.y; j < (uint32_t)njobs; j += gridDim.y) {
        const abub_stat_job jb = jobs[j];
        const StatPlan pl = st_plan(jb, mu != nullptr, frames_bytes, model_bytes, frame_bytes);
        if (!pl.ok)
            continue; // (the same in every thread of every block of the job)
        StatSrc src;
        src.p = frames + jb.cur;
        src.m = pl.model ? mu + jb.model : src.p;
        src.s = pl.model ? sigma6 + jb.model : src.p;
        src.r = pl.model && pl.ref ? frames + jb.ref : src.p;
        StatAcc c = !pl.model ? st_job<false, false>(src, frame_bytes, blockIdx.x)
                    : pl.ref  ? st_job<true, true>(src, frame_bytes, blockIdx.x)
                              : st_job<true, false>(src, frame_bytes, blockIdx.x);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            c.mn = min(c.mn, (uint32_t)__shfl_xor(c.mn, o));
            c.mx = max(c.mx, (uint32_t)__shfl_xor(c.mx, o));
            c.n_zero += __shfl_xor(c.n_zero, o);
            c.n_sat += __shfl_xor(c.n_sat, o);
            c.n_out += __shfl_xor(c.n_out, o);
            c.n_moved += __shfl_xor(c.n_moved, o);
            c.sum += __shfl_xor(c.sum, o);
            c.sumsq += __shfl_xor(c.sumsq, o);
            c.sum_out += __shfl_xor(c.sum_out, o);
            c.sum_moved += __shfl_xor(c.sum_moved, o);
        }
        if ((threadIdx.x & 63) == 0) {
            uint32_t *w = part[threadIdx.x >> 6];
            w[0] = c.mn, w[1] = c.mx, w[2] = c.n_zero, w[3] = c.n_sat, w[4] = c.n_out;
            w[5] = c.n_moved, w[6] = c.sum, w[7] = c.sumsq, w[8] = c.sum_out, w[9] = c.sum_moved;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t v[ST_NVALS];
#pragma unroll
            for (int k = 0; k < ST_NVALS; ++k) {
                v[k] = part[0][k];
#pragma unroll
                for (int w = 1; w < ST_THREADS / 64; ++w)
                    v[k] = k == 0 ? min(v[k], part[w][k]) : k == 1 ? max(v[k], part[w][k]) : v[k] + part[w][k];
            }
            abub_stat_result *r = results + j;
            atomicMin(&r->min, v[0]);
            atomicMax(&r->max, v[1]);
            uint32_t *const n32[4] = {&r->n_zero, &r->n_sat, &r->n_out, &r->n_moved};
            unsigned long long *const n64[4] = {(unsigned long long *)&r->sum, (unsigned long long *)&r->sumsq,
                                                (unsigned long long *)&r->sum_out, (unsigned long long *)&r->sum_moved};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (v[2 + k])
                    atomicAdd(n32[k], v[2 + k]);
                if (v[6 + k])
                    atomicAdd(n64[k], (unsigned long long)v[6 + k]);
            }
        }
        __syncthreads(); // (part is written again for the block's next job)
    }
}

} // namespace

extern "C" int abub_frame_stats_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, const uint8_t *sigma6,
                                    size_t model_bytes, const abub_stat_job *jobs, int njobs, size_t frame_bytes,
                                    abub_stat_result *results, void *stream)
{
    if (!frames || !jobs || !results || njobs < 0 || (mu && !sigma6))
        return set_err(ABUB_E_INVALID, "abub_frame_stats_dev: null pointer or negative count");
    if (frame_bytes < 1 || frame_bytes > (size_t)0xfffffffeu)
        return set_err(ABUB_E_INVALID, "abub_frame_stats_dev: frame_bytes must be in [1, 2^32 - 2]");
    if (((uintptr_t)jobs | (uintptr_t)results) & 7)
        return set_err(ABUB_E_INVALID, "abub_frame_stats_dev: jobs and results must be 8-byte aligned");
    if (njobs == 0)
        return ABUB_OK;
    hipStream_t st = (hipStream_t)stream;
    k_stat_init<<<(unsigned)(((size_t)njobs + ST_THREADS - 1) / ST_THREADS), ST_THREADS, 0, st>>>(
        (uint64_t)frames_bytes, mu != nullptr, (uint64_t)model_bytes, jobs, njobs, (uint64_t)frame_bytes, results);
    HIPCHK(hipGetLastError());
    const dim3 grid((unsigned)((frame_bytes + ST_TILE - 1) / ST_TILE), (unsigned)(njobs < 65535 ? njobs : 65535));
    k_stat<<<grid, ST_THREADS, 0, st>>>(frames, (uint64_t)frames_bytes, mu, sigma6, (uint64_t)model_bytes, jobs, njobs,
                                        (uint32_t)frame_bytes, results);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}
