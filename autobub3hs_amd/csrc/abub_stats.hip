// abub_stats.hip -- per-frame statistics of resident frames: abub_frame_stats_dev (include/abub_hip.h, DESIGN section 3,
// "Surveying a run"); below it the per-pixel planes (abub_pixel_activity_dev), the shift search (abub_frame_shift_dev) and
// the per-cell shift field (abub_frame_shift_cells_dev), the per-cell light record (abub_frame_light_cells_dev), the
// per-cell edge agreement (abub_frame_focus_cells_dev), the per-cell noise record (abub_frame_noise_cells_dev) and the per-line sums
// (abub_frame_lines_dev), each under a header of its own.  What a byte loop over a decoded frame does on a host thread (host/survey.cpp frameStatsHost, the
// definition): per job the grey-level range, sum, sum of squares, black and saturated pixels of the frame, and against a
// model (mu, sigma6) and a reference frame the count and sum of sat(|p - m| - s) and of sat(|p - r| - s).
//
// The grid is jobs x contiguous 16 KiB tiles of the frame; a block of four waves owns a tile, as in abub_compare.hip.  A
// lane issues FR_UNR independent loads of every stream in play (the frame; with a model mu and sigma6; with a reference
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
// ref != UINT64_MAX, ref + frame_bytes <= frames_bytes; with a model, model + frame_bytes <= model_bytes.  Otherwise
// E_RANGE, found alike by k_stat_init, which writes the status and zeroes the rest, and by every block of k_stat, which
// then goes on to its next job.  Within a job every load lies in [0, frame_bytes) of its stream: the walk of
// abub_frames.hpp.  Only results[j] is written, j < njobs.
#include "abub_frames.hpp"
#include <algorithm>

namespace {

#define ST_NONE 0xffffffffffffffffull /* a job without that stream */

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
    pl.ok = frame_in_range(jb.cur, frames_bytes, frame_bytes) && (!pl.ref || frame_in_range(jb.ref, frames_bytes, frame_bytes)) &&
            (!pl.model || frame_in_range(jb.model, model_bytes, frame_bytes));
    return pl;
}

// what one lane found in its (at most 65) bytes of a tile; every field fits u32 for a whole block (header comment)
struct StatAcc {
    uint32_t mn = 255u, mx = 0, n_zero = 0, n_sat = 0, n_out = 0, n_moved = 0, sum = 0, sumsq = 0, sum_out = 0, sum_moved = 0;

    // sat(|p - q| - s) of the four bytes of a dword: how many are nonzero, and their sum
    static __device__ __forceinline__ void clamped(uint32_t p, uint32_t q, uint32_t s, uint32_t &n, uint32_t &total)
    {
        const uint32_t lo = pk_subsat(pk_absdiff(widen_lo(p), widen_lo(q)), widen_lo(s));
        const uint32_t hi = pk_subsat(pk_absdiff(widen_hi(p), widen_hi(q)), widen_hi(s));
        const uint32_t o = lo + hi, c = pk_min1(lo) + pk_min1(hi); // (lanes <= 510 and <= 2: no carry between them)
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
        n_zero += 4u - nonzero_bytes(p);
        n_sat += 4u - nonzero_bytes(~p);
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

// what a unit of each width adds
template <bool MODEL, bool REF>
__device__ __forceinline__ void st_add(StatAcc &c, u32x4 p, u32x4 r, u32x4 m, u32x4 s)
{
    c.dword<MODEL, REF>(p.x, r.x, m.x, s.x);
    c.dword<MODEL, REF>(p.y, r.y, m.y, s.y);
    c.dword<MODEL, REF>(p.z, r.z, m.z, s.z);
    c.dword<MODEL, REF>(p.w, r.w, m.w, s.w);
}
template <bool MODEL, bool REF>
__device__ __forceinline__ void st_add(StatAcc &c, uint32_t p, uint32_t r, uint32_t m, uint32_t s) { c.dword<MODEL, REF>(p, r, m, s); }
template <bool MODEL, bool REF>
__device__ __forceinline__ void st_add(StatAcc &c, uint8_t p, uint8_t r, uint8_t m, uint8_t s) { c.byte<MODEL, REF>(p, r, m, s); }

// the four streams of a job: the frame, the reference frame, mu and sigma6 (the last three only where the job has them)
struct StatSrc {
    const uint8_t *p, *r, *m, *s;
};

// Tile `tile` of a job -> what this lane found
template <bool MODEL, bool REF>
__device__ __forceinline__ StatAcc st_job(const StatSrc &src, uint32_t frame_bytes, uint32_t tile)
{
    const uint32_t lp = (uint32_t)(uintptr_t)src.p;
    uint32_t apart = 0; // the low address bits in which the streams in play differ
    if (MODEL)
        apart |= (lp ^ (uint32_t)(uintptr_t)src.m) | (lp ^ (uint32_t)(uintptr_t)src.s);
    if (REF)
        apart |= lp ^ (uint32_t)(uintptr_t)src.r;
    StatAcc c;
    frame_width(lp, apart, frame_bytes, [&](auto unit, uint32_t head) {
        typedef decltype(unit) T;
        const T *up = reinterpret_cast<const T *>(src.p + head), *ur = reinterpret_cast<const T *>(src.r + head);
        const T *um = reinterpret_cast<const T *>(src.m + head), *us = reinterpret_cast<const T *>(src.s + head);
        frame_walk<T>(
            frame_bytes, head, tile,
            [&](uint32_t base, uint32_t end, auto full) {
                T vp[FR_UNR], vr[FR_UNR], vm[FR_UNR], vs[FR_UNR];
                frame_loads<full>(vp, up, base, end);
#pragma unroll
                for (int u = 0; u < FR_UNR; ++u) { // (mu and sigma6 of a unit one after the other)
                    const uint32_t i = base + (uint32_t)u * FR_THREADS + threadIdx.x;
                    vm[u] = frame_unit<full>(um, i, end, MODEL);
                    vs[u] = frame_unit<full>(us, i, end, MODEL);
                }
                frame_loads<full>(vr, ur, base, end, REF);
#pragma unroll
                for (int u = 0; u < FR_UNR; ++u)
                    if (full || base + (uint32_t)u * FR_THREADS + threadIdx.x < end)
                        st_add<MODEL, REF>(c, vp[u], vr[u], vm[u], vs[u]);
            },
            [&](uint32_t at) {
                if (at != FR_NONE)
                    c.byte<MODEL, REF>(src.p[at], REF ? src.r[at] : 0u, MODEL ? src.m[at] : 0u, MODEL ? src.s[at] : 0u);
            });
    });
    return c;
}

// results[j]: the state k_stat's atomics start from (min 255, the flags of the streams the job has, all else 0), or
// {E_RANGE, all else 0}, the whole answer for a job that is not read
__global__ __launch_bounds__(FR_THREADS) void k_stat_init(uint64_t frames_bytes, bool have_mu, uint64_t model_bytes,
                                                          const abub_stat_job *__restrict__ jobs, int njobs, uint64_t frame_bytes,
                                                          abub_stat_result *__restrict__ results)
{
    const uint64_t j = (uint64_t)blockIdx.x * FR_THREADS + threadIdx.x;
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
__global__ __launch_bounds__(FR_THREADS) void k_stat(const uint8_t *frames, uint64_t frames_bytes, const uint8_t *mu,
                                                     const uint8_t *sigma6, uint64_t model_bytes,
                                                     const abub_stat_job *__restrict__ jobs, int njobs, uint32_t frame_bytes,
                                                     abub_stat_result *__restrict__ results)
{
    __shared__ uint32_t part[FR_THREADS / 64][ST_NVALS];
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
        wave_reduce<WaveMin, WaveMax, WaveSum, WaveSum, WaveSum, WaveSum, WaveSum, WaveSum, WaveSum, WaveSum>(
            c.mn, c.mx, c.n_zero, c.n_sat, c.n_out, c.n_moved, c.sum, c.sumsq, c.sum_out, c.sum_moved);
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
                for (int w = 1; w < FR_THREADS / 64; ++w)
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
    if (!frame_bytes_ok(frame_bytes))
        return set_err(ABUB_E_INVALID, "abub_frame_stats_dev: frame_bytes must be in [1, 2^32 - 2]");
    if (!frame_lists_aligned(jobs, results))
        return set_err(ABUB_E_INVALID, "abub_frame_stats_dev: jobs and results must be 8-byte aligned");
    if (njobs == 0)
        return ABUB_OK;
    hipStream_t st = (hipStream_t)stream;
    k_stat_init<<<(unsigned)(((size_t)njobs + FR_THREADS - 1) / FR_THREADS), FR_THREADS, 0, st>>>(
        (uint64_t)frames_bytes, mu != nullptr, (uint64_t)model_bytes, jobs, njobs, (uint64_t)frame_bytes, results);
    HIPCHK(hipGetLastError());
    k_stat<<<frame_grid(frame_bytes, njobs), FR_THREADS, 0, st>>>(frames, (uint64_t)frames_bytes, mu, sigma6, (uint64_t)model_bytes, jobs,
                                                                  njobs, (uint32_t)frame_bytes, results);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}

// ---- per-pixel activity planes: abub_pixel_activity_dev ("Surveying a run per pixel") ------------------
// The sum across the frames of a camera that the per-frame records form across the pixels of a frame (host/survey.cpp
// activityAddHost, the definition): six u32 planes, += per job: p == 0, p == 255, and with a model count and sum of
// sat(|p - m| - s), with a reference frame too count and sum of sat(|p - r| - s).
//
// A thread owns AC_PX = 8 consecutive pixels for the whole call and walks the jobs in list order with its 6 x 8 sums in
// registers; mu and sigma6 of its pixels are loaded once.  Every plane word has one owner, so nothing is atomic and the
// planes are read and written once per call.  The jobs go in groups of AC_UNR: the loads of the next group (one 8-byte load
// of the frame and one of the reference frame per job) are issued before the arithmetic of the current one.  Inside a group
// the clamped differences stay u16 pairs (widen / v_pk_sub_i16 / v_pk_max_i16 / v_pk_sub_u16 clamp, as k_stat forms them;
// a lane <= AC_UNR * 255) and are taken apart into the u32 sums once per group.  Planes 0 and 1 count the bytes that are NOT
// 0 / 255 (min(x, 1) of the widened byte and of its complement) and are turned round at the end with the number of jobs read.
//
// Pixels: with `head` = the bytes in front of the first multiple of 8 of the anchor stream (mu, without a model the frames'
// base), thread t of k_act<8> owns [head + 8 t, head + 8 t + 8), t < nunits = (frame_bytes - head) / 8; the head bytes and
// the tail bytes behind the last unit (at most 7 each) are single pixels of k_act<1>, one thread each.  A unit of a stream
// is read by one 8-byte load where its address is a multiple of 8, by two 4-byte loads where of 4, else byte by byte; the
// address's low bits are those of (base + offset + head), the same in every thread, so that choice is a scalar branch.
//
// Bounds.  A job is read only if cur, and ref where it is not UINT64_MAX, lie inside `frames` (frame_in_range);
// otherwise it adds nothing, and thread 0 of block 0 stores ABUB_ACT_E_RANGE to *status (the entry clears it on the stream
// first).  That is decided from the job record alone, before any add, alike in every thread.  Every load of a stream is at
// pixel index < frame_bytes; the only stores are planes[k * plane_stride + i], k < 6, i < frame_bytes, and *status.
namespace {

#define AC_THREADS 256
#define AC_PX 8  /* pixels a thread of the wide kernel owns: one 8-byte load per stream and job */
#define AC_UNR 4 /* jobs whose loads a thread has in flight */

template <int PX>
struct ActUnit; // PX consecutive bytes of a stream, as PX / 4 dwords (PX = 1: the byte in the low bits of one)
template <>
struct ActUnit<8> {
    static constexpr int NPK = 4; // u16 pairs
    uint32_t w[2];
    static __device__ __forceinline__ ActUnit load(const uint8_t *p, uint32_t low)
    {
        ActUnit u;
        if ((low & 7u) == 0u) {
            const uint2 v = *reinterpret_cast<const uint2 *>(p);
            u.w[0] = v.x, u.w[1] = v.y;
        } else if ((low & 3u) == 0u) {
            u.w[0] = reinterpret_cast<const uint32_t *>(p)[0];
            u.w[1] = reinterpret_cast<const uint32_t *>(p)[1];
        } else {
            u.w[0] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
            u.w[1] = (uint32_t)p[4] | (uint32_t)p[5] << 8 | (uint32_t)p[6] << 16 | (uint32_t)p[7] << 24;
        }
        return u;
    }
    // the u16 pairs of the unit: pair k holds pixels 2 k (low lane) and 2 k + 1
    __device__ __forceinline__ uint32_t pair(int k) const { return k & 1 ? widen_hi(w[k >> 1]) : widen_lo(w[k >> 1]); }
    __device__ __forceinline__ ActUnit inverted() const
    {
        ActUnit u;
        u.w[0] = ~w[0], u.w[1] = ~w[1];
        return u;
    }
};
template <>
struct ActUnit<1> {
    static constexpr int NPK = 1;
    uint32_t w[1];
    static __device__ __forceinline__ ActUnit load(const uint8_t *p, uint32_t)
    {
        ActUnit u;
        u.w[0] = *p;
        return u;
    }
    __device__ __forceinline__ uint32_t pair(int) const { return w[0]; } // (the high lane stays 0 throughout)
    __device__ __forceinline__ ActUnit inverted() const
    {
        ActUnit u;
        u.w[0] = w[0] ^ 0xffu;
        return u;
    }
};

// what a group of AC_UNR jobs is: per job whether it is read and whether it has a reference frame, and their offsets
struct ActGroup {
    uint64_t cur[AC_UNR], ref[AC_UNR];
    bool ok[AC_UNR], has_ref[AC_UNR];
    bool bad; // a job of the group names a stream that runs past `frames`
};
template <bool MODEL>
__device__ __forceinline__ ActGroup act_group(const abub_act_job *__restrict__ jobs, int njobs, int j0, uint64_t frames_bytes,
                                              uint64_t frame_bytes)
{
    ActGroup g;
    g.bad = false;
#pragma unroll
    for (int u = 0; u < AC_UNR; ++u) {
        g.ok[u] = g.has_ref[u] = false;
        g.cur[u] = g.ref[u] = 0;
        if (j0 + u >= njobs)
            continue;
        const abub_act_job jb = jobs[j0 + u];
        const bool ref = jb.ref != ST_NONE;
        if (!frame_in_range(jb.cur, frames_bytes, frame_bytes) || (ref && !frame_in_range(jb.ref, frames_bytes, frame_bytes))) {
            g.bad = true;
            continue;
        }
        g.ok[u] = true;
        g.has_ref[u] = MODEL && ref;
        g.cur[u] = jb.cur;
        g.ref[u] = g.has_ref[u] ? jb.ref : jb.cur;
    }
    return g;
}

// `at`: this thread's first pixel, whose low three bits are those of `head` in every thread of the wide kernel.  The loads
// of every job of the group that is read
template <int PX>
__device__ __forceinline__ void act_loads(const ActGroup &g, const uint8_t *frames, uint64_t at, uint32_t head, ActUnit<PX> *c,
                                          ActUnit<PX> *r)
{
    const uint32_t base = (uint32_t)(uintptr_t)frames + head;
#pragma unroll
    for (int u = 0; u < AC_UNR; ++u)
        if (g.ok[u])
            c[u] = ActUnit<PX>::load(frames + g.cur[u] + at, base + (uint32_t)g.cur[u]);
#pragma unroll
    for (int u = 0; u < AC_UNR; ++u)
        if (g.has_ref[u])
            r[u] = ActUnit<PX>::load(frames + g.ref[u] + at, base + (uint32_t)g.ref[u]);
}

// Grid: x over the threads' units.  PX = 8: unit t is the pixels [head + 8 t, + 8), t < count.  PX = 1: unit t is the
// pixel t for t < head, else body_end + (t - head): the head and tail bytes, count of them in all
template <int PX, bool MODEL>
__global__ __launch_bounds__(AC_THREADS) void k_act(const uint8_t *frames, uint64_t frames_bytes, const uint8_t *mu,
                                                    const uint8_t *sigma6, const abub_act_job *__restrict__ jobs, int njobs,
                                                    uint64_t frame_bytes, uint32_t head, uint64_t body_end, uint64_t count,
                                                    uint32_t *planes, uint64_t plane_stride, uint32_t *status)
{
    typedef ActUnit<PX> Unit;
    constexpr int NPK = Unit::NPK;
    const uint64_t t = (uint64_t)blockIdx.x * AC_THREADS + threadIdx.x;
    const bool mine = t < count;
    // (a thread past the end works on unit 0's addresses and stores nothing: every load stays in bounds)
    const uint64_t unit = mine ? t : 0;
    const uint64_t at = PX == 1 ? (unit < head ? unit : body_end + (unit - head)) : (uint64_t)head + unit * PX;

    uint32_t mp[NPK], sp[NPK]; // mu and sigma6 of the unit as u16 pairs
    if (MODEL) {
        const Unit m = Unit::load(mu + at, (uint32_t)(uintptr_t)mu + head);
        const Unit s = Unit::load(sigma6 + at, (uint32_t)(uintptr_t)sigma6 + head);
#pragma unroll
        for (int k = 0; k < NPK; ++k)
            mp[k] = m.pair(k), sp[k] = s.pair(k);
    }
    // sums per pixel: [plane][pixel]; planes 0 and 1 hold the jobs in which the pixel was NOT 0 / 255 until the end
    uint32_t acc[6][2 * NPK];
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int i = 0; i < 2 * NPK; ++i)
            acc[k][i] = 0;
    uint32_t n_read = 0, bad = 0; // jobs read; a job was refused (the same in every thread)

    Unit c[AC_UNR], r[AC_UNR], cn[AC_UNR], rn[AC_UNR];
#pragma unroll
    for (int u = 0; u < AC_UNR; ++u)
        c[u] = r[u] = cn[u] = rn[u] = Unit();
    ActGroup g = act_group<MODEL>(jobs, njobs, 0, frames_bytes, frame_bytes);
    act_loads<PX>(g, frames, at, head, c, r);
    for (int64_t j0 = 0; j0 < njobs; j0 += AC_UNR) {
        ActGroup gn = g;
        if (j0 + AC_UNR < njobs) { // the next group's loads, before this group's arithmetic
            gn = act_group<MODEL>(jobs, njobs, (int)(j0 + AC_UNR), frames_bytes, frame_bytes);
            act_loads<PX>(gn, frames, at, head, cn, rn);
        }
        bad |= g.bad;
        uint32_t pk[6][NPK]; // the group's sums as u16 pairs (a lane <= AC_UNR * 255)
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
            for (int i = 0; i < NPK; ++i)
                pk[k][i] = 0;
#pragma unroll
        for (int u = 0; u < AC_UNR; ++u) {
            if (!g.ok[u])
                continue;
            ++n_read;
            const Unit inv = c[u].inverted();
#pragma unroll
            for (int i = 0; i < NPK; ++i) {
                const uint32_t p = c[u].pair(i);
                pk[0][i] += pk_min1(p);
                pk[1][i] += pk_min1(inv.pair(i));
                if (MODEL) {
                    const uint32_t o = pk_subsat(pk_absdiff(p, mp[i]), sp[i]);
                    pk[2][i] += pk_min1(o);
                    pk[3][i] += o;
                }
            }
            if (MODEL && g.has_ref[u]) {
#pragma unroll
                for (int i = 0; i < NPK; ++i) {
                    const uint32_t o = pk_subsat(pk_absdiff(c[u].pair(i), r[u].pair(i)), sp[i]);
                    pk[4][i] += pk_min1(o);
                    pk[5][i] += o;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
            for (int i = 0; i < NPK; ++i) {
                acc[k][2 * i] += pk[k][i] & 0xffffu;
                acc[k][2 * i + 1] += pk[k][i] >> 16;
            }
        g = gn;
#pragma unroll
        for (int u = 0; u < AC_UNR; ++u)
            c[u] = cn[u], r[u] = rn[u];
    }
    if (bad && t == 0)
        *status = (uint32_t)ABUB_ACT_E_RANGE;
    if (!mine || n_read == 0)
        return;
#pragma unroll
    for (int k = 0; k < (MODEL ? 6 : 2); ++k) {
        uint32_t *row = planes + (uint64_t)k * plane_stride + at;
        if constexpr (PX == 8) {
            if ((head & 3u) == 0u) { // (planes is 16-byte aligned, plane_stride a multiple of 4: so is this address)
                u32x4 *q = reinterpret_cast<u32x4 *>(row);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    u32x4 v = q[h];
                    const uint32_t a0 = acc[k][4 * h], a1 = acc[k][4 * h + 1], a2 = acc[k][4 * h + 2], a3 = acc[k][4 * h + 3];
                    v.x += k < 2 ? n_read - a0 : a0;
                    v.y += k < 2 ? n_read - a1 : a1;
                    v.z += k < 2 ? n_read - a2 : a2;
                    v.w += k < 2 ? n_read - a3 : a3;
                    q[h] = v;
                }
                continue;
            }
        }
#pragma unroll
        for (int i = 0; i < PX; ++i)
            row[i] += k < 2 ? n_read - acc[k][i] : acc[k][i];
    }
}

template <int PX>
int act_launch(bool model, unsigned blocks, hipStream_t st, const uint8_t *frames, uint64_t frames_bytes, const uint8_t *mu,
               const uint8_t *sigma6, const abub_act_job *jobs, int njobs, uint64_t frame_bytes, uint32_t head, uint64_t body_end,
               uint64_t count, uint32_t *planes, uint64_t plane_stride, uint32_t *status)
{
    if (model)
        k_act<PX, true><<<blocks, AC_THREADS, 0, st>>>(frames, frames_bytes, mu, sigma6, jobs, njobs, frame_bytes, head, body_end, count,
                                                       planes, plane_stride, status);
    else
        k_act<PX, false><<<blocks, AC_THREADS, 0, st>>>(frames, frames_bytes, mu, sigma6, jobs, njobs, frame_bytes, head, body_end, count,
                                                        planes, plane_stride, status);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}

} // namespace

extern "C" int abub_pixel_activity_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, const uint8_t *sigma6,
                                       const abub_act_job *jobs, int njobs, size_t frame_bytes, uint32_t *planes,
                                       size_t plane_stride, uint32_t *status, void *stream)
{
    if (!frames || !jobs || !planes || !status || njobs < 0 || (mu == nullptr) != (sigma6 == nullptr))
        return set_err(ABUB_E_INVALID, "abub_pixel_activity_dev: null pointer, negative count, or one of mu and sigma6 without the other");
    if (!frame_bytes_ok(frame_bytes))
        return set_err(ABUB_E_INVALID, "abub_pixel_activity_dev: frame_bytes must be in [1, 2^32 - 2]");
    if (plane_stride < frame_bytes || (plane_stride & 3) || ((uintptr_t)planes & 15))
        return set_err(ABUB_E_INVALID,
                       "abub_pixel_activity_dev: plane_stride must be a multiple of 4 and >= frame_bytes, planes 16-byte aligned");
    if (((uintptr_t)jobs & 7) || ((uintptr_t)status & 3))
        return set_err(ABUB_E_INVALID, "abub_pixel_activity_dev: jobs must be 8-byte aligned, status 4-byte aligned");
    if (njobs == 0)
        return ABUB_OK;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(status, 0, sizeof(uint32_t), st));
    const uintptr_t anchor = (uintptr_t)(mu ? mu : frames);
    const uint32_t head = (uint32_t)std::min<uint64_t>((8u - (anchor & 7u)) & 7u, frame_bytes);
    const uint64_t nunits = (frame_bytes - head) / AC_PX, body_end = head + nunits * AC_PX, edge = head + (frame_bytes - body_end);
    if (nunits) {
        const int rc = act_launch<AC_PX>(mu != nullptr, (unsigned)((nunits + AC_THREADS - 1) / AC_THREADS), st, frames, frames_bytes, mu,
                                         sigma6, jobs, njobs, frame_bytes, head, body_end, nunits, planes, plane_stride, status);
        if (rc != ABUB_OK)
            return rc;
    }
    if (edge) // (at most 14 single pixels)
        return act_launch<1>(mu != nullptr, 1u, st, frames, frames_bytes, mu, sigma6, jobs, njobs, frame_bytes, head, body_end, edge,
                             planes, plane_stride, status);
    return ABUB_OK;
}

// ---- per-frame shift search: abub_frame_shift_dev ("Surveying a run for movement") ----------------------
// The SAD between a frame p and its model plane m (mu) at every integer displacement within a radius R (host/survey.cpp
// frameShiftHost, the definition): with the interior I = [R, W - R) x [R, H - R),
//   sad[(dy + R) * (2 R + 1) + (dx + R)] = sum over (x, y) in I of |p(x + dx, y + dy) - m(x, y)|,    -R <= dx, dy <= R.
//
// The grid is jobs x tiles of the interior, SH_TW = 256 pixels by SH_TH = 64 rows; a block of four waves owns a tile.  It
// reads the tile of the frame with its halo of R pixels on every side from memory once, into LDS, in rows of dwords (row r,
// dword c: the four pixels from (x0 - R + 4 c, y0 - R + r) on, in memory order).  Lane l owns the four pixels from
// x0 + 4 l on of the tile's rows w, w + 4, ... (w: its wave) and holds their mu dwords in registers for the whole tile.  Per
// dy (a loop that is not unrolled) it has 2 R + 1 u32 sums in registers: of every row it owns it reads the ceil((2 R + 4) / 4)
// dwords of LDS row + dy that lie under its pixels at all dx, forms the byte-shifted dword of each dx with v_alignbyte_b32
// and adds v_sad_u8 of it against mu.  Pixels of a dword beyond the interior's right edge are cleared in both operands; a
// block whose 256 columns all lie inside takes a path without the masks, and there, from R = 2 on, four consecutive dx at a
// time are one v_qsad_pk_u16_u8 of two neighbouring dwords against mu, into four u16 sums that are taken apart once per dy
// (a lane adds at most 16 rows * 4 * 255 = 16320 into a u16: whether the instruction wraps or saturates never shows).  The sums of a dy are added over the wave
// with shuffles and kept in LDS per wave; at the end thread t adds the four waves' values of displacement t and issues one u64
// atomic add into the job's surface (an add of 0 is left out).  A tile has at most 256 * 64 pixels, and 16384 * 255 < 2^32:
// every partial sum of a block fits u32.  Integer adds commute, so a surface does not depend on the order the blocks
// arrive in, and no workgroup waits for another.  k_shift_init writes the status and clears the surface first.
//
// A stream's dword at any byte index is formed from the two aligned dwords around it (one where the address is a multiple
// of 4) where both lie inside the frame, else from single bytes; a byte beyond the frame's end reads as 0 and only ever
// meets a cleared mu byte or a row that is not summed.
//
// Bounds.  A job is read only if cur + W * H <= frames_bytes and model + W * H <= model_bytes; otherwise E_RANGE, found
// alike by k_shift_init and by every block of k_shift.  Within a job every load of sh_load4 lies in [0, W * H) of its
// stream (the test is on the index itself).  LDS: row r < rows + 2 R <= SH_TH + 2 R, dword c < SH_TW / 4 + ND - 1, the
// array's bounds; a lane reads dwords l .. l + ND - 1 of rows it was given.  Stores: status[j] and sad[j * N + t], j < njobs,
// t < N = (2 R + 1)^2.
namespace {

#define SH_TW 256u /* interior pixels of a tile across: one dword per lane */
#define SH_TH 64u  /* rows of a tile: 16 per wave */
#define SH_ROWS (SH_TH / (FR_THREADS / 64))

__device__ __forceinline__ bool sh_job_ok(const abub_shift_job &jb, uint64_t frames_bytes, uint64_t model_bytes, uint64_t P)
{
    return frame_in_range(jb.cur, frames_bytes, P) && frame_in_range(jb.model, model_bytes, P);
}

// the four bytes from index i on of a stream of P bytes, in memory order; bytes at P and beyond read as 0
__device__ __forceinline__ uint32_t sh_load4(const uint8_t *s, uint64_t i, uint64_t P)
{
    const uint32_t mis = (uint32_t)((uintptr_t)(s + i) & 3u);
    if (mis == 0u && i + 4u <= P)
        return *reinterpret_cast<const uint32_t *>(s + i);
    if (i >= mis && i - mis + 8u <= P) {
        const uint32_t *a = reinterpret_cast<const uint32_t *>(s + (i - mis));
        return __builtin_amdgcn_alignbyte(a[1], a[0], mis);
    }
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
        if (i + k < P)
            v |= (uint32_t)s[i + k] << (8u * k);
    return v;
}

__global__ __launch_bounds__(FR_THREADS) void k_shift_init(uint64_t frames_bytes, uint64_t model_bytes,
                                                           const abub_shift_job *__restrict__ jobs, int njobs, uint64_t P, uint32_t N,
                                                           uint32_t *__restrict__ status, uint64_t *__restrict__ sad)
{
    const uint64_t t = (uint64_t)blockIdx.x * FR_THREADS + threadIdx.x;
    if (t >= (uint64_t)njobs * N)
        return;
    sad[t] = 0;
    if (t % N == 0u) {
        const uint64_t j = t / N;
        status[j] = sh_job_ok(jobs[j], frames_bytes, model_bytes, P) ? 0u : (uint32_t)ABUB_SHIFT_E_RANGE;
    }
}

template <int R, bool FULL, bool QSAD = false>
__device__ __forceinline__ void sh_tile(const uint32_t *tile, const uint32_t (&m)[SH_ROWS], uint32_t mask, uint32_t rows,
                                        uint32_t (*part)[(2 * R + 1) * (2 * R + 1)])
{
    constexpr int D = 2 * R + 1, ND = (2 * R + 4 + 3) / 4, RS = SH_TW / 4 + ND - 1;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll 1
    for (int dy = 0; dy < D; ++dy) {
        uint32_t acc[D];
#pragma unroll
        for (int o = 0; o < D; ++o)
            acc[o] = 0;
        // QSAD: the displacements 4 g .. 4 g + 3 of a group g whose upper dword the lane has read, as four u16 sums of one
        // v_qsad_pk_u16_u8 (a lane adds at most SH_ROWS * 4 * 255 = 16320 into each: no carry, no saturation)
        constexpr int NQ = QSAD ? ND - 1 : 0;
        uint64_t qacc[NQ ? NQ : 1] = {};
#pragma unroll
        for (uint32_t r = 0; r < SH_ROWS; ++r) {
            const uint32_t row = r * (FR_THREADS / 64) + wave; // (the same in every lane of the wave)
            if (row >= rows)
                break;
            const uint32_t *src = tile + (row + (uint32_t)dy) * RS + lane;
            uint32_t d[ND];
#pragma unroll
            for (int k = 0; k < ND; ++k)
                d[k] = src[k];
#pragma unroll
            for (int g = 0; g < NQ; ++g)
                qacc[g] = __builtin_amdgcn_qsad_pk_u16_u8((uint64_t)d[g] | (uint64_t)d[g + 1] << 32, m[r], qacc[g]);
#pragma unroll
            for (int o = 4 * NQ; o < D; ++o) {
                uint32_t a = d[o >> 2]; // the four pixels at dx = o - R: bytes o .. o + 3 of what the lane read
                if (o & 3)
                    a = __builtin_amdgcn_alignbyte(d[(o + 3) >> 2], a, (uint32_t)(o & 3));
                if (!FULL)
                    a &= mask;
                acc[o] = __builtin_amdgcn_sad_u8(a, m[r], acc[o]);
            }
        }
#pragma unroll
        for (int o = 0; o < 4 * NQ && o < D; ++o)
            acc[o] = (uint32_t)(qacc[o >> 2] >> (16 * (o & 3))) & 0xffffu;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1)
#pragma unroll
            for (int o = 0; o < D; ++o)
                acc[o] += (uint32_t)__shfl_xor(acc[o], s);
        if (lane == 0u) {
#pragma unroll
            for (int o = 0; o < D; ++o)
                part[wave][dy * D + o] = acc[o];
        }
    }
}

template <int R>
__global__ __launch_bounds__(FR_THREADS) void k_shift(const uint8_t *frames, uint64_t frames_bytes, const uint8_t *mu, uint64_t model_bytes,
                                                      const abub_shift_job *__restrict__ jobs, int njobs, uint32_t W, uint32_t H,
                                                      uint32_t tiles_x, uint64_t *__restrict__ sad)
{
    constexpr int D = 2 * R + 1, N = D * D, ND = (2 * R + 4 + 3) / 4, RS = SH_TW / 4 + ND - 1;
    __shared__ uint32_t tile[(SH_TH + 2 * R) * RS];
    __shared__ uint32_t part[FR_THREADS / 64][N];
    const uint64_t P = (uint64_t)W * H;
    // the tile: interior pixels [x0, x0 + cols) x [y0, y0 + rows), cols and rows at least 1 by the grid's shape
    const uint32_t x0 = (uint32_t)R + (blockIdx.x % tiles_x) * SH_TW, y0 = (uint32_t)R + (blockIdx.x / tiles_x) * SH_TH;
    const uint32_t cols = min(SH_TW, W - (uint32_t)R - x0), rows = min(SH_TH, H - (uint32_t)R - y0);
    const uint32_t ndw = (cols + 2u * R + 3u) / 4u; // dwords of a tile row that hold a pixel some lane uses: <= RS
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // which of the lane's four pixels lie in the interior
    const uint32_t left = 4u * lane < cols ? min(4u, cols - 4u * lane) : 0u;
    const uint32_t mask = left == 4u ? 0xffffffffu : (1u << (8u * left)) - 1u;
    for (uint32_t j = blockIdx.y; j < (uint32_t)njobs; j += gridDim.y) {
        const abub_shift_job jb = jobs[j];
        if (!sh_job_ok(jb, frames_bytes, model_bytes, P))
            continue; // (the same in every thread of every block of the job)
        const uint8_t *p = frames + jb.cur, *q = mu + jb.model;
        for (uint32_t i = threadIdx.x; i < (rows + 2u * R) * RS; i += FR_THREADS) {
            const uint32_t r = i / RS, c = i % RS;
            tile[i] = c < ndw ? sh_load4(p, (uint64_t)(y0 - R + r) * W + (x0 - R) + 4u * c, P) : 0u;
        }
        uint32_t m[SH_ROWS];
#pragma unroll
        for (uint32_t r = 0; r < SH_ROWS; ++r) {
            const uint32_t row = r * (FR_THREADS / 64) + wave;
            m[r] = row < rows && left ? sh_load4(q, (uint64_t)(y0 + row) * W + x0 + 4u * lane, P) & mask : 0u;
        }
        __syncthreads();
        if (cols == SH_TW)
            sh_tile<R, true, R >= 2>(tile, m, mask, rows, part); // (the quad form measured 2 to 3 % faster from R = 2 on, 1 % slower at 1)
        else
            sh_tile<R, false>(tile, m, mask, rows, part);
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < (uint32_t)N; t += FR_THREADS) {
            uint32_t v = part[0][t];
#pragma unroll
            for (int w = 1; w < FR_THREADS / 64; ++w)
                v += part[w][t];
            if (v)
                atomicAdd((unsigned long long *)(sad + (uint64_t)j * N + t), (unsigned long long)v);
        }
        __syncthreads(); // (tile and part are written again for the block's next job)
    }
}

template <int R>
void shift_launch(dim3 grid, hipStream_t st, const uint8_t *frames, uint64_t frames_bytes, const uint8_t *mu, uint64_t model_bytes,
                  const abub_shift_job *jobs, int njobs, uint32_t W, uint32_t H, uint32_t tiles_x, uint64_t *sad)
{
    k_shift<R><<<grid, FR_THREADS, 0, st>>>(frames, frames_bytes, mu, model_bytes, jobs, njobs, W, H, tiles_x, sad);
}

} // namespace

extern "C" int abub_frame_shift_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, size_t model_bytes,
                                    const abub_shift_job *jobs, int njobs, int W, int H, int R, uint32_t *status, uint64_t *sad,
                                    void *stream)
{
    if (!frames || !mu || !jobs || !status || !sad || njobs < 0)
        return set_err(ABUB_E_INVALID, "abub_frame_shift_dev: null pointer or negative count");
    if (R < 1 || R > 8)
        return set_err(ABUB_E_INVALID, "abub_frame_shift_dev: R must be in [1, 8]");
    if (W < 2 * R + 1 || W > 65535 || H < 2 * R + 1 || H > 65535)
        return set_err(ABUB_E_INVALID, "abub_frame_shift_dev: W and H must be in [2 R + 1, 65535]");
    if (!frame_lists_aligned(jobs, sad) || ((uintptr_t)status & 3))
        return set_err(ABUB_E_INVALID, "abub_frame_shift_dev: jobs and sad must be 8-byte aligned, status 4-byte aligned");
    if (njobs == 0)
        return ABUB_OK;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t P = (uint64_t)W * (uint64_t)H;
    const uint32_t N = (uint32_t)((2 * R + 1) * (2 * R + 1));
    k_shift_init<<<(unsigned)(((uint64_t)njobs * N + FR_THREADS - 1) / FR_THREADS), FR_THREADS, 0, st>>>(
        (uint64_t)frames_bytes, (uint64_t)model_bytes, jobs, njobs, P, N, status, sad);
    HIPCHK(hipGetLastError());
    const uint32_t tiles_x = ((uint32_t)(W - 2 * R) + SH_TW - 1) / SH_TW, tiles_y = ((uint32_t)(H - 2 * R) + SH_TH - 1) / SH_TH;
    const dim3 grid(tiles_x * tiles_y, (unsigned)(njobs < 65535 ? njobs : 65535)); // (at most 256 * 1024 tiles)
    typedef void (*Launch)(dim3, hipStream_t, const uint8_t *, uint64_t, const uint8_t *, uint64_t, const abub_shift_job *, int, uint32_t,
                           uint32_t, uint32_t, uint64_t *);
    static const Launch launch[8] = {shift_launch<1>, shift_launch<2>, shift_launch<3>, shift_launch<4>,
                                     shift_launch<5>, shift_launch<6>, shift_launch<7>, shift_launch<8>};
    launch[R - 1](grid, st, frames, (uint64_t)frames_bytes, mu, (uint64_t)model_bytes, jobs, njobs, (uint32_t)W, (uint32_t)H, tiles_x, sad);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}

// ---- per-cell products: what the field, light, focus and noise kernels share ----------------------------------------------
// Each gives WORDS words per job and cell of FC_CELL x FC_CELL pixels, on a grid of ncx x ncy whole cells from (x0, y0)
// that lies inside the frame with a ring of `ring` pixels around it: rec[((j ncy + cy) ncx + cx) WORDS + t].
//
// The grid is cells x jobs; a block of four waves owns one cell of one job at a time and with it the cell's WORDS words: it
// writes each of them once with a plain store, so there is no atomic, no clearing launch and no other launch (the block of
// cell 0 writes the job's status word).  A cell is 32 dwords wide, so the 64 lanes of a wave span two cell rows: lane l
// owns dword col = l & 31 of the cell rows 8 k + first, first = 2 w + (l >> 5), k < FC_ROWS = 16 (w: its wave); in a stream
// that is the dword at byte Cell::at(k).  A kernel is
//     c = cells_here(..); for (j = blockIdx.y; j < njobs; j += gridDim.y) {
//         ok = its range test; out = cells_open(j, ok, ..); if (!ok) { cells_zero(out); continue; }
//         its sums; cells_close(c, sums, part, out); }
// cells_close adds a lane's sums over its wave with shuffles, over the four waves through `part`, and stores the record.
// The loop and the branch stay in the kernel, which keeps the code of the four what it was when each had a copy of all this
// (profiles/r28): behind a functor of a shared loop a product's arithmetic is compiled on its own before the loop around it
// is seen, and k_noise_cells went from 112 to 129 VGPRs, from 4 waves per SIMD to 3; with the branch inside cells_open
// k_light_cells ran 2.5 % and k_focus_cells 1.4 % slower.
//
// A refused job.  A job is read only if the product's range test holds (sh_job_ok, nc_job_ok); otherwise its status is
// E_RANGE and its record zero.  The test depends on the job and the launch alone, so it comes out the same in every thread
// of every block of the job: a block leaves the job as one, before the job's first barrier.
//
// Bounds.  Stores: status[j] and rec[(j * cells + cell) * WORDS + t] with j < njobs, cell < cells = gridDim.x and t < WORDS,
// inside the njobs and njobs * cells * WORDS words the caller gives.  LDS: part[wave][t], wave < 4, t < WORDS; the barrier
// that ends cells_close stands between a job's last read of `part` and of the product's tiles and the next job's first
// write.  cells_check admits only grids with ring <= x0, x0 + 128 ncx + ring <= W and so in y: a cell's pixels and the ring
// around them lie inside the W * H bytes of a frame or model plane, which the range test has placed inside its buffer.
namespace {

#define FC_CELL ((uint32_t)ABUB_FIELD_CELL)
#define FC_ROWS (FC_CELL / (2u * (FR_THREADS / 64))) /* rows of a cell per lane: 16 */
static_assert(FC_CELL == 128u && FC_ROWS == SH_ROWS, "a wave spans two rows of 32 dwords; the u16 bound is that of sh_tile");

struct Cell {
    uint64_t P;                      // bytes of a frame or model plane
    uint32_t W, xc, yc;              // the cell's first pixel
    uint32_t lane, wave, first, col; // the lane's rows and dword (above)
    __device__ __forceinline__ uint64_t at(uint32_t k) const { return (uint64_t)(yc + k * 8u + first) * W + xc + 4u * col; }
};
__device__ __forceinline__ Cell cells_here(uint32_t W, uint32_t H, uint32_t ncx, uint32_t x0, uint32_t y0)
{
    const uint32_t cell = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    return {(uint64_t)W * H, W, x0 + (cell % ncx) * FC_CELL, y0 + (cell / ncx) * FC_CELL, lane, wave, 2u * wave + (lane >> 5), lane & 31u};
}

// A job begins: its status word.  -> the block's record
template <uint32_t WORDS, class T>
__device__ __forceinline__ T *cells_open(uint32_t j, bool good, uint32_t *status, T *rec)
{
    T *out = rec + ((uint64_t)j * gridDim.x + blockIdx.x) * WORDS;
    if (blockIdx.x == 0u && threadIdx.x == 0u)
        status[j] = good ? 0u : (uint32_t)ABUB_SHIFT_E_RANGE;
    return out;
}
// the record of a refused job
template <uint32_t WORDS, class T>
__device__ __forceinline__ void cells_zero(T *out)
{
    for (uint32_t t = threadIdx.x; t < WORDS; t += FR_THREADS)
        out[t] = 0;
}
// A job ends: word t of its record is the sum of part[wave][t] over the waves
template <uint32_t WORDS, class T>
__device__ __forceinline__ void cells_close(const T (*part)[WORDS], T *out)
{
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < WORDS; t += FR_THREADS) {
        T v = part[0][t];
#pragma unroll
        for (int w = 1; w < FR_THREADS / 64; ++w)
            v += part[w][t];
        out[t] = v;
    }
    __syncthreads();
}
// the same from the lanes' sums
template <uint32_t WORDS, class T>
__device__ __forceinline__ void cells_close(const Cell &c, T (&acc)[WORDS], T (*part)[WORDS], T *out)
{
    wave_reduce_all<WaveSum>(acc);
    if (c.lane == 0u) {
#pragma unroll
        for (uint32_t o = 0; o < WORDS; ++o)
            part[c.wave][o] = acc[o];
    }
    cells_close(part, out);
}

// The entries' side.  CELLS_LAUNCH, or what the entry returns: its error, or ABUB_OK for an empty job list
#define CELLS_LAUNCH 1
int cells_check(const char *entry, bool pointers, const void *jobs, const void *status, const void *rec, int njobs, int W, int H, int x0,
                int y0, int ncx, int ncy, int ring)
{
    const int C = ABUB_FIELD_CELL;
    char msg[192];
    if (!pointers || njobs < 0)
        snprintf(msg, sizeof msg, "%s: null pointer or negative count", entry);
    else if (W < C + 2 * ring || W > 65535 || H < C + 2 * ring || H > 65535)
        snprintf(msg, sizeof msg, "%s: W and H must be in [%d, 65535]", entry, C + 2 * ring);
    // (ncx, ncy <= 511 once the sides are bounded, so the sums below cannot overflow an int)
    else if (ncx < 1 || ncy < 1 || ncx > (W - 2 * ring) / C || ncy > (H - 2 * ring) / C || x0 < ring || y0 < ring ||
             x0 > W - ring - C * ncx || y0 > H - ring - C * ncy)
        snprintf(msg, sizeof msg, "%s: the grid of whole cells and a ring of %d pixels around it must lie inside the frame", entry, ring);
    else if (((uintptr_t)jobs & 7) || (((uintptr_t)status | (uintptr_t)rec) & 3))
        snprintf(msg, sizeof msg, "%s: jobs must be 8-byte aligned, status and the records 4-byte aligned", entry);
    else
        return njobs == 0 ? ABUB_OK : CELLS_LAUNCH;
    return set_err(ABUB_E_INVALID, msg);
}
inline dim3 cells_grid(int ncx, int ncy, int njobs) { return dim3((unsigned)(ncx * ncy), (unsigned)(njobs < 65535 ? njobs : 65535)); } // (at most 511 * 511 cells)

} // namespace

// ---- per-cell shift field: abub_frame_shift_cells_dev ("Surveying a run for local movement") ------------
// The same sums as above, kept apart per cell of FC_CELL x FC_CELL interior pixels (host/survey.cpp fieldCellsHost, the
// definition): with (ncx, ncy, x0, y0) = abub_frame_cells_grid(W, H, R), for cell (cx, cy)
//   sad[((j ncy + cy) ncx + cx) (2 R + 1)^2 + (dy + R) (2 R + 1) + (dx + R)] = sum of |p(x + dx, y + dy) - m(x, y)|
// over x0 + 128 cx <= x < x0 + 128 (cx + 1), y0 + 128 cy <= y < y0 + 128 (cy + 1).  Only whole cells exist.
//
// A block reads the cell with its halo of R pixels on every side once into LDS, 128 + 2 R rows of RS = 32 + ND - 1 dwords
// (row r, dword c: the four pixels from (xc - R + 4 c, yc - R + r) on), and a lane holds the mu dwords of its rows in
// registers.  The two halves of a wave are the two lane groups of a ds_read_b32 / ds_read2_b32 (banks mod 32), and within a
// half the lanes read 32 consecutive dwords of one row: no bank conflict at any RS.  The arithmetic is sh_tile's full-tile
// path: per dy 2 R + 1 sums in registers, from R = 2 on four dx at a time with v_qsad_pk_u16_u8 (a lane adds at most
// 16 rows * 4 * 255 = 16320 into a u16), the rest with v_alignbyte_b32 and v_sad_u8.  fc_cell adds the lanes of a wave
// itself, a dy at a time, and leaves the (2 R + 1)^2 sums in `part`: the field closes a job with cells_close(part, out).  A surface
// entry sums 16384 pixels: at most 16384 * 255 < 2^32.
//
// Bounds.  The ring is the halo, R.  The last dword of a tile row ends at byte 4 RS >= 128 + 2 R of it, at most 3 bytes
// behind the halo: sh_load4 tests the index itself against W * H, a byte beyond reads as 0, and no lane uses a byte behind
// the halo (its last is 4 * 31 + 2 R + 3).  LDS: row < 128 + 2 R, dword < RS.
namespace {

template <int R>
__device__ __forceinline__ void fc_cell(const uint32_t *tile, const uint32_t (&m)[FC_ROWS], uint32_t (*part)[(2 * R + 1) * (2 * R + 1)])
{
    constexpr int D = 2 * R + 1, ND = (2 * R + 4 + 3) / 4, RS = FC_CELL / 4 + ND - 1;
    constexpr int NQ = R >= 2 ? ND - 1 : 0; // (as k_shift chose: the quad form from R = 2 on)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t first = 2u * wave + (lane >> 5), col = lane & 31u;
#pragma unroll 1
    for (int dy = 0; dy < D; ++dy) {
        uint32_t acc[D];
#pragma unroll
        for (int o = 0; o < D; ++o)
            acc[o] = 0;
        uint64_t qacc[NQ ? NQ : 1] = {};
#pragma unroll
        for (uint32_t r = 0; r < FC_ROWS; ++r) {
            const uint32_t *src = tile + (r * 8u + first + (uint32_t)dy) * RS + col;
            uint32_t d[ND];
#pragma unroll
            for (int k = 0; k < ND; ++k)
                d[k] = src[k];
#pragma unroll
            for (int g = 0; g < NQ; ++g)
                qacc[g] = __builtin_amdgcn_qsad_pk_u16_u8((uint64_t)d[g] | (uint64_t)d[g + 1] << 32, m[r], qacc[g]);
#pragma unroll
            for (int o = 4 * NQ; o < D; ++o) {
                uint32_t a = d[o >> 2]; // the four pixels at dx = o - R: bytes o .. o + 3 of what the lane read
                if (o & 3)
                    a = __builtin_amdgcn_alignbyte(d[(o + 3) >> 2], a, (uint32_t)(o & 3));
                acc[o] = __builtin_amdgcn_sad_u8(a, m[r], acc[o]);
            }
        }
#pragma unroll
        for (int o = 0; o < 4 * NQ && o < D; ++o)
            acc[o] = (uint32_t)(qacc[o >> 2] >> (16 * (o & 3))) & 0xffffu;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1)
#pragma unroll
            for (int o = 0; o < D; ++o)
                acc[o] += (uint32_t)__shfl_xor(acc[o], s);
        if (lane == 0u) {
#pragma unroll
            for (int o = 0; o < D; ++o)
                part[wave][dy * D + o] = acc[o];
        }
    }
}

template <int R>
__global__ __launch_bounds__(FR_THREADS) void k_shift_cells(const uint8_t *frames, uint64_t frames_bytes, const uint8_t *mu,
                                                            uint64_t model_bytes, const abub_shift_job *__restrict__ jobs, int njobs,
                                                            uint32_t W, uint32_t H, uint32_t ncx, uint32_t x0, uint32_t y0,
                                                            uint32_t *__restrict__ status, uint32_t *__restrict__ sad)
{
    constexpr int D = 2 * R + 1, N = D * D, ND = (2 * R + 4 + 3) / 4, RS = FC_CELL / 4 + ND - 1, TR = FC_CELL + 2 * R;
    __shared__ uint32_t tile[TR * RS];
    __shared__ uint32_t part[FR_THREADS / 64][(uint32_t)N];
    const Cell c = cells_here(W, H, ncx, x0, y0);
    for (uint32_t j = blockIdx.y; j < (uint32_t)njobs; j += gridDim.y) {
        const abub_shift_job jb = jobs[j];
        const bool ok = sh_job_ok(jb, frames_bytes, model_bytes, c.P);
        uint32_t *out = cells_open<(uint32_t)N>(j, ok, status, sad);
        if (!ok) {
            cells_zero<(uint32_t)N>(out);
            continue;
        }
        const uint8_t *p = frames + jb.cur, *q = mu + jb.model;
        for (uint32_t i = threadIdx.x; i < (uint32_t)(TR * RS); i += FR_THREADS) {
            const uint32_t r = i / (uint32_t)RS, d = i % (uint32_t)RS;
            tile[i] = sh_load4(p, (uint64_t)(c.yc - R + r) * W + (c.xc - R) + 4u * d, c.P);
        }
        uint32_t m[FC_ROWS];
#pragma unroll
        for (uint32_t r = 0; r < FC_ROWS; ++r)
            m[r] = sh_load4(q, c.at(r), c.P);
        __syncthreads();
        fc_cell<R>(tile, m, part);
        cells_close(part, out);
    }
}

template <int R>
void cells_launch(dim3 grid, hipStream_t st, const uint8_t *frames, uint64_t frames_bytes, const uint8_t *mu, uint64_t model_bytes,
                  const abub_shift_job *jobs, int njobs, uint32_t W, uint32_t H, uint32_t ncx, uint32_t x0, uint32_t y0, uint32_t *status,
                  uint32_t *sad)
{
    k_shift_cells<R><<<grid, FR_THREADS, 0, st>>>(frames, frames_bytes, mu, model_bytes, jobs, njobs, W, H, ncx, x0, y0, status, sad);
}

} // namespace

extern "C" int abub_frame_cells_grid(int W, int H, int R, int *ncx, int *ncy, int *x0, int *y0)
{
    if (!ncx || !ncy || !x0 || !y0)
        return set_err(ABUB_E_INVALID, "abub_frame_cells_grid: null pointer");
    if (R < 1 || R > 8 || W < 0 || H < 0)
        return set_err(ABUB_E_INVALID, "abub_frame_cells_grid: R must be in [1, 8], W and H not negative");
    const int C = ABUB_FIELD_CELL, iw = std::max(W - 2 * R, 0), ih = std::max(H - 2 * R, 0);
    *ncx = iw / C;
    *ncy = ih / C;
    *x0 = R + (iw - C * *ncx) / 2;
    *y0 = R + (ih - C * *ncy) / 2;
    return ABUB_OK;
}

extern "C" int abub_frame_shift_cells_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, size_t model_bytes,
                                          const abub_shift_job *jobs, int njobs, int W, int H, int R, uint32_t *status, uint32_t *sad,
                                          void *stream)
{
    if (R < 1 || R > 8)
        return set_err(ABUB_E_INVALID, "abub_frame_shift_cells_dev: R must be in [1, 8]");
    int ncx = 0, ncy = 0, x0 = 0, y0 = 0;
    abub_frame_cells_grid(W, H, R, &ncx, &ncy, &x0, &y0); // (a side it refuses or that has no whole cell is below 128 + 2 R)
    const int chk = cells_check("abub_frame_shift_cells_dev", frames && mu && jobs && status && sad, jobs, status, sad, njobs, W, H, x0,
                                y0, ncx, ncy, R);
    if (chk != CELLS_LAUNCH)
        return chk;
    const dim3 grid = cells_grid(ncx, ncy, njobs);
    typedef void (*Launch)(dim3, hipStream_t, const uint8_t *, uint64_t, const uint8_t *, uint64_t, const abub_shift_job *, int, uint32_t,
                           uint32_t, uint32_t, uint32_t, uint32_t, uint32_t *, uint32_t *);
    static const Launch launch[8] = {cells_launch<1>, cells_launch<2>, cells_launch<3>, cells_launch<4>,
                                     cells_launch<5>, cells_launch<6>, cells_launch<7>, cells_launch<8>};
    launch[R - 1](grid, (hipStream_t)stream, frames, (uint64_t)frames_bytes, mu, (uint64_t)model_bytes, jobs, njobs, (uint32_t)W,
                  (uint32_t)H, (uint32_t)ncx, (uint32_t)x0, (uint32_t)y0, status, sad);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}

// ---- per-cell light record: abub_frame_light_cells_dev ("Surveying a run for lighting changes") ----------
// Per cell of FC_CELL x FC_CELL pixels on a grid the caller gives (x0, y0, ncx, ncy: abub_frame_cells_grid's, or any other
// that lies inside the frame) six u32 sums over the cell's pixels p of the frame and m of mu (host/survey.cpp
// lightCellsHost, the definition):
//   rec[((j ncy + cy) ncx + cx) 6 + 0 .. 5] = sum p, sum p^2, sum p m, sum |p - m|, the pixels with p == 0, with p == 255.
//
// There is no halo and so no LDS tile: p and m come straight into registers through sh_load4.  Per dword: sum p is
// v_sad_u8 against 0, sum |p - m| v_sad_u8(p, m), sum p^2 and sum p m v_dot4_u32_u8; the two counts are the set top bits of
// ((x & 0x7f7f7f7f) + 0x7f7f7f7f | x | 0x7f7f7f7f) inverted, x = p and ~p: 0x7f + 0x7f = 0xfe never carries into the next
// byte, so the test is exact per byte.  A lane sums 64 pixels (at most 64 * 65025 < 2^32), a cell 16384 (at most
// 16384 * 65025 = 1065369600 < 2^31).
//
// Bounds.  No ring: every dword a lane loads lies wholly inside the W * H bytes of its stream; sh_load4 tests the index
// against W * H besides.
namespace {

#define LC_WORDS 6u

// 0x80 in every byte of x that is 0, 0 in the others (no carry crosses a byte)
__device__ __forceinline__ uint32_t lc_zero_bytes(uint32_t x)
{
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

__global__ __launch_bounds__(FR_THREADS) void k_light_cells(const uint8_t *frames, uint64_t frames_bytes, const uint8_t *mu,
                                                            uint64_t model_bytes, const abub_shift_job *__restrict__ jobs, int njobs,
                                                            uint32_t W, uint32_t H, uint32_t ncx, uint32_t x0, uint32_t y0,
                                                            uint32_t *__restrict__ status, uint32_t *__restrict__ rec)
{
    __shared__ uint32_t part[FR_THREADS / 64][LC_WORDS];
    const Cell c = cells_here(W, H, ncx, x0, y0);
    for (uint32_t j = blockIdx.y; j < (uint32_t)njobs; j += gridDim.y) {
        const abub_shift_job jb = jobs[j];
        const bool ok = sh_job_ok(jb, frames_bytes, model_bytes, c.P);
        uint32_t *out = cells_open<LC_WORDS>(j, ok, status, rec);
        if (!ok) {
            cells_zero<LC_WORDS>(out);
            continue;
        }
        const uint8_t *p = frames + jb.cur, *q = mu + jb.model;
        uint32_t acc[LC_WORDS] = {};
#pragma unroll
        for (uint32_t r = 0; r < FC_ROWS; ++r) {
            const uint64_t i = c.at(r);
            const uint32_t a = sh_load4(p, i, c.P), b = sh_load4(q, i, c.P);
            acc[0] = __builtin_amdgcn_sad_u8(a, 0u, acc[0]);
            acc[1] = __builtin_amdgcn_udot4(a, a, acc[1], false);
            acc[2] = __builtin_amdgcn_udot4(a, b, acc[2], false);
            acc[3] = __builtin_amdgcn_sad_u8(a, b, acc[3]);
            acc[4] += (uint32_t)__builtin_popcount(lc_zero_bytes(a));
            acc[5] += (uint32_t)__builtin_popcount(lc_zero_bytes(~a));
        }
        cells_close(c, acc, part, out);
    }
}

} // namespace

extern "C" int abub_frame_light_cells_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, size_t model_bytes,
                                          const abub_shift_job *jobs, int njobs, int W, int H, int x0, int y0, int ncx, int ncy,
                                          uint32_t *status, uint32_t *rec, void *stream)
{
    const int chk = cells_check("abub_frame_light_cells_dev", frames && mu && jobs && status && rec, jobs, status, rec, njobs, W, H, x0,
                                y0, ncx, ncy, 0);
    if (chk != CELLS_LAUNCH)
        return chk;
    k_light_cells<<<cells_grid(ncx, ncy, njobs), FR_THREADS, 0, (hipStream_t)stream>>>(
        frames, (uint64_t)frames_bytes, mu, (uint64_t)model_bytes, jobs, njobs, (uint32_t)W, (uint32_t)H, (uint32_t)ncx, (uint32_t)x0,
        (uint32_t)y0, status, rec);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}

// ---- per-cell edge agreement: abub_frame_focus_cells_dev ("Surveying a run for lost focus") -------------
// Per cell of FC_CELL x FC_CELL pixels on a grid the caller gives (x0, y0, ncx, ncy: abub_frame_cells_grid's, or any other
// that lies inside the frame with a ring of one pixel around it) five i32 over the cell's pixels, with the central
// differences gx = p(x + 1, y) - p(x - 1, y), gy = p(x, y + 1) - p(x, y - 1) of the frame and hx, hy of mu (host/survey.cpp
// focusCellsHost, the definition):
//   rec[((j ncy + cy) ncx + cx) 5 + 0 .. 4] = sum gx^2, sum gy^2, sum gx hx, sum gy hy, the pixels with p == 0 or p == 255.
//
// A block reads the cell with its ring once into two LDS tiles, one of the frame and one of mu, each FO_TR = 130 rows of
// FO_RS = 33 dwords (row r, dword c: the four pixels from (xc - 1 + 4 c, yc - 1 + r) on): 2 * 130 * 33 * 4 = 34320 bytes.
// The two halves of a wave are the two lane groups of a ds_read_b32 / ds_read2_b32 and within a half the lanes read 32
// consecutive dwords of one tile row, so there is no bank conflict.  Of a cell row y the lane reads dwords
// col and col + 1 of the tile rows y, y + 1, y + 2 of both tiles.  With d0, d1 those of tile row y + 1, its four pixels are
// bytes 1 .. 4 of the pair: their left neighbours are d0, their right neighbours v_alignbyte_b32(d1, d0, 2), the pixels
// themselves v_alignbyte_b32(d1, d0, 1); the pixels above and below are the same alignment by one byte of the tile rows y and
// y + 2.  No byte is unpacked: with l, r the neighbours in the frame and L, R those in mu (packed, four to a dword)
//   sum (r - l)^2 = r.r + l.l - 2 r.l,   sum (r - l)(R - L) = r.R + l.L - r.L - l.R,
// each product one v_dot4_u32_u8: seven per direction and dword.  The clipped pixels are the set top bits of
// lc_zero_bytes(p) | lc_zero_bytes(~p).  A lane sums 64 pixels, so each of its eight u32 sums holds at most
// 2 * 64 * 65025 < 2^24; the differences are formed per lane in i32, where the squares' are never negative and a product's
// magnitude is at most 64 * 65025.  A cell's magnitude is at most 16384 * 65025 = 1065369600 < 2^31, and so is that of
// every partial sum.
//
// Bounds.  The ring is 1, so the tile's 130 rows yc - 1 .. yc + 128 lie inside the frame and so do the 130 pixels
// xc - 1 .. xc + 128 of each; a tile row's last dword
// ends at byte 132 of it, two behind the ring: sh_load4 tests the index itself against W * H, a byte beyond reads as 0, and
// no lane uses a byte behind the ring (its last is byte 4 * 31 + 5 = 129).  A block whose tile lies far enough inside the
// stream, its first byte index lo >= 3 and the index of its last dword's first byte lo + 129 W + 128 <= W * H - 8, fills it
// through fo_fill_inside instead: every load is one of the two aligned dwords around a tile dword's first byte, at stream
// bytes >= lo - 3 >= 0 and < lo + 129 W + 128 + 8 <= W * H, so inside the job's frame or model plane, which sh_job_ok has
// placed inside its buffer.  Every other block (the first and the last rows of cells of a frame with no margin) keeps sh_load4.  LDS: tile row first + 8 k + 2 <= 129 < FO_TR,
// dword col + 1 <= 32 < FO_RS.
namespace {

#define FO_WORDS 5u
#define FO_RS (FC_CELL / 4u + 1u) /* dwords of a tile row: 128 + 2 pixels */
#define FO_TR (FC_CELL + 2u)      /* rows of a tile */

// the seven products of one direction: a, b the neighbours behind and ahead in the frame, A, B those in mu
__device__ __forceinline__ void fo_dir(uint32_t a, uint32_t b, uint32_t A, uint32_t B, uint32_t &sq, uint32_t &cross, uint32_t &pos,
                                       uint32_t &neg)
{
    sq = __builtin_amdgcn_udot4(b, b, sq, false);
    sq = __builtin_amdgcn_udot4(a, a, sq, false);
    cross = __builtin_amdgcn_udot4(b, a, cross, false);
    pos = __builtin_amdgcn_udot4(b, B, pos, false);
    pos = __builtin_amdgcn_udot4(a, A, pos, false);
    neg = __builtin_amdgcn_udot4(b, A, neg, false);
    neg = __builtin_amdgcn_udot4(a, B, neg, false);
}

// A tile filled without a test per load, for a tile whose every byte index i in the stream has 3 <= i and i + 8 <= P: the
// two aligned dwords around s + i then lie in [i - 3, i + 8) of the stream whatever its address, and the four bytes from i on
// are v_alignbyte_b32 of them.  A lane issues its loads six at a time before it uses the first (the loop with sh_load4's
// tests waits for every load in turn)
__device__ __forceinline__ void fo_fill_inside(uint32_t *tile, const uint8_t *s, uint64_t lo, uint32_t W)
{
    constexpr uint32_t STEPS = (FO_TR * FO_RS + FR_THREADS - 1u) / FR_THREADS, BATCH = 6u; // (17 loads in batches of 6: registers)
#pragma unroll
    for (uint32_t k0 = 0; k0 < STEPS; k0 += BATCH) {
        uint32_t d0[BATCH], d1[BATCH], mis[BATCH];
#pragma unroll
        for (uint32_t k = 0; k < BATCH; ++k) {
            // (the last step's spare lanes load the last dword again)
            const uint32_t i = min((k0 + k) * FR_THREADS + threadIdx.x, FO_TR * FO_RS - 1u);
            const uintptr_t a = (uintptr_t)(s + lo + (uint64_t)(i / FO_RS) * W + 4u * (i % FO_RS));
            const uint32_t *d = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
            mis[k] = (uint32_t)(a & 3u);
            d0[k] = d[0];
            d1[k] = d[1];
        }
#pragma unroll
        for (uint32_t k = 0; k < BATCH; ++k) {
            const uint32_t i = (k0 + k) * FR_THREADS + threadIdx.x;
            if (i < FO_TR * FO_RS)
                tile[i] = __builtin_amdgcn_alignbyte(d1[k], d0[k], mis[k]);
        }
        __builtin_amdgcn_sched_barrier(0); // (the next batch's loads stay behind this batch's stores)
    }
}

__global__ __launch_bounds__(FR_THREADS, 4) void k_focus_cells(const uint8_t *frames, uint64_t frames_bytes, const uint8_t *mu,
                                                            uint64_t model_bytes, const abub_shift_job *__restrict__ jobs, int njobs,
                                                            uint32_t W, uint32_t H, uint32_t ncx, uint32_t x0, uint32_t y0,
                                                            uint32_t *__restrict__ status, int32_t *__restrict__ rec)
{
    __shared__ uint32_t tp[FO_TR * FO_RS], tm[FO_TR * FO_RS];
    __shared__ int32_t part[FR_THREADS / 64][FO_WORDS];
    const Cell c = cells_here(W, H, ncx, x0, y0);
    // the tile's bytes are those at lo + r W + 0 .. 131 of a stream, r < 130: inside iff every one of them has the two aligned
    // dwords around it within the stream wherever the stream begins (the same in every thread of the block, for every job)
    const uint64_t lo = (uint64_t)(c.yc - 1u) * W + (c.xc - 1u);
    const bool inside = lo >= 3u && lo + (uint64_t)(FO_TR - 1u) * W + 4u * FO_RS + 4u <= c.P;
    for (uint32_t j = blockIdx.y; j < (uint32_t)njobs; j += gridDim.y) {
        const abub_shift_job jb = jobs[j];
        const bool ok = sh_job_ok(jb, frames_bytes, model_bytes, c.P);
        int32_t *out = cells_open<FO_WORDS>(j, ok, status, rec);
        if (!ok) {
            cells_zero<FO_WORDS>(out);
            continue;
        }
        const uint8_t *p = frames + jb.cur, *q = mu + jb.model;
        if (inside) {
            fo_fill_inside(tp, p, lo, W);
            fo_fill_inside(tm, q, lo, W);
        } else {
            for (uint32_t i = threadIdx.x; i < FO_TR * FO_RS; i += FR_THREADS) {
                const uint64_t at = lo + (uint64_t)(i / FO_RS) * W + 4u * (i % FO_RS);
                tp[i] = sh_load4(p, at, c.P);
                tm[i] = sh_load4(q, at, c.P);
            }
        }
        __syncthreads();
        uint32_t xs = 0, xc2 = 0, xp = 0, xn = 0, ys = 0, yc2 = 0, yp = 0, yn = 0, clip = 0;
#pragma unroll
        for (uint32_t r = 0; r < FC_ROWS; ++r) {
            const uint32_t at = (r * 8u + c.first) * FO_RS + c.col; // tile row y: the pixels above cell row y
            const uint32_t pu = __builtin_amdgcn_alignbyte(tp[at + 1u], tp[at], 1u), mu_ = __builtin_amdgcn_alignbyte(tm[at + 1u], tm[at], 1u);
            const uint32_t p0 = tp[at + FO_RS], p1 = tp[at + FO_RS + 1u], m0 = tm[at + FO_RS], m1 = tm[at + FO_RS + 1u];
            const uint32_t pd = __builtin_amdgcn_alignbyte(tp[at + 2u * FO_RS + 1u], tp[at + 2u * FO_RS], 1u);
            const uint32_t md = __builtin_amdgcn_alignbyte(tm[at + 2u * FO_RS + 1u], tm[at + 2u * FO_RS], 1u);
            fo_dir(p0, __builtin_amdgcn_alignbyte(p1, p0, 2u), m0, __builtin_amdgcn_alignbyte(m1, m0, 2u), xs, xc2, xp, xn);
            fo_dir(pu, pd, mu_, md, ys, yc2, yp, yn);
            const uint32_t x = __builtin_amdgcn_alignbyte(p1, p0, 1u);
            clip += (uint32_t)__builtin_popcount(lc_zero_bytes(x) | lc_zero_bytes(~x));
        }
        int32_t acc[FO_WORDS] = {(int32_t)(xs - 2u * xc2), (int32_t)(ys - 2u * yc2), (int32_t)xp - (int32_t)xn, (int32_t)yp - (int32_t)yn,
                                 (int32_t)clip};
        cells_close(c, acc, part, out);
    }
}

} // namespace

extern "C" int abub_frame_focus_cells_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, size_t model_bytes,
                                          const abub_shift_job *jobs, int njobs, int W, int H, int x0, int y0, int ncx, int ncy,
                                          uint32_t *status, int32_t *rec, void *stream)
{
    const int chk = cells_check("abub_frame_focus_cells_dev", frames && mu && jobs && status && rec, jobs, status, rec, njobs, W, H, x0,
                                y0, ncx, ncy, 1);
    if (chk != CELLS_LAUNCH)
        return chk;
    k_focus_cells<<<cells_grid(ncx, ncy, njobs), FR_THREADS, 0, (hipStream_t)stream>>>(
        frames, (uint64_t)frames_bytes, mu, (uint64_t)model_bytes, jobs, njobs, (uint32_t)W, (uint32_t)H, (uint32_t)ncx, (uint32_t)x0,
        (uint32_t)y0, status, rec);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}

// ---- per-cell frame-pair noise record: abub_frame_noise_cells_dev ("Surveying a run for noise changes") --
// Per cell of FC_CELL x FC_CELL pixels on a grid the caller gives (x0, y0, ncx, ncy: abub_frame_cells_grid's, or any other
// that lies inside the frame) six i32 over the cell's pixels p of the frame, r of its reference frame and s of sigma6, with
// d = p - r (host/survey.cpp noiseCellsHost, the definition):
//   rec[((j ncy + cy) ncx + cx) 6 + 0 .. 5] = the pixels with |d| > s, the pixels where p or r is 0 or 255, sum d and sum d^2
//   over the pixels with |d| <= s (the inside ones), sum |d| and sum d^2 over all.
//
// No LDS tile: p, r and s come straight into registers through sh_load4.  Per dword: sum |d| is v_sad_u8(p, r);
// sum d^2 = p.p + r.r - 2 p.r from three v_dot4_u32_u8, exact mod 2^32.  sat(|d| - s) of
// the four bytes comes as u16 pairs (widen, pk_absdiff, pk_subsat); pk_min1 makes each 1 where the pixel is over, v_perm
// packs the four into the bytes of a dword `over`, and (over ^ 0x01010101) * 0xff is 0xff in the bytes of the inside pixels
// (a byte is 0 or 1 times 255: no carry).  With P = p & mask and R = r & mask an outside pixel contributes 0 - 0, so the
// inside sum of d is sad(P, 0) - sad(R, 0) and that of d^2 P.P + R.R - 2 P.R.  The clipped pixels are the set bits of
// lc_zero_bytes of p, ~p, r and ~r, OR-ed.
// A lane sums 64 pixels: each of its nine partial sums is at most 64 * 2 * 65025 < 2^24.  A cell has 16384: the sums of
// squares and of |d| at most 16384 * 255^2 = 1065369600 < 2^31, sum d a magnitude of at most 16384 * 255, the counts at most
// 16384.  The differences (sum d, the two p.p + r.r - 2 p.r) are taken per lane in u32, where they are exact mod 2^32, and
// the true value of every word fits i32, and the sums over lanes and waves are exact mod 2^32 as well.
//
// Bounds.  A job is read only if all three of its streams lie inside their buffers (nc_job_ok).  No ring: every dword a
// lane loads lies wholly inside the W * H bytes of its stream; sh_load4 tests the index against W * H besides.
namespace {

#define NC_WORDS 6u

__device__ __forceinline__ bool nc_job_ok(const abub_stat_job &jb, uint64_t frames_bytes, uint64_t model_bytes, uint64_t P)
{
    return frame_in_range(jb.cur, frames_bytes, P) && frame_in_range(jb.ref, frames_bytes, P) && frame_in_range(jb.model, model_bytes, P);
}

__global__ __launch_bounds__(FR_THREADS) void k_noise_cells(const uint8_t *frames, uint64_t frames_bytes, const uint8_t *sigma6,
                                                            uint64_t model_bytes, const abub_stat_job *__restrict__ jobs, int njobs,
                                                            uint32_t W, uint32_t H, uint32_t ncx, uint32_t x0, uint32_t y0,
                                                            uint32_t *__restrict__ status, uint32_t *__restrict__ rec)
{
    __shared__ uint32_t part[FR_THREADS / 64][NC_WORDS];
    const Cell c = cells_here(W, H, ncx, x0, y0);
    for (uint32_t j = blockIdx.y; j < (uint32_t)njobs; j += gridDim.y) {
        const abub_stat_job jb = jobs[j];
        const bool ok = nc_job_ok(jb, frames_bytes, model_bytes, c.P);
        uint32_t *out = cells_open<NC_WORDS>(j, ok, status, rec);
        if (!ok) {
            cells_zero<NC_WORDS>(out);
            continue;
        }
        const uint8_t *p = frames + jb.cur, *q = frames + jb.ref, *sg = sigma6 + jb.model;
        uint32_t nOver = 0, nClip = 0, inP = 0, inR = 0, inSq = 0, inPr = 0, sad = 0, allSq = 0, allPr = 0;
#pragma unroll
        for (uint32_t r = 0; r < FC_ROWS; ++r) {
            const uint64_t i = c.at(r);
            const uint32_t a = sh_load4(p, i, c.P), b = sh_load4(q, i, c.P), s = sh_load4(sg, i, c.P);
            sad = __builtin_amdgcn_sad_u8(a, b, sad);
            allSq = __builtin_amdgcn_udot4(a, a, allSq, false);
            allSq = __builtin_amdgcn_udot4(b, b, allSq, false);
            allPr = __builtin_amdgcn_udot4(a, b, allPr, false);
            const uint32_t lo = pk_min1(pk_subsat(pk_absdiff(widen_lo(a), widen_lo(b)), widen_lo(s)));
            const uint32_t hi = pk_min1(pk_subsat(pk_absdiff(widen_hi(a), widen_hi(b)), widen_hi(s)));
            const uint32_t over = __builtin_amdgcn_perm(hi, lo, 0x06040200u); // 1 in the byte of every pixel with |d| > s
            const uint32_t mask = (over ^ 0x01010101u) * 0xffu;
            const uint32_t am = a & mask, bm = b & mask;
            nOver += (uint32_t)__builtin_popcount(over);
            inP = __builtin_amdgcn_sad_u8(am, 0u, inP);
            inR = __builtin_amdgcn_sad_u8(bm, 0u, inR);
            inSq = __builtin_amdgcn_udot4(am, am, inSq, false);
            inSq = __builtin_amdgcn_udot4(bm, bm, inSq, false);
            inPr = __builtin_amdgcn_udot4(am, bm, inPr, false);
            nClip += (uint32_t)__builtin_popcount(lc_zero_bytes(a) | lc_zero_bytes(~a) | lc_zero_bytes(b) | lc_zero_bytes(~b));
        }
        uint32_t acc[NC_WORDS] = {nOver, nClip, inP - inR, inSq - 2u * inPr, sad, allSq - 2u * allPr};
        cells_close(c, acc, part, out);
    }
}

} // namespace

extern "C" int abub_frame_noise_cells_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *sigma6, size_t model_bytes,
                                          const abub_stat_job *jobs, int njobs, int W, int H, int x0, int y0, int ncx, int ncy,
                                          uint32_t *status, int32_t *rec, void *stream)
{
    const int chk = cells_check("abub_frame_noise_cells_dev", frames && sigma6 && jobs && status && rec, jobs, status, rec, njobs, W, H,
                                x0, y0, ncx, ncy, 0);
    if (chk != CELLS_LAUNCH)
        return chk;
    k_noise_cells<<<cells_grid(ncx, ncy, njobs), FR_THREADS, 0, (hipStream_t)stream>>>(
        frames, (uint64_t)frames_bytes, sigma6, (uint64_t)model_bytes, jobs, njobs, (uint32_t)W, (uint32_t)H, (uint32_t)ncx, (uint32_t)x0,
        (uint32_t)y0, status, (uint32_t *)rec);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}

// ---- per-line sums of whole frames: abub_frame_lines_dev ("Surveying a run for torn, repeated and banded
// frames") ----------------------------------------------------------------------------------------------------------------
// Per job and image row y five u32 over the row's W pixels p of the frame, m of mu and r of the reference frame (host/survey.cpp
// linesHost, the definition): sum p, sum |p - m|, the pixels at 0 or 255, sum |p - r|, the pixels with p == r (the last two 0
// for a job without a reference, ref == UINT64_MAX); per image column x the first three over the column's H pixels.
//
// One block of four waves owns one job at a time and with it every output word of the job: plain stores, no atomics on
// memory, no clearing launch.  The frame is walked in bands of LN_BAND rows and, inside a band, in strips of LN_STRIP pixels
// across; in a strip lane l owns the 16 pixels from 16 l on, down the band, and wave w takes the band's rows w, w + 4, ...
// (48 bytes of a lane in flight per row, 16 waves on a CU: no unrolling over rows).  A lane keeps its 16 columns' three sums in 48 registers through the strip; at the strip's end the
// four waves add them into 48 x 64 words of LDS (ds_add, integers: any order gives the same bits), and thread t hands columns
// t, t + 256, ... to cols[]: stored in the frame's first band, added to its own word in the later ones (the same thread every
// time, so program order is enough).  A row's five sums are packed into three words (sum p < 2^18 and n_clip <= 1024 in one,
// sum |p - m| and n_same in the next, sum |p - r|), summed over the wave by the butterfly, and lane 0 keeps the row's five
// words in LDS: stored in the band's first strip, added to in the others, by that one thread; after the band's last strip
// the block writes the band's rows out in one contiguous run.
// Loads: a lane's 16 bytes of a stream come in one 16-byte load where the row's address in the strip is a multiple of 16 and
// the bytes end inside the stream, else as five aligned dwords and v_alignbyte (single bytes at the stream's two ends).
// Bytes past the row's end belong to the next row (or are zeros past the stream): the row sums mask them out, and the column
// sums of columns >= W are never stored.
// Bounds.  A job is read only if its frame and its plane lie inside their buffers and its reference is absent or inside
// (ln_job_ok); otherwise E_RANGE and zero records.  Every load is at an index below P = W * H of its stream (ln_load16 tests
// every one of its three forms).  Stores: status[j], rows[(j H + y) 5 + k] with y < H, cols[(j W + x) 3 + k] with
// x < W, j < njobs.  Sums: a lane's column sums over at most 256 rows, the LDS words over at most 1024 rows, a word of the
// result at most 65535 * 255 < 2^24.
namespace {

#define LN_ROW_WORDS ((uint32_t)ABUB_LINES_ROW_WORDS)
#define LN_COL_WORDS ((uint32_t)ABUB_LINES_COL_WORDS)
#define LN_WAVES (FR_THREADS / 64u)
#define LN_STRIP 1024u /* pixels of a strip across: 64 lanes of 16 */
#define LN_BAND 1024u  /* rows of a band: 20 KiB of row words in LDS */
#define LN_PAD 65u     /* words of a row of the column sums in LDS (64 lanes and one: the readers spread over the banks) */
static_assert(LN_ROW_WORDS == 5u && LN_COL_WORDS == 3u, "the packing below is of five and three words");

__device__ __forceinline__ bool ln_job_ok(const abub_stat_job &jb, uint64_t frames_bytes, uint64_t model_bytes, uint64_t P)
{
    return frame_in_range(jb.cur, frames_bytes, P) && frame_in_range(jb.model, model_bytes, P) &&
           (jb.ref == ST_NONE || frame_in_range(jb.ref, frames_bytes, P));
}

// the 16 bytes from index i on of a stream of P bytes, in memory order (wide: the address is a multiple of 16); bytes at P
// and beyond read as 0; zeros where `on` is false.  Nothing outside [s, s + P) is touched: the five aligned dwords around
// the bytes only where they lie inside, else byte by byte (the stream's first and last bytes)
// (P = W * H <= 65535^2 and i < P + 1040: 32 bits hold every index and every sum below)
__device__ __forceinline__ u32x4 ln_load16(const uint8_t *s, uint32_t i, uint32_t P, bool wide, bool on)
{
    u32x4 v = {0u, 0u, 0u, 0u};
    if (!on)
        return v;
    if (wide && i + 16u <= P)
        return *reinterpret_cast<const u32x4 *>(s + i);
    const uint32_t mis = (uint32_t)((uintptr_t)(s + i) & 3u);
    if (i >= mis && i - mis + 20u <= P) {
        const uint32_t *a = reinterpret_cast<const uint32_t *>(s + (i - mis));
        const uint32_t a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4];
        v.x = __builtin_amdgcn_alignbyte(a1, a0, mis);
        v.y = __builtin_amdgcn_alignbyte(a2, a1, mis);
        v.z = __builtin_amdgcn_alignbyte(a3, a2, mis);
        v.w = __builtin_amdgcn_alignbyte(a4, a3, mis);
        return v;
    }
#pragma unroll 1
    for (uint32_t k = 0; k < 16u; ++k) { // (a 16-byte shift register: byte k ends at place k)
        const uint32_t byte = i + k < P ? (uint32_t)s[i + k] : 0u;
        v.x = (v.x >> 8) | (v.y << 24);
        v.y = (v.y >> 8) | (v.z << 24);
        v.z = (v.z >> 8) | (v.w << 24);
        v.w = (v.w >> 8) | (byte << 24);
    }
    return v;
}

struct LnRow { // what a lane holds of one row
    u32x4 p, m, r;
};

struct LnCols { // a lane's 16 columns
    uint32_t sum[16], dev[16], clip[16];
};

// one dword of a row: its four columns, and the row's sums under the mask of the bytes that lie in the row
template <int D>
__device__ __forceinline__ void ln_dword(uint32_t p, uint32_t m, uint32_t r, bool ref, uint32_t vm, LnCols &c, uint32_t &sp, uint32_t &sm,
                                         uint32_t &sr, uint32_t &nclip, uint32_t &nsame)
{
    const uint32_t clip = lc_zero_bytes(p) | lc_zero_bytes(~p); // 0x80 in the bytes at 0 or 255
    const uint32_t pv = p & vm;
    sp = __builtin_amdgcn_sad_u8(pv, 0u, sp);
    sm = __builtin_amdgcn_sad_u8(pv, m & vm, sm);
    nclip += (uint32_t)__builtin_popcount(clip & vm);
    if (ref) {
        sr = __builtin_amdgcn_sad_u8(pv, r & vm, sr);
        nsame += (uint32_t)__builtin_popcount(lc_zero_bytes(p ^ r) & vm);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t byte = 0xffu << (8 * k), pk = p & byte;
        c.sum[4 * D + k] = __builtin_amdgcn_sad_u8(pk, 0u, c.sum[4 * D + k]);
        c.dev[4 * D + k] = __builtin_amdgcn_sad_u8(pk, m & byte, c.dev[4 * D + k]);
        c.clip[4 * D + k] += (clip >> (8 * k + 7)) & 1u;
    }
}

__global__ __launch_bounds__(FR_THREADS) void k_lines(const uint8_t *frames, uint64_t frames_bytes, const uint8_t *mu, uint64_t model_bytes,
                                                      const abub_stat_job *__restrict__ jobs, int njobs, uint32_t W, uint32_t H,
                                                      uint32_t *__restrict__ status, uint32_t *__restrict__ rows,
                                                      uint32_t *__restrict__ cols)
{
    __shared__ uint32_t rowpart[LN_BAND][LN_ROW_WORDS];
    __shared__ uint32_t colsum[LN_COL_WORDS][16][LN_PAD];
    const uint32_t P = W * H; // (at most 65535^2 < 2^32)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll 1
    for (uint32_t t = threadIdx.x; t < LN_COL_WORDS * 16u * LN_PAD; t += FR_THREADS)
        (&colsum[0][0][0])[t] = 0u;
    __syncthreads();
    for (uint32_t j = blockIdx.x; j < (uint32_t)njobs; j += gridDim.x) {
        const abub_stat_job jb = jobs[j];
        const bool ok = ln_job_ok(jb, frames_bytes, model_bytes, (uint64_t)P); // (the same in every thread of the block)
        uint32_t *jrows = rows + (uint64_t)j * H * LN_ROW_WORDS, *jcols = cols + (uint64_t)j * W * LN_COL_WORDS;
        if (threadIdx.x == 0u)
            status[j] = ok ? 0u : (uint32_t)ABUB_SHIFT_E_RANGE;
        if (!ok) {
#pragma unroll 1
            for (uint32_t t = threadIdx.x; t < H * LN_ROW_WORDS; t += FR_THREADS)
                jrows[t] = 0u;
#pragma unroll 1
            for (uint32_t t = threadIdx.x; t < W * LN_COL_WORDS; t += FR_THREADS)
                jcols[t] = 0u;
            continue;
        }
        const bool ref = jb.ref != ST_NONE;
        const uint8_t *p = frames + jb.cur, *m = mu + jb.model, *q = frames + (ref ? jb.ref : jb.cur);
        const uint32_t lowP = (uint32_t)(uintptr_t)p, lowM = (uint32_t)(uintptr_t)m, lowQ = (uint32_t)(uintptr_t)q;
        for (uint32_t yb = 0; yb < H; yb += LN_BAND) {
            const uint32_t yEnd = min(H, yb + LN_BAND);
            for (uint32_t xs = 0; xs < W; xs += LN_STRIP) {
                const uint32_t x = xs + 16u * lane;
                const bool on = x < W;
                const uint32_t left = on ? min(W - x, 16u) : 0u; // the lane's bytes that lie in the row
                uint32_t vm[4];
#pragma unroll
                for (uint32_t d = 0; d < 4u; ++d)
                    vm[d] = left >= 4u * d + 4u ? 0xffffffffu : left > 4u * d ? (1u << (8u * (left - 4u * d))) - 1u : 0u;
                LnCols c = {};
#pragma unroll 1
                for (uint32_t y = yb + wave; y < yEnd; y += LN_WAVES) {
                    const uint32_t low = y * W + xs, i = low + 16u * lane; // (mod 16 the row's address in the strip is the stream's plus `low`)
                    LnRow row;
                    row.p = ln_load16(p, i, P, ((lowP + low) & 15u) == 0u, on);
                    row.m = ln_load16(m, i, P, ((lowM + low) & 15u) == 0u, on);
                    row.r = ln_load16(q, i, P, ((lowQ + low) & 15u) == 0u, on && ref);
                    uint32_t sp = 0, sm = 0, sr = 0, nclip = 0, nsame = 0;
                    ln_dword<0>(row.p.x, row.m.x, row.r.x, ref, vm[0], c, sp, sm, sr, nclip, nsame);
                    ln_dword<1>(row.p.y, row.m.y, row.r.y, ref, vm[1], c, sp, sm, sr, nclip, nsame);
                    ln_dword<2>(row.p.z, row.m.z, row.r.z, ref, vm[2], c, sp, sm, sr, nclip, nsame);
                    ln_dword<3>(row.p.w, row.m.w, row.r.w, ref, vm[3], c, sp, sm, sr, nclip, nsame);
                    // (over the wave: sums of at most 1024 * 255 < 2^18, counts of at most 1024 < 2^11)
                    uint32_t a = sp | (nclip << 18), b = sm | (nsame << 18), d = sr;
                    wave_reduce<WaveSum, WaveSum, WaveSum>(a, b, d);
                    if (lane == 0u) {
                        uint32_t *rp = rowpart[y - yb];
                        const uint32_t v[LN_ROW_WORDS] = {a & 0x3ffffu, b & 0x3ffffu, a >> 18, d, b >> 18};
#pragma unroll
                        for (uint32_t k = 0; k < LN_ROW_WORDS; ++k)
                            rp[k] = xs == 0u ? v[k] : rp[k] + v[k];
                    }
                }
                // (a lane of a strip's columns >= W holds what the next row's bytes gave it: it is never stored)
#pragma unroll
                for (uint32_t k = 0; k < 16u; ++k) {
                    atomicAdd(&colsum[0][k][lane], c.sum[k]);
                    atomicAdd(&colsum[1][k][lane], c.dev[k]);
                    atomicAdd(&colsum[2][k][lane], c.clip[k]);
                }
                __syncthreads();
#pragma unroll 1
                for (uint32_t cx = threadIdx.x; cx < LN_STRIP; cx += FR_THREADS) {
#pragma unroll
                    for (uint32_t k = 0; k < LN_COL_WORDS; ++k) {
                        const uint32_t v = colsum[k][cx & 15u][cx >> 4];
                        colsum[k][cx & 15u][cx >> 4] = 0u;
                        if (xs + cx < W) {
                            uint32_t *out = jcols + (uint64_t)(xs + cx) * LN_COL_WORDS + k;
                            *out = yb == 0u ? v : *out + v;
                        }
                    }
                }
                __syncthreads(); // (the column sums are zero again, and every row word of the strip is in LDS)
            }
#pragma unroll 1
            for (uint32_t t = threadIdx.x; t < (yEnd - yb) * LN_ROW_WORDS; t += FR_THREADS)
                jrows[(uint64_t)yb * LN_ROW_WORDS + t] = (&rowpart[0][0])[t];
            __syncthreads(); // (rowpart is written again in the next band, or job)
        }
    }
}

} // namespace

extern "C" int abub_frame_lines_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, size_t model_bytes,
                                    const abub_stat_job *jobs, int njobs, int W, int H, uint32_t *status, uint32_t *rows, uint32_t *cols,
                                    void *stream)
{
    if (!frames || !mu || !jobs || !status || !rows || !cols || njobs < 0)
        return set_err(ABUB_E_INVALID, "abub_frame_lines_dev: null pointer or negative count");
    if (W < 1 || W > 65535 || H < 1 || H > 65535)
        return set_err(ABUB_E_INVALID, "abub_frame_lines_dev: W and H must be in [1, 65535]");
    if (((uintptr_t)jobs & 7) || (((uintptr_t)status | (uintptr_t)rows | (uintptr_t)cols) & 3))
        return set_err(ABUB_E_INVALID, "abub_frame_lines_dev: jobs must be 8-byte aligned, status, rows and cols 4-byte aligned");
    if (njobs == 0)
        return ABUB_OK;
    k_lines<<<dim3((unsigned)(njobs < 65535 ? njobs : 65535)), FR_THREADS, 0, (hipStream_t)stream>>>(
        frames, (uint64_t)frames_bytes, mu, (uint64_t)model_bytes, jobs, njobs, (uint32_t)W, (uint32_t)H, status, rows, cols);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}
