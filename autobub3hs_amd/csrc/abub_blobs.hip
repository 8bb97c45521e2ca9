// abub_blobs.hip -- what the host needs to trace an image's contours, decided on the GPU (gfx950):
//   k_binarize_thr                 Otsu threshold of the TOZERO'd image from its histogram (binarizeThresholdFromHist)
//   K4b k4b_small, k4b_large       8-connected labelling of each slot's foreground (val > thr) with a box filter
//       k4b_scan, k4b_scatter      per-slot offsets of the kept lists, compaction
//
// Why the box filter cannot change a result.  Tracking frames (L3Localizer.cpp:785-836, host/L3Localizer.cpp
// CalculatePostTriggerFrameParams) drop every contour whose bounding rect has area <= 10.  The vertices of a contour that
// ContourFinder traces are pixels of one 8-connected component, so the contour's bounding rect lies inside the
// component's bbox: a component with bbox area <= 10 can only yield a contour that tracking drops.  Such a component
// cannot enclose another one either: enclosing needs an 8-connected ring around a 4-connected background ring around an
// inner pixel, i.e. a bbox of at least 5 x 5.  So removing it changes neither the contours of the other components nor
// which of them RETR_EXTERNAL reports.  The GPU does not decide nesting: it keeps every component that passes the
// filter and ContourFinder still drops the nested ones.  Genesis images and bellows residuals pass min_box_area = -1
// (keep everything): largestBoxArea and allInBellowsMask (L3Localizer.cpp:123-178) depend on the small contours.
#include <float.h>

#include "abub_dev.hpp"

// ------------------------------------------------------------------------------------------------
// Otsu (host/hostlogic.cpp binarizeThresholdFromHist, reference L3Localizer.cpp:252-254, 786-787): one lane per slot
// runs the host's serial loops in double, in the host's order (the summation order is part of the result; the TU is
// built with -ffp-contract=off like the host).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_binarize_thr(const uint32_t *__restrict__ hist, const int32_t *__restrict__ tozero,
                                                     int nslots, double scale, int32_t *__restrict__ thr)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots)
        return;
    const uint32_t *hs = hist + (size_t)s * 256;
    const int tz = tozero[s];
    // h[i] = 0 for i <= tz, h[0] = the folded mass (0 when tz < 0, as on the host)
    double folded = 0;
    for (int i = 0; i <= tz && i < 256; ++i)
        folded += (double)hs[i];
    double mu = 0;
    for (int i = 0; i < 256; ++i) {
        const double h = i == 0 ? folded : (i <= tz ? 0. : (double)hs[i]);
        mu += i * h;
    }
    mu *= scale;
    double mu1 = 0, q1 = 0, best = 0;
    int T = 0;
    for (int i = 0; i < 256; ++i) {
        const double h = i == 0 ? folded : (i <= tz ? 0. : (double)hs[i]);
        const double p = h * scale;
        mu1 *= q1;
        q1 += p;
        const double q2 = 1. - q1;
        if ((q1 < q2 ? q1 : q2) < (double)FLT_EPSILON || (q1 < q2 ? q2 : q1) > 1. - (double)FLT_EPSILON)
            continue;
        mu1 = (mu1 + i * p) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double between = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
        if (between > best) {
            best = between;
            T = i;
        }
    }
    thr[s] = tz > T ? tz : T;
}

extern "C" int abub_binarize_thr_dev(const uint32_t *hist, const int32_t *tozero, int nslots, int W, int H, int32_t *thr,
                                     void *stream)
{
    if (!hist || !tozero || !thr || nslots < 0 || W <= 0 || H <= 0)
        return set_err(ABUB_E_INVALID, "abub_binarize_thr_dev: bad arguments");
    if (nslots == 0)
        return ABUB_OK;
    const double scale = 1. / (double)((size_t)W * H);
    hipLaunchKernelGGL(k_binarize_thr, dim3((nslots + 63) / 64), dim3(64), 0, (hipStream_t)stream, hist, tozero, nslots,
                       scale, thr);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}

// ------------------------------------------------------------------------------------------------
// K4b
// ------------------------------------------------------------------------------------------------
#define K4B_LDS_N 2048  /* foreground pixels a slot may have to be labelled in LDS (k4b_small) */
#define K4B_SMALL_T 256 /* threads of k4b_small: K4B_LDS_N / K4B_SMALL_T consecutive positions per thread */
#define K4B_LARGE_T 1024
#define K4B_LARGE_WG 4  /* workgroups of k4b_large; each owns K4B_PLANES planes of W*H u32 in the scratch */
#define K4B_PLANES 5    /* label, x0, x1, y1, count */
#define K4B_RUN 16      /* consecutive raster pixels per thread in k4b_large's ordered compaction */

// scratch layout (each piece 256-byte aligned): header (large-slot counter), large-slot list [nslots], kept pixel count
// per slot [nslots], staged kept pixels [in_cap], staged descriptors [in_cap] (with_comp only), planes
struct K4bScratch {
    uint32_t *hdr, *large, *kc, *stage;
    abub_blob *cstage;
    uint32_t *planes;
};
static size_t k4b_align(size_t b) { return (b + 255) & ~(size_t)255; }
static size_t k4b_layout(int nslots, int W, int H, uint32_t in_cap, int with_comp, char *base, K4bScratch *o)
{
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *p = base ? base + off : nullptr;
        off += k4b_align(bytes);
        return p;
    };
    K4bScratch s;
    s.hdr = (uint32_t *)take(256);
    s.large = (uint32_t *)take((size_t)nslots * 4);
    s.kc = (uint32_t *)take((size_t)nslots * 4);
    s.stage = (uint32_t *)take((size_t)in_cap * 4);
    s.cstage = with_comp ? (abub_blob *)take((size_t)in_cap * sizeof(abub_blob)) : nullptr;
    s.planes = (uint32_t *)take((size_t)K4B_LARGE_WG * K4B_PLANES * W * H * 4);
    if (o)
        *o = s;
    return off;
}

// exclusive prefix sum of two per-thread counts over the workgroup (in thread order) + totals
template <int NT>
__device__ __forceinline__ void k4b_scan2(uint32_t a, uint32_t b, uint32_t &pa, uint32_t &pb, uint32_t &ta, uint32_t &tb,
                                          uint32_t *lds /* [2 * NT / 64] */)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    constexpr int NW = NT / 64;
    uint32_t ia = a, ib = b;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t xa = __shfl_up(ia, o), xb = __shfl_up(ib, o);
        if (lane >= o) {
            ia += xa;
            ib += xb;
        }
    }
    __syncthreads(); // (lds may still be read by a previous call)
    if (lane == 63) {
        lds[w] = ia;
        lds[NW + w] = ib;
    }
    __syncthreads();
    uint32_t ba = 0, bb = 0;
    ta = tb = 0;
    for (int k = 0; k < NW; ++k) {
        if (k < w) {
            ba += lds[k];
            bb += lds[NW + k];
        }
        ta += lds[k];
        tb += lds[NW + k];
    }
    pa = ba + ia - a;
    pb = bb + ib - b;
}

__device__ __forceinline__ bool k4b_keep(int x0, int y0, int x1, int y1, int min_box)
{
    return min_box < 0 || (long long)(x1 - x0 + 1) * (long long)(y1 - y0 + 1) > (long long)min_box;
}

// ---- LDS path: sort the slot's foreground indices, neighbours by binary search, union-find on positions ----------------
__device__ __forceinline__ uint32_t k4b_find_lds(volatile uint32_t *par, uint32_t a)
{
    uint32_t p = par[a];
    while (p != a) {
        a = p;
        p = par[a];
    }
    return a;
}
// Playne & Hawick's atomicMin union: the smaller position becomes the root, so a root is its component's first pixel
__device__ __forceinline__ void k4b_union_lds(uint32_t *par, uint32_t a, uint32_t b)
{
    for (;;) {
        a = k4b_find_lds(par, a);
        b = k4b_find_lds(par, b);
        if (a == b)
            return;
        if (a < b) {
            const uint32_t old = atomicMin(&par[b], a);
            if (old == b)
                return;
            b = old;
        } else {
            const uint32_t old = atomicMin(&par[a], b);
            if (old == a)
                return;
            a = old;
        }
    }
}

__global__ __launch_bounds__(K4B_SMALL_T) void k4b_small(const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ idx,
                                                         const uint8_t *__restrict__ val, uint32_t in_cap, int W,
                                                         const int32_t *__restrict__ thr, const int32_t *__restrict__ min_box,
                                                         uint32_t *__restrict__ ncomp, uint32_t *__restrict__ nkept_comp,
                                                         K4bScratch S, uint32_t *__restrict__ stats)
{
    __shared__ uint32_t key[K4B_LDS_N], par[K4B_LDS_N], bx0[K4B_LDS_N], bx1[K4B_LDS_N], by1[K4B_LDS_N], cnt[K4B_LDS_N];
    __shared__ uint32_t red[2 * K4B_SMALL_T / 64];
    __shared__ uint32_t nk;
    const int s = blockIdx.x, t = threadIdx.x;
    uint32_t o0 = offsets[s], o1 = offsets[s + 1];
    o0 = o0 < in_cap ? o0 : in_cap; // an overflowed list: read only what was written (the caller redoes the batch)
    o1 = o1 < in_cap ? o1 : in_cap;
    o1 = o1 > o0 ? o1 : o0;
    const int th = thr[s], mb = min_box[s];
    uint32_t nfg = 0, tot, td, pd, pd2;
    for (uint32_t k = o0 + t; k < o1; k += K4B_SMALL_T)
        nfg += (int)val[k] > th;
    k4b_scan2<K4B_SMALL_T>(nfg, 0, pd, pd2, tot, td, red);
    const uint32_t n = tot;
    if (t == 0)
        atomicAdd(&stats[1], n);
    if (n > K4B_LDS_N) {
        if (t == 0) {
            S.large[atomicAdd(&S.hdr[0], 1u)] = (uint32_t)s;
            atomicAdd(&stats[0], 1u);
        }
        return;
    }
    if (t == 0)
        nk = 0;
    uint32_t np2 = 1;
    while (np2 < n)
        np2 <<= 1;
    __syncthreads();
    for (uint32_t k = o0 + t; k < o1; k += K4B_SMALL_T)
        if ((int)val[k] > th)
            key[atomicAdd(&nk, 1u)] = idx[k];
    for (uint32_t p = n + t; p < np2; p += K4B_SMALL_T)
        key[p] = 0xffffffffu;
    __syncthreads();
    // bitonic sort of key[0 .. np2)
    for (uint32_t size = 2; size <= np2; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t q = t; q < np2 / 2; q += K4B_SMALL_T) {
                const uint32_t i = 2 * q - (q & (stride - 1)), j = i + stride;
                const bool up = (i & size) == 0;
                const uint32_t a = key[i], b = key[j];
                if ((a > b) == up) {
                    key[i] = b;
                    key[j] = a;
                }
            }
            __syncthreads();
        }
    for (uint32_t p = t; p < n; p += K4B_SMALL_T) {
        const uint32_t k = key[p];
        par[p] = p;
        bx0[p] = bx1[p] = k % (uint32_t)W;
        by1[p] = k / (uint32_t)W;
        cnt[p] = 0;
    }
    __syncthreads();
    // earlier 8-neighbours W, NW, N, NE
    for (uint32_t p = t; p < n; p += K4B_SMALL_T) {
        const uint32_t k = key[p], x = k % (uint32_t)W, y = k / (uint32_t)W;
        if (x > 0 && p > 0 && key[p - 1] == k - 1)
            k4b_union_lds(par, p, p - 1);
        if (y > 0) {
            const uint32_t lo = (y - 1) * W + (x > 0 ? x - 1 : 0), hi = (y - 1) * W + (x + 1 < (uint32_t)W ? x + 1 : x);
            uint32_t a = 0, b = p; // lower_bound(key[0 .. p), lo)
            while (a < b) {
                const uint32_t m = (a + b) >> 1;
                if (key[m] < lo)
                    a = m + 1;
                else
                    b = m;
            }
            for (; a < p && key[a] <= hi; ++a)
                k4b_union_lds(par, p, a);
        }
    }
    __syncthreads();
    for (uint32_t p = t; p < n; p += K4B_SMALL_T)
        par[p] = k4b_find_lds(par, p);
    __syncthreads();
    for (uint32_t p = t; p < n; p += K4B_SMALL_T) {
        const uint32_t r = par[p], k = key[p], x = k % (uint32_t)W, y = k / (uint32_t)W;
        atomicMin(&bx0[r], x);
        atomicMax(&bx1[r], x);
        atomicMax(&by1[r], y);
        atomicAdd(&cnt[r], 1u);
    }
    __syncthreads();
    // ordered compaction: thread t owns positions [t*R, t*R + R)
    constexpr uint32_t R = K4B_LDS_N / K4B_SMALL_T;
    const uint32_t p0 = t * R, p1 = p0 + R < n ? p0 + R : n;
    uint32_t kp = 0, kr = 0, nr = 0;
    for (uint32_t p = p0; p < p1; ++p) {
        const uint32_t r = par[p];
        const bool kept = k4b_keep(bx0[r], key[r] / (uint32_t)W, bx1[r], by1[r], mb);
        kp += kept;
        kr += kept && r == p;
        nr += r == p;
    }
    uint32_t pp, pr, tkp, tkr;
    k4b_scan2<K4B_SMALL_T>(kp, kr, pp, pr, tkp, tkr, red);
    for (uint32_t p = p0; p < p1; ++p) {
        const uint32_t r = par[p], y0 = key[r] / (uint32_t)W;
        if (!k4b_keep(bx0[r], y0, bx1[r], by1[r], mb))
            continue;
        S.stage[o0 + pp++] = key[p]; // (kept <= foreground <= o1 - o0: stays inside the slot's range)
        if (r == p && S.cstage) {
            abub_blob b;
            b.first = key[p];
            b.x0 = (int32_t)bx0[p];
            b.y0 = (int32_t)y0;
            b.x1 = (int32_t)bx1[p];
            b.y1 = (int32_t)by1[p];
            b.npix = cnt[p];
            S.cstage[o0 + pr++] = b;
        }
    }
    k4b_scan2<K4B_SMALL_T>(nr, 0, pd, pd2, tot, td, red);
    if (t == 0) {
        S.kc[s] = tkp;
        ncomp[s] = tot;
        nkept_comp[s] = tkr;
        atomicAdd(&stats[2], tot);
        atomicAdd(&stats[3], tkr);
    }
}

// ---- global path: slots with more than K4B_LDS_N foreground pixels, on dense planes in the scratch ---------------------
// planes: the K4B_LARGE_WG label planes, then 4 planes per workgroup.  L holds label + 1 per pixel (0 = background); x0 / x1 / y1 / count are read at the root only.  Everything goes
// through L2 (agent-scope atomics, atomic loads and stores), so no wave of the workgroup ever reads a stale L1 line.
__device__ __forceinline__ uint32_t k4b_ld(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void k4b_st(uint32_t *p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t k4b_find_g(const uint32_t *L, uint32_t a)
{
    uint32_t p = k4b_ld(&L[a]) - 1;
    while (p != a) {
        a = p;
        p = k4b_ld(&L[a]) - 1;
    }
    return a;
}
__device__ __forceinline__ void k4b_union_g(uint32_t *L, uint32_t a, uint32_t b)
{
    for (;;) {
        a = k4b_find_g(L, a);
        b = k4b_find_g(L, b);
        if (a == b)
            return;
        if (a < b) {
            const uint32_t old = atomicMin(&L[b], a + 1) - 1;
            if (old == b)
                return;
            b = old;
        } else {
            const uint32_t old = atomicMin(&L[a], b + 1) - 1;
            if (old == a)
                return;
            a = old;
        }
    }
}
__device__ __forceinline__ void k4b_phase()
{
    __threadfence();
    __syncthreads();
}

__global__ __launch_bounds__(K4B_LARGE_T) void k4b_large(const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ idx,
                                                         const uint8_t *__restrict__ val, uint32_t in_cap, int W, int H,
                                                         const int32_t *__restrict__ thr, const int32_t *__restrict__ min_box,
                                                         uint32_t *__restrict__ ncomp, uint32_t *__restrict__ nkept_comp,
                                                         K4bScratch S, uint32_t *__restrict__ stats)
{
    __shared__ uint32_t red[2 * K4B_LARGE_T / 64];
    __shared__ uint32_t lohi[2];
    const int t = threadIdx.x;
    const uint32_t P = (uint32_t)W * (uint32_t)H;
    uint32_t *L = S.planes + (size_t)blockIdx.x * P, *bx0 = S.planes + (size_t)(K4B_LARGE_WG + 4 * blockIdx.x) * P,
             *bx1 = bx0 + P, *by1 = bx1 + P, *cnt = by1 + P;
    const uint32_t nlarge = k4b_ld(&S.hdr[0]);
    for (uint32_t j = blockIdx.x; j < nlarge; j += gridDim.x) {
        const int s = (int)S.large[j];
        uint32_t o0 = offsets[s], o1 = offsets[s + 1];
        o0 = o0 < in_cap ? o0 : in_cap;
        o1 = o1 < in_cap ? o1 : in_cap;
        o1 = o1 > o0 ? o1 : o0;
        const int th = thr[s], mb = min_box[s];
        if (t == 0) {
            lohi[0] = 0xffffffffu;
            lohi[1] = 0;
        }
        __syncthreads();
        for (uint32_t k = o0 + t; k < o1; k += K4B_LARGE_T) {
            const uint32_t i = idx[k];
            if ((int)val[k] > th && i < P) {
                k4b_st(&L[i], i + 1);
                k4b_st(&bx0[i], i % (uint32_t)W);
                k4b_st(&bx1[i], i % (uint32_t)W);
                k4b_st(&by1[i], i / (uint32_t)W);
                k4b_st(&cnt[i], 0);
                atomicMin(&lohi[0], i);
                atomicMax(&lohi[1], i);
            }
        }
        k4b_phase();
        for (uint32_t k = o0 + t; k < o1; k += K4B_LARGE_T) {
            const uint32_t i = idx[k];
            if (!((int)val[k] > th && i < P))
                continue;
            const uint32_t x = i % (uint32_t)W, y = i / (uint32_t)W;
            if (x > 0 && k4b_ld(&L[i - 1]))
                k4b_union_g(L, i, i - 1);
            if (y > 0) {
                if (x > 0 && k4b_ld(&L[i - W - 1]))
                    k4b_union_g(L, i, i - W - 1);
                if (k4b_ld(&L[i - W]))
                    k4b_union_g(L, i, i - W);
                if (x + 1 < (uint32_t)W && k4b_ld(&L[i - W + 1]))
                    k4b_union_g(L, i, i - W + 1);
            }
        }
        k4b_phase();
        for (uint32_t k = o0 + t; k < o1; k += K4B_LARGE_T) {
            const uint32_t i = idx[k];
            if ((int)val[k] > th && i < P)
                k4b_st(&L[i], k4b_find_g(L, i) + 1);
        }
        k4b_phase();
        for (uint32_t k = o0 + t; k < o1; k += K4B_LARGE_T) {
            const uint32_t i = idx[k];
            if (!((int)val[k] > th && i < P))
                continue;
            const uint32_t r = k4b_ld(&L[i]) - 1, x = i % (uint32_t)W, y = i / (uint32_t)W;
            atomicMin(&bx0[r], x);
            atomicMax(&bx1[r], x);
            atomicMax(&by1[r], y);
            atomicAdd(&cnt[r], 1u);
        }
        k4b_phase();
        // ordered compaction over the raster range the slot's foreground spans, K4B_RUN pixels per thread and round
        const uint32_t lo = lohi[0], hi = lohi[1];
        uint32_t wp = o0, wr = o0, nr = 0;
        for (uint32_t base = lo; lo <= hi && base <= hi; base += K4B_RUN * K4B_LARGE_T) {
            const uint32_t i0 = base + (uint32_t)t * K4B_RUN;
            uint32_t kp = 0, kr = 0, rr = 0;
            for (uint32_t i = i0; i < i0 + K4B_RUN && i <= hi; ++i) {
                const uint32_t l = k4b_ld(&L[i]);
                if (!l)
                    continue;
                const uint32_t r = l - 1;
                const bool kept = k4b_keep(k4b_ld(&bx0[r]), r / (uint32_t)W, k4b_ld(&bx1[r]), k4b_ld(&by1[r]), mb);
                kp += kept;
                kr += kept && r == i;
                rr += r == i;
            }
            uint32_t pp, pr, tkp, tkr;
            k4b_scan2<K4B_LARGE_T>(kp, kr, pp, pr, tkp, tkr, red);
            uint32_t q = wp + pp, qr = wr + pr;
            for (uint32_t i = i0; (kp || kr) && i < i0 + K4B_RUN && i <= hi; ++i) {
                const uint32_t l = k4b_ld(&L[i]);
                if (!l)
                    continue;
                const uint32_t r = l - 1, x0 = k4b_ld(&bx0[r]), x1 = k4b_ld(&bx1[r]), y1 = k4b_ld(&by1[r]);
                if (!k4b_keep(x0, r / (uint32_t)W, x1, y1, mb))
                    continue;
                if (q < o1) // (always: kept <= foreground <= o1 - o0)
                    S.stage[q++] = i;
                if (r == i && S.cstage && qr < o1) {
                    abub_blob b;
                    b.first = i;
                    b.x0 = (int32_t)x0;
                    b.y0 = (int32_t)(r / (uint32_t)W);
                    b.x1 = (int32_t)x1;
                    b.y1 = (int32_t)y1;
                    b.npix = k4b_ld(&cnt[r]);
                    S.cstage[qr++] = b;
                }
            }
            wp += tkp;
            wr += tkr;
            uint32_t d0, d1, trr, td;
            k4b_scan2<K4B_LARGE_T>(rr, 0, d0, d1, trr, td, red);
            nr += trr;
        }
        // leave the label plane zero for the next slot
        for (uint32_t k = o0 + t; k < o1; k += K4B_LARGE_T) {
            const uint32_t i = idx[k];
            if ((int)val[k] > th && i < P)
                k4b_st(&L[i], 0);
        }
        if (t == 0) {
            S.kc[s] = wp - o0;
            ncomp[s] = nr;
            nkept_comp[s] = wr - o0;
            atomicAdd(&stats[2], nr);
            atomicAdd(&stats[3], wr - o0);
        }
        k4b_phase();
    }
}

// single block: kept_off / comp_off = exclusive scans of the per-slot counts
__global__ __launch_bounds__(1024) void k4b_scan(const uint32_t *__restrict__ kc, const uint32_t *__restrict__ nkc,
                                                 uint32_t nslots, uint32_t *__restrict__ kept_off, uint32_t *__restrict__ comp_off)
{
    __shared__ uint32_t red[2 * 1024 / 64];
    const uint32_t t = threadIdx.x, per = (nslots + 1023) / 1024;
    const uint32_t lo = t * per < nslots ? t * per : nslots, hi = lo + per < nslots ? lo + per : nslots;
    uint32_t a = 0, b = 0;
    for (uint32_t i = lo; i < hi; ++i) {
        a += kc[i];
        b += nkc[i];
    }
    uint32_t pa, pb, ta, tb;
    k4b_scan2<1024>(a, b, pa, pb, ta, tb, red);
    for (uint32_t i = lo; i < hi; ++i) {
        kept_off[i] = pa;
        comp_off[i] = pb;
        pa += kc[i];
        pb += nkc[i];
    }
    if (t == 0) {
        kept_off[nslots] = ta;
        comp_off[nslots] = tb;
    }
}

__global__ __launch_bounds__(256) void k4b_scatter(const uint32_t *__restrict__ offsets, uint32_t in_cap,
                                                   const uint32_t *__restrict__ kept_off, const uint32_t *__restrict__ comp_off,
                                                   const uint32_t *__restrict__ nkc, K4bScratch S,
                                                   uint32_t *__restrict__ kept_idx, uint32_t cap, abub_blob *__restrict__ comp,
                                                   uint32_t comp_cap)
{
    const int s = blockIdx.x;
    const uint32_t o0 = offsets[s] < in_cap ? offsets[s] : in_cap;
    const uint32_t n = S.kc[s], d = kept_off[s];
    for (uint32_t k = threadIdx.x; k < n; k += 256)
        if (d + k < cap && o0 + k < in_cap)
            kept_idx[d + k] = S.stage[o0 + k];
    if (comp) {
        const uint32_t nc = nkc[s], dc = comp_off[s];
        for (uint32_t k = threadIdx.x; k < nc; k += 256)
            if (dc + k < comp_cap && o0 + k < in_cap)
                comp[dc + k] = S.cstage[o0 + k];
    }
}

extern "C" size_t abub_label_blobs_scratch_bytes(int nslots, int W, int H, uint32_t in_cap, int with_comp)
{
    if (nslots <= 0 || W <= 0 || H <= 0 || (size_t)W * H > 0xffffffffull - 1)
        return 0;
    return k4b_layout(nslots, W, H, in_cap, with_comp, nullptr, nullptr);
}

extern "C" int abub_label_blobs_dev(const uint32_t *offsets, const uint32_t *idx, const uint8_t *val, uint32_t in_cap,
                                    int nslots, int W, int H, const int32_t *thr, const int32_t *min_box_area,
                                    uint32_t *kept_off, uint32_t *kept_idx, uint32_t cap, uint32_t *ncomp,
                                    uint32_t *nkept_comp, uint32_t *comp_off, abub_blob *comp, uint32_t comp_cap,
                                    uint32_t *stats, void *scratch, size_t scratch_bytes, void *stream)
{
    if (!offsets || !idx || !val || !thr || !min_box_area || !kept_off || !kept_idx || !ncomp || !nkept_comp || !comp_off ||
        !stats || !scratch || nslots <= 0 || W <= 0 || H <= 0 || in_cap == 0 || cap == 0 || (comp && comp_cap == 0))
        return set_err(ABUB_E_INVALID, "abub_label_blobs_dev: bad arguments");
    const size_t need = abub_label_blobs_scratch_bytes(nslots, W, H, in_cap, comp != nullptr);
    if (need == 0 || scratch_bytes < need || ((uintptr_t)scratch & 255))
        return set_err(ABUB_E_INVALID, "abub_label_blobs_dev: scratch too small or not 256-byte aligned");
    K4bScratch S;
    k4b_layout(nslots, W, H, in_cap, comp != nullptr, (char *)scratch, &S);
    hipStream_t st = (hipStream_t)stream;
    const size_t P = (size_t)W * H;
    HIPCHK(hipMemsetAsync(S.hdr, 0, 256, st));
    HIPCHK(hipMemsetAsync(stats, 0, 4 * sizeof(uint32_t), st));
    // label planes start zero (k4b_large leaves them zero again, but a launch must not depend on the previous one)
    HIPCHK(hipMemsetAsync(S.planes, 0, (size_t)K4B_LARGE_WG * P * 4, st));
    hipLaunchKernelGGL(k4b_small, dim3(nslots), dim3(K4B_SMALL_T), 0, st, offsets, idx, val, in_cap, W, thr, min_box_area, ncomp,
                       nkept_comp, S, stats);
    hipLaunchKernelGGL(k4b_large, dim3(K4B_LARGE_WG), dim3(K4B_LARGE_T), 0, st, offsets, idx, val, in_cap, W, H, thr,
                       min_box_area, ncomp, nkept_comp, S, stats);
    hipLaunchKernelGGL(k4b_scan, dim3(1), dim3(1024), 0, st, S.kc, nkept_comp, (uint32_t)nslots, kept_off, comp_off);
    hipLaunchKernelGGL(k4b_scatter, dim3(nslots), dim3(256), 0, st, offsets, in_cap, kept_off, comp_off, nkept_comp, S, kept_idx,
                       cap, comp, comp_cap);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}
