// abub_match.hip -- batched bellows-veto template matcher (L3Localizer::TrackAFeature, L3Localizer.cpp:473-543):
// cv::matchTemplate(CV_TM_CCORR_NORMED) of one template against many resident frames, exact integer terms, and the
// host's bestMatchFromTerms (hostlogic.cpp) on the device, so that a job returns 8 bytes instead of 16 per placement.
//
//   k_match_num    num = sum(T*I) per placement.  v_dot4_u32_u8: a lane owns 4 adjacent placements x = 4m..4m+3 and
//                  reads ALIGNED image words I[4m + 4c ..]; placement 4m + k uses the template shifted right by k bytes
//                  (four shifted copies staged in LDS, broadcast reads), so no byte realignment is needed at all.  A wave
//                  owns MR output rows and walks the image rows once: every image word feeds 4*MR dot products.  Sums
//                  stay in u32 for at most `flushEvery` image rows (one template row adds <= 65025*tw), then widen to
//                  u64.  Small batches split the template rows over workgroups (u64 atomics, integer: exact).
//   k_match_wsum2  sum(I*I) per placement from column running sums of I*I and a per-row prefix sum (u64).
//   k_match_tnorm / k_match_norm / k_match_first / k_match_sub
//                  the CCORR_NORMED plane, its min / max, the first maximum of the min-max normalised plane, and the
//                  3x3 centre of mass -- every operation in the host's order and precision.
#include "abub_dev.hpp"

#include <float.h>

namespace {

constexpr int MR = 8;                // output rows per wave
constexpr int MWAVES = 4;            // waves per workgroup (stacked vertically, sharing the template chunk)
constexpr int MTPL = 16384 / 16;     // uint4 entries of the LDS template chunk (16 KiB)
constexpr int WS_ROWS = 8;           // output rows per workgroup of k_match_wsum2
constexpr int WS_MAXW = 4096;        // widest frame k_match_wsum2 keeps in LDS
constexpr int WS_MAXTH = 66051;      // tallest template its u32 column sums hold: 66051 * 255 * 255 < 2^32

struct MatchGeom {
    int rw, rh, nc, ybl, nsplit, rsplit, flushEvery;
    dim3 grid;
};

static MatchGeom match_geom(int W, int H, int tw, int th, int njobs)
{
    MatchGeom g;
    g.rw = W - tw + 1;
    g.rh = H - th + 1;
    g.nc = (tw + 2) / 4 + 1; // words that cover template columns up to tw - 1 under a shift of 3
    g.ybl = (g.rh + MR * MWAVES - 1) / (MR * MWAVES);
    const long long base = (long long)((g.rw + 255) / 256) * g.ybl * njobs;
    g.nsplit = 1;
    if (base < 1024)
        g.nsplit = (int)std::min<long long>((1024 + base - 1) / base, std::max(1, th / 32));
    g.rsplit = (th + g.nsplit - 1) / g.nsplit;
    g.nsplit = (th + g.rsplit - 1) / g.rsplit;
    g.flushEvery = (int)(0xffffffffull / (65025ull * (unsigned long long)tw));
    g.grid = dim3((g.rw + 255) / 256, g.ybl * g.nsplit, njobs);
    return g;
}

// bytes [o, o + 4) of a frame of n bytes as a little-endian word; bytes past the frame read as 0 (they only ever meet
// zero template bytes or placements that are discarded)
__device__ __forceinline__ uint32_t ld4(const uint8_t *__restrict__ f, size_t o, size_t n)
{
    if (o + 4 <= n) {
        uint32_t w;
        __builtin_memcpy(&w, f + o, 4);
        return w;
    }
    uint32_t w = 0;
    for (int b = 0; b < 4; ++b)
        if (o + b < n)
            w |= (uint32_t)f[o + b] << (8 * b);
    return w;
}

__device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    return a | b << 8 | c << 16 | d << 24;
}

__global__ __launch_bounds__(256) void k_match_num(const uint8_t *__restrict__ frames, int W, int H,
                                                   const uint32_t *__restrict__ fidx, const uint8_t *__restrict__ tmpl,
                                                   int tw, int th, int rw, int rh, int nc, int ybl, int rsplit,
                                                   int flushEvery, unsigned long long *__restrict__ num, int atomic)
{
    __shared__ uint4 ts[MTPL];
    const int job = blockIdx.z, yb = blockIdx.y % ybl, sp = blockIdx.y / ybl;
    const int r0 = sp * rsplit, r1 = min(th, r0 + rsplit);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y0 = (yb * MWAVES + wave) * MR;
    const int x0 = (blockIdx.x * 64 + lane) * 4;
    const size_t fbytes = (size_t)W * H;
    const uint8_t *fr = frames + (size_t)fidx[job] * fbytes;
    const int rc = max(1, MTPL / nc);
    uint32_t acc[MR][4];
    unsigned long long tot[MR][4];
#pragma unroll
    for (int j = 0; j < MR; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            acc[j][k] = 0;
            tot[j][k] = 0;
        }
    int since = 0;
    for (int ra = r0; ra < r1; ra += rc) {
        const int rb = min(r1, ra + rc);
        __syncthreads();
        // ts[(r - ra) * nc + c].{x,y,z,w} = template row r, word c, shifted right by 0, 1, 2, 3 bytes
        for (int e = threadIdx.x; e < (rb - ra) * nc; e += 256) {
            const int rr = e / nc, c = e - rr * nc;
            const uint8_t *trow = tmpl + (size_t)(ra + rr) * tw;
            uint32_t b[7];
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                const int col = 4 * c - 3 + q;
                b[q] = (col >= 0 && col < tw) ? trow[col] : 0u;
            }
            ts[e] = make_uint4(pack4(b[3], b[4], b[5], b[6]), pack4(b[2], b[3], b[4], b[5]), pack4(b[1], b[2], b[3], b[4]),
                               pack4(b[0], b[1], b[2], b[3]));
        }
        __syncthreads();
        if (y0 >= rh)
            continue;
        // image row iy meets template row r = iy - y0 - j for output row y0 + j
        for (int iy = y0 + ra; iy < y0 + rb + MR - 1; ++iy) {
            if (iy >= H)
                break; // only output rows >= rh would use it
            const int jlo = max(0, iy - y0 - (rb - 1)), jhi = min(MR - 1, iy - y0 - ra);
            const size_t ro = (size_t)iy * W + x0;
            const uint4 *tb = ts + (size_t)(iy - y0 - ra) * nc;
            if (jlo == 0 && jhi == MR - 1) {
                for (int c = 0; c < nc; ++c) {
                    const uint32_t w = ld4(fr, ro + 4 * c, fbytes);
#pragma unroll
                    for (int j = 0; j < MR; ++j) {
                        const uint4 t = tb[c - j * nc];
                        acc[j][0] = __builtin_amdgcn_udot4(w, t.x, acc[j][0], false);
                        acc[j][1] = __builtin_amdgcn_udot4(w, t.y, acc[j][1], false);
                        acc[j][2] = __builtin_amdgcn_udot4(w, t.z, acc[j][2], false);
                        acc[j][3] = __builtin_amdgcn_udot4(w, t.w, acc[j][3], false);
                    }
                }
            } else {
                for (int c = 0; c < nc; ++c) {
                    const uint32_t w = ld4(fr, ro + 4 * c, fbytes);
#pragma unroll
                    for (int j = 0; j < MR; ++j)
                        if (j >= jlo && j <= jhi) {
                            const uint4 t = tb[c - j * nc];
                            acc[j][0] = __builtin_amdgcn_udot4(w, t.x, acc[j][0], false);
                            acc[j][1] = __builtin_amdgcn_udot4(w, t.y, acc[j][1], false);
                            acc[j][2] = __builtin_amdgcn_udot4(w, t.z, acc[j][2], false);
                            acc[j][3] = __builtin_amdgcn_udot4(w, t.w, acc[j][3], false);
                        }
                }
            }
            if (++since == flushEvery) { // every accumulator took at most one template row per image row
                since = 0;
#pragma unroll
                for (int j = 0; j < MR; ++j)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        tot[j][k] += acc[j][k];
                        acc[j][k] = 0;
                    }
            }
        }
    }
    if (y0 >= rh)
        return;
#pragma unroll
    for (int j = 0; j < MR; ++j) {
        const int y = y0 + j;
        if (y >= rh)
            break;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = x0 + k;
            if (x >= rw)
                break;
            const unsigned long long v = tot[j][k] + acc[j][k];
            unsigned long long *p = num + ((size_t)job * rh + y) * rw + x;
            if (atomic)
                atomicAdd(p, v);
            else
                *p = v;
        }
    }
}

// wsum2[job][y][x] = sum over the th x tw window of I^2: column window sums cs[x] (u32: th * 65025 < 2^32 for
// th <= WS_MAXTH) slid down the rows, then per row an exclusive prefix sum P (u64) and P[x + tw] - P[x]
__global__ __launch_bounds__(256) void k_match_wsum2(const uint8_t *__restrict__ frames, int W, int H,
                                                     const uint32_t *__restrict__ fidx, int tw, int th, int rw, int rh,
                                                     unsigned long long *__restrict__ wsum2)
{
    __shared__ uint32_t cs[WS_MAXW];
    __shared__ unsigned long long P[WS_MAXW + 1];
    __shared__ unsigned long long part[256];
    const int job = blockIdx.y, y0 = blockIdx.x * WS_ROWS, t = threadIdx.x;
    const uint8_t *fr = frames + (size_t)fidx[job] * W * H;
    for (int x = t; x < W; x += 256) {
        uint32_t s = 0;
        for (int r = 0; r < th; ++r) {
            const uint32_t v = fr[(size_t)(y0 + r) * W + x];
            s += v * v;
        }
        cs[x] = s;
    }
    const int seg = (W + 255) / 256, a = min(W, t * seg), b = min(W, a + seg);
    for (int yy = 0; yy < WS_ROWS; ++yy) {
        const int y = y0 + yy;
        if (y >= rh)
            break;
        if (yy > 0)
            for (int x = t; x < W; x += 256) {
                const uint32_t vin = fr[(size_t)(y + th - 1) * W + x], vout = fr[(size_t)(y - 1) * W + x];
                cs[x] = cs[x] + vin * vin - vout * vout;
            }
        __syncthreads();
        unsigned long long s = 0;
        for (int x = a; x < b; ++x)
            s += cs[x];
        part[t] = s;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) { // inclusive scan of the 256 segment sums
            const unsigned long long v = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        s = part[t] - s; // exclusive
        if (t == 0)
            P[0] = 0;
        for (int x = a; x < b; ++x) {
            s += cs[x];
            P[x + 1] = s;
        }
        __syncthreads();
        unsigned long long *out = wsum2 + ((size_t)job * rh + y) * rw;
        for (int x = t; x < rw; x += 256)
            out[x] = P[x + tw] - P[x];
        __syncthreads();
    }
}

struct MatchStats { // per job, in the scratch buffer
    uint32_t *minKey, *maxKey, *best;
    double *tnorm;
};

// template norm the way bestMatchFromTerms derives it (integer sums are exact in any order)
__global__ __launch_bounds__(256) void k_match_tnorm(const uint8_t *__restrict__ tmpl, int n, double *__restrict__ out)
{
    __shared__ unsigned long long ss[256], qq[256];
    unsigned long long s = 0, q = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const unsigned long long v = tmpl[i];
        s += v;
        q += v * v;
    }
    ss[threadIdx.x] = s;
    qq[threadIdx.x] = q;
    __syncthreads();
    if (threadIdx.x)
        return;
    for (int i = 1; i < 256; ++i) {
        s += ss[i];
        q += qq[i];
    }
    const double N = (double)n, sum = (double)s, sq = (double)q;
    const double invArea = 1. / N, mean = sum * invArea;
    const double var = sq * invArea - mean * mean;
    const double sdv = sqrt(var > 0 ? var : 0);
    double templNorm = sqrt(sdv * sdv + mean * mean);
    templNorm /= sqrt(invArea);
    *out = templNorm;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
    for (int o = 32; o; o >>= 1)
        v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    for (int o = 32; o; o >>= 1)
        v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

// the CV_32F correlation plane (every value >= 0: its bits order like the values) and its min / max
__global__ __launch_bounds__(256) void k_match_norm(const unsigned long long *__restrict__ num,
                                                    const unsigned long long *__restrict__ wsum2, size_t n,
                                                    const double *__restrict__ tnorm, float *__restrict__ res,
                                                    uint32_t *__restrict__ minKey, uint32_t *__restrict__ maxKey)
{
    const int job = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t lo = 0xffffffffu, hi = 0;
    if (i < n) {
        const size_t o = (size_t)job * n + i;
        const double templNorm = *tnorm;
        double v = (double)(float)(double)num[o];
        const double w2 = (double)wsum2[o];
        const double lim = 10 * FLT_EPSILON * w2;
        const double t = (w2 <= (0.5 < lim ? 0.5 : lim)) ? 0 : sqrt(w2) * templNorm;
        if (fabs(v) < t)
            v /= t;
        else if (fabs(v) < t * 1.125)
            v = v > 0 ? 1 : -1;
        else
            v = 0;
        const float r = (float)v;
        res[o] = r;
        lo = hi = __float_as_uint(r);
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&minKey[job], lo);
        atomicMax(&maxKey[job], hi);
    }
}

__device__ __forceinline__ void match_scale(uint32_t lo, uint32_t hi, float &a, float &b)
{
    const double smin = (double)__uint_as_float(lo), smax = (double)__uint_as_float(hi);
    const double scale = (smax - smin > DBL_EPSILON) ? 1. / (smax - smin) : 0;
    a = (float)scale;
    b = (float)(0.0 - smin * scale);
}

// first placement (raster order) whose normalised value res*a + b equals that of the maximum (the map is monotone)
__global__ __launch_bounds__(256) void k_match_first(const float *__restrict__ res, size_t n,
                                                     const uint32_t *__restrict__ minKey, const uint32_t *__restrict__ maxKey,
                                                     uint32_t *__restrict__ best)
{
    const int job = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    float a, b;
    match_scale(minKey[job], maxKey[job], a, b);
    const float pa = __uint_as_float(maxKey[job]) * a;
    const float target = pa + b;
    uint32_t hit = 0xffffffffu;
    if (i < n) {
        const float v = res[(size_t)job * n + i] * a;
        if (v + b == target)
            hit = (uint32_t)i;
    }
    hit = wave_min(hit);
    if ((threadIdx.x & 63) == 0 && hit != 0xffffffffu)
        atomicMin(&best[job], hit);
}

// 3x3 centre of mass around the maximum, x offset outer, y offset inner, neighbours off the plane skipped
__global__ __launch_bounds__(64) void k_match_sub(const float *__restrict__ res, int rw, int rh, int njobs,
                                                  const uint32_t *__restrict__ minKey, const uint32_t *__restrict__ maxKey,
                                                  const uint32_t *__restrict__ best, float2 *__restrict__ out)
{
    const int job = blockIdx.x * 64 + threadIdx.x;
    if (job >= njobs)
        return;
    const size_t n = (size_t)rw * rh;
    float a, b;
    match_scale(minKey[job], maxKey[job], a, b);
    const uint32_t bi = best[job];
    const int mx = (int)(bi % (uint32_t)rw), my = (int)(bi / (uint32_t)rw);
    float sx = 0.f, sy = 0.f, mass = 0.f;
    for (int i = -1; i <= 1; ++i)
        for (int j = -1; j <= 1; ++j) {
            const int x = mx + i, y = my + j;
            if (x < 0 || y < 0 || x >= rw || y >= rh)
                continue;
            const float v = res[(size_t)job * n + (size_t)y * rw + x] * a;
            const float pv = v + b;
            const float px = (float)x * pv, py = (float)y * pv;
            sx = sx + px;
            sy = sy + py;
            mass = mass + pv;
        }
    const float inv = (float)(1.0 / mass);
    out[job] = make_float2(sx * inv, sy * inv);
}

// the shapes every entry admits: k_match_wsum2 keeps a frame row and u32 column sums in LDS, k_match_num one template row
// of nc words, k_match_first a u32 placement index with 0xffffffff for "none"
static bool match_shape_ok(int W, int H, int tw, int th, int njobs)
{
    return W > 0 && H > 0 && tw > 0 && th > 0 && tw <= W && th <= H && njobs > 0 && njobs <= 65535 && W <= WS_MAXW &&
           (tw + 2) / 4 + 1 <= MTPL && th <= WS_MAXTH && (H - th + 1) <= 65535 * MR * MWAVES &&
           (size_t)(W - tw + 1) * (size_t)(H - th + 1) < 0xffffffffull;
}

static bool match_args_ok(const uint8_t *frames, int W, int H, const uint32_t *fidx, int njobs, const uint8_t *tmpl,
                          int tw, int th)
{
    return frames && fidx && tmpl && match_shape_ok(W, H, tw, th, njobs);
}

static int launch_terms(const uint8_t *frames, int W, int H, const uint32_t *fidx, int njobs, const uint8_t *tmpl,
                        int tw, int th, unsigned long long *num, unsigned long long *wsum2, hipStream_t st)
{
    const MatchGeom g = match_geom(W, H, tw, th, njobs);
    if (g.flushEvery < 1 || (long long)g.ybl * g.nsplit > 65535)
        return set_err(ABUB_E_INVALID, "abub_match: template too large for the u32 accumulators");
    if (g.nsplit > 1)
        HIPCHK(hipMemsetAsync(num, 0, (size_t)njobs * g.rw * g.rh * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_match_num, g.grid, dim3(256), 0, st, frames, W, H, fidx, tmpl, tw, th, g.rw, g.rh, g.nc, g.ybl,
                       g.rsplit, g.flushEvery, num, g.nsplit > 1 ? 1 : 0);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_match_wsum2, dim3((g.rh + WS_ROWS - 1) / WS_ROWS, njobs), dim3(256), 0, st, frames, W, H, fidx,
                       tw, th, g.rw, g.rh, wsum2);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}

static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

} // namespace

extern "C" int abub_match_ccorr_batch_dev(const uint8_t *frames, int W, int H, const uint32_t *frame_idx, int njobs,
                                          const uint8_t *tmpl, int tw, int th, unsigned long long *num,
                                          unsigned long long *wsum2, void *stream)
{
    if (!match_args_ok(frames, W, H, frame_idx, njobs, tmpl, tw, th) || !num || !wsum2)
        return set_err(ABUB_E_INVALID, "abub_match_ccorr_batch_dev: bad arguments");
    return launch_terms(frames, W, H, frame_idx, njobs, tmpl, tw, th, num, wsum2, (hipStream_t)stream);
}

extern "C" size_t abub_match_best_scratch_bytes(int W, int H, int tw, int th, int njobs)
{
    if (!match_shape_ok(W, H, tw, th, njobs))
        return 0;
    const size_t n = (size_t)(W - tw + 1) * (H - th + 1) * njobs;
    return 2 * align256(n * 8) + align256(n * 4) + 3 * align256((size_t)njobs * 4) + 256;
}

extern "C" int abub_match_best_batch_dev(const uint8_t *frames, int W, int H, const uint32_t *frame_idx, int njobs,
                                         const uint8_t *tmpl, int tw, int th, float *best_xy, void *scratch,
                                         size_t scratch_bytes, void *stream)
{
    if (!match_args_ok(frames, W, H, frame_idx, njobs, tmpl, tw, th) || !best_xy || !scratch ||
        ((uintptr_t)scratch & 255) || scratch_bytes < abub_match_best_scratch_bytes(W, H, tw, th, njobs))
        return set_err(ABUB_E_INVALID, "abub_match_best_batch_dev: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int rw = W - tw + 1, rh = H - th + 1;
    const size_t n = (size_t)rw * rh, nn = n * njobs;
    uint8_t *p = (uint8_t *)scratch;
    unsigned long long *num = (unsigned long long *)p;
    p += align256(nn * 8);
    unsigned long long *w2 = (unsigned long long *)p;
    p += align256(nn * 8);
    float *res = (float *)p;
    p += align256(nn * 4);
    uint32_t *minKey = (uint32_t *)p;
    p += align256((size_t)njobs * 4);
    uint32_t *maxKey = (uint32_t *)p;
    p += align256((size_t)njobs * 4);
    uint32_t *best = (uint32_t *)p;
    p += align256((size_t)njobs * 4);
    double *tnorm = (double *)p;
    int rc = launch_terms(frames, W, H, frame_idx, njobs, tmpl, tw, th, num, w2, st);
    if (rc != ABUB_OK)
        return rc;
    HIPCHK(hipMemsetAsync(minKey, 0xff, (size_t)njobs * 4, st));
    HIPCHK(hipMemsetAsync(maxKey, 0, (size_t)njobs * 4, st));
    HIPCHK(hipMemsetAsync(best, 0xff, (size_t)njobs * 4, st));
    hipLaunchKernelGGL(k_match_tnorm, dim3(1), dim3(256), 0, st, tmpl, tw * th, tnorm);
    const dim3 pg((unsigned)((n + 255) / 256), njobs);
    hipLaunchKernelGGL(k_match_norm, pg, dim3(256), 0, st, num, w2, n, tnorm, res, minKey, maxKey);
    hipLaunchKernelGGL(k_match_first, pg, dim3(256), 0, st, res, n, minKey, maxKey, best);
    hipLaunchKernelGGL(k_match_sub, dim3((njobs + 63) / 64), dim3(64), 0, st, res, rw, rh, njobs, minKey, maxKey, best,
                       (float2 *)best_xy);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}
