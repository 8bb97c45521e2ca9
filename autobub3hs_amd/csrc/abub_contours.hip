// abub_contours.hip -- K5: the polygons of cv::findContours(RETR_EXTERNAL, CHAIN_APPROX_TC89_L1) from K4b's kept lists
// (gfx950).  Per slot exactly what host/hostlogic.cpp ContourFinder::find returns for the slot's kept pixels: the same
// contours in the same order (last discovered first), the same vertices in the order approxChainTC89L1 emits them
// (reference L3Localizer.cpp:264, 374, 793).
//
// One wave per slot.  The slot's sorted raster indices and one byte of marks per listed pixel live in LDS; a pixel
// lookup is a binary search in that run, so the padded plane of the host never exists.  The raster scan of the host is a
// walk over the list: each listed pixel, plus the one empty position behind the end of each run (further empty pixels
// change no state).  Border following probes the up-to-16 neighbour positions of one step with 16 lanes and a ballot
// picks the first hit.  The chain and its points go to LDS; Teh-Chin's support regions are independent per chain
// position and go across the lanes, the suppression and clean-up passes modify the list in list order and run on lane 0.
//
// Output offsets need the counts of every slot, and a slot's contours come out in reverse discovery order, so the kernel
// runs twice: pass 1 counts (and leaves each contour's vertex count in the scratch), k5_scan makes the offsets, pass 2
// traces again and writes every vertex at its final place.  Both passes do the same integer work: deterministic.
//
// A slot with more than K5_MAX_PIX pixels, or with a chain of more than K5_MAX_CHAIN codes, is declined (status 1, no
// contour): the caller traces it on the host from its kept pixels.
#include "abub_dev.hpp"

#define K5_MAX_PIX 2048   /* = K4B_LDS_N of abub_blobs.hip */
#define K5_MAX_CHAIN 1024 /* Freeman codes of one border */
#define K5_NODES (K5_MAX_CHAIN + 8)

struct K5Lds {
    uint32_t key[K5_MAX_PIX];  // raster indices, increasing
    uint32_t pt[K5_NODES];     // x | y << 16 of chain position i (Node::pt)
    int16_t next[K5_NODES];    // Node::next; the list head is node len + 7 as on the host
    uint16_t kk[K5_NODES];     // Node::k
    uint8_t sv[K5_NODES];      // Node::s
    uint8_t code[K5_MAX_CHAIN];
    uint8_t mark[K5_MAX_PIX];  // 1, 2 or 2|-128, the plane values of the listed pixels
};

__device__ __forceinline__ int k5_dx(int d) { return ((0x901A >> (2 * d)) & 3) - 1; } // {1,1,0,-1,-1,-1,0,1}
__device__ __forceinline__ int k5_dy(int d) { return ((0xA901 >> (2 * d)) & 3) - 1; } // {0,-1,-1,-1,0,1,1,1}
__device__ __forceinline__ int k5_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// position of pixel (x, y) in key[0 .. n), -1 when it is not listed or outside the frame.  x and y are tested against the
// frame: (W-1, y) and (0, y+1) are adjacent raster indices and no neighbours.
__device__ __forceinline__ int k5_lookup(const uint32_t *key, int n, int x, int y, int W, int H)
{
    if (x < 0 || y < 0 || x >= W || y >= H)
        return -1;
    const uint32_t q = (uint32_t)y * (uint32_t)W + (uint32_t)x;
    int a = 0, b = n;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (key[m] < q)
            a = m + 1;
        else
            b = m;
    }
    return (a < n && key[a] == q) ? a : -1;
}

// ContourFinder::traceBorder from list position `start`: codes and points to LDS, marks updated.  Returns the chain
// length (0: isolated pixel), -1 when the chain would exceed K5_MAX_CHAIN.  Wave-uniform control flow.
__device__ int k5_trace(K5Lds &L, int n, int W, int H, int start, int lane)
{
    const uint32_t k0 = L.key[start];
    const int x0 = k5_uni((int)(k0 % (uint32_t)W)), y0 = k5_uni((int)(k0 / (uint32_t)W));
    int s, p1;
    {
        // clockwise from NW to SW: s = 3, 2, 1, 0, 7, 6, 5
        const int d = (3 - lane) & 7;
        int pos = -1;
        if (lane < 7)
            pos = k5_lookup(L.key, n, x0 + k5_dx(d), y0 + k5_dy(d), W, H);
        const unsigned long long hit = __ballot(pos >= 0);
        if (hit == 0) {
            if (lane == 0)
                L.mark[start] = (uint8_t)0x82;
            return 0;
        }
        const int j = __ffsll((long long)hit) - 1;
        s = (3 - j) & 7;
        p1 = k5_uni(__shfl(pos, j));
    }
    int p3 = start, x3 = x0, y3 = y0, cnt = 0;
    for (;;) {
        const int sEnd = s;
        const int sj = s + 1 + lane, d = sj & 7;
        int pos = -1;
        if (sj <= 15)
            pos = k5_lookup(L.key, n, x3 + k5_dx(d), y3 + k5_dy(d), W, H);
        const unsigned long long hit = __ballot(pos >= 0);
        if (hit == 0) // (cannot happen: the pixel the step came from is among the probes)
            return cnt;
        const int j = __ffsll((long long)hit) - 1;
        const int p4 = k5_uni(__shfl(pos, j));
        s = (s + 1 + j) & 7;
        if (cnt >= K5_MAX_CHAIN)
            return -1;
        if (lane == 0) {
            if ((unsigned)(s - 1) < (unsigned)sEnd)
                L.mark[p3] = (uint8_t)0x82;
            else if (L.mark[p3] == 1)
                L.mark[p3] = 2;
            L.code[cnt] = (uint8_t)s;
            L.pt[cnt] = (uint32_t)x3 | ((uint32_t)y3 << 16);
        }
        ++cnt;
        if (p4 == start && p3 == p1)
            break;
        p3 = p4;
        x3 += k5_dx(s);
        y3 += k5_dy(s);
        s = (s + 4) & 7;
    }
    return cnt;
}

// approxChainTC89L1 on the chain in LDS.  Returns the number of vertices; with WRITE they go to out[0 ..) as far as `room`
// allows.  Called by the whole wave.
template <bool WRITE>
__device__ uint32_t k5_approx(K5Lds &L, int len, uint32_t origin, int lane, uint32_t *__restrict__ out, uint32_t room)
{
    if (len == 0) {
        if (WRITE && lane == 0 && room > 0)
            out[0] = origin;
        return 1;
    }
    const int HEAD = len + 7;
    // Node::s and Node::k
    for (int i = lane; i < len; i += 64) {
        const int c = L.code[i], pc = L.code[i == 0 ? len - 1 : i - 1];
        int t = c - pc;
        t = t < 0 ? -t : t;
        L.sv[i] = (uint8_t)(t <= 4 ? t : 8 - t);
        L.kk[i] = 0;
    }
    __syncthreads();
    // the list of the positions with s != 0, in chain order
    int carry = -1;
    for (int c = (len + 63) / 64 - 1; c >= 0; --c) {
        const int i = c * 64 + lane;
        const bool nz = i < len && L.sv[i] != 0;
        const unsigned long long mask = __ballot(nz);
        const unsigned long long higher = lane == 63 ? 0ull : (mask & (~0ull << (lane + 1)));
        if (i < len)
            L.next[i] = (int16_t)(nz ? (higher ? c * 64 + __ffsll((long long)higher) - 1 : carry) : -1);
        if (mask)
            carry = c * 64 + __ffsll((long long)mask) - 1;
    }
    if (carry < 0) {
        if (WRITE && lane == 0 && room > 0)
            out[0] = origin;
        return 1;
    }
    if (lane == 0)
        L.next[HEAD] = (int16_t)carry;
    __syncthreads();
    // support regions
    for (int cur = lane; cur < len; cur += 64) {
        if (L.sv[cur] == 0)
            continue;
        const uint32_t q0 = L.pt[cur];
        const int p0x = (int)(q0 & 0xffff), p0y = (int)(q0 >> 16);
        int k, l = 0, dNum = 0;
        for (k = 1;; ++k) {
            int i1 = cur - k, i2 = cur + k;
            i1 = i1 < 0 ? i1 + len : i1;
            i2 = i2 >= len ? i2 - len : i2;
            const uint32_t q1 = L.pt[i1], q2 = L.pt[i2];
            const int x1 = (int)(q1 & 0xffff), y1 = (int)(q1 >> 16), x2 = (int)(q2 & 0xffff), y2 = (int)(q2 >> 16);
            const int dx = x2 - x1, dy = y2 - y1;
            const int lk = dx * dx + dy * dy;
            const int dkNum = (p0x - x1) * dy - (p0y - y1) * dx;
            const float d = (float)(((double)dNum) * lk - ((double)dkNum) * l);
            const int32_t bits = __float_as_int(d);
            if (k > 1 && (l >= lk || (dNum > 0 && bits <= 0) || (dNum < 0 && bits >= 0)))
                break;
            dNum = dkNum;
            l = lk;
            if (k >= len) {
                ++k;
                break;
            }
        }
        L.kk[cur] = (uint16_t)(k - 1);
    }
    __syncthreads();
    uint32_t nout = 0;
    if (lane == 0) {
        auto wrapDown = [len](int i) { return i < 0 ? i + len : i; };
        auto wrapUp = [len](int i) { return i >= len ? i - len : i; };
        // non-maxima suppression inside half the support region
        for (int prev = HEAD, cur = L.next[HEAD]; cur >= 0;) {
            const int half = L.kk[cur] >> 1, s = L.sv[cur];
            int j = 1;
            for (; j <= half; ++j) {
                if (L.sv[wrapDown(cur - j)] > s)
                    break;
                if (L.sv[wrapUp(cur + j)] > s)
                    break;
            }
            const int nxt = L.next[cur];
            if (j <= half) {
                L.next[prev] = (int16_t)nxt;
                L.sv[cur] = 0;
            } else
                prev = cur;
            cur = nxt;
        }
        // drop weak points whose support region has length one
        for (int prev = HEAD, cur = L.next[HEAD]; cur >= 0;) {
            const int nxt = L.next[cur];
            bool drop = false;
            if (L.kk[cur] == 1) {
                const int s = L.sv[cur];
                drop = s <= L.sv[wrapDown(cur - 1)] || s <= L.sv[wrapUp(cur + 1)];
            }
            if (drop) {
                L.next[prev] = (int16_t)nxt;
                L.sv[cur] = 0;
            } else
                prev = cur;
            cur = nxt;
        }
        // clean runs of adjacent survivors (L1 variant)
        bool allSurvived = false;
        if (L.sv[0] != 0 && L.sv[len - 1] != 0) { // a run wraps around the start of the chain
            int i1 = 1;
            for (; i1 < len && L.sv[i1] != 0; ++i1)
                L.sv[i1 - 1] = 0;
            if (i1 == len)
                allSurvived = true;
            else {
                --i1;
                int i2 = len - 2;
                for (; i2 > 0 && L.sv[i2] != 0; --i2) {
                    L.next[i2] = -1;
                    L.sv[i2 + 1] = 0;
                }
                ++i2;
                if (i1 == 0 && i2 == len - 1) { // only two points in the run
                    i1 = L.next[0];
                    L.pt[len] = L.pt[0];
                    L.kk[len] = L.kk[0];
                    L.sv[len] = L.sv[0];
                    L.next[len] = -1;
                    L.next[len - 1] = (int16_t)len;
                }
                L.next[HEAD] = (int16_t)i1;
            }
        }
        if (!allSurvived) {
            int first = HEAD, prev = HEAD, run = 1;
            for (int cur = L.next[HEAD]; cur >= 0;) {
                const int nxt = L.next[cur];
                if (nxt < 0 || nxt - cur != 1) {
                    if (run >= 2) {
                        if (run == 2) {
                            const int s1 = L.sv[prev], s2 = L.sv[cur];
                            if (s1 > s2 || (s1 == s2 && L.kk[prev] <= L.kk[cur]))
                                L.next[prev] = (int16_t)nxt; // second of the couple goes
                            else
                                L.next[first] = (int16_t)cur; // first of the couple goes
                        } else
                            L.next[L.next[first]] = (int16_t)cur; // keep only the ends of a longer run
                    }
                    first = cur;
                    run = 1;
                } else
                    ++run;
                prev = cur;
                cur = nxt;
            }
        }
        for (int cur = L.next[HEAD]; cur >= 0; cur = L.next[cur]) {
            if (WRITE && nout < room)
                out[nout] = L.pt[cur];
            ++nout;
        }
    }
    __syncthreads();
    return (uint32_t)k5_uni((int)nout);
}

// scratch: contour vertex counts in discovery order [in_cap] (slot s owns [kept_off[s], kept_off[s+1]): a slot has at
// most one contour per pixel), vertices per slot [nslots]
struct K5Scratch {
    uint32_t *cstage, *tot;
};
static size_t k5_align(size_t b) { return (b + 255) & ~(size_t)255; }
static size_t k5_layout(int nslots, uint32_t in_cap, char *base, K5Scratch *o)
{
    const size_t a = k5_align((size_t)in_cap * 4), b = k5_align((size_t)nslots * 4);
    if (o) {
        o->cstage = (uint32_t *)base;
        o->tot = (uint32_t *)(base + a);
    }
    return a + b;
}

template <bool WRITE>
__global__ __launch_bounds__(64) void k5_trace_slots(const uint32_t *__restrict__ kept_off, const uint32_t *__restrict__ kept_idx,
                                                     uint32_t in_cap, int W, int H, uint32_t *__restrict__ status,
                                                     uint32_t *__restrict__ ncont, const uint32_t *__restrict__ cont_off,
                                                     uint32_t *__restrict__ cont_npts, uint32_t cont_cap,
                                                     const uint32_t *__restrict__ pt_off, uint32_t *__restrict__ pts,
                                                     uint32_t pts_cap, K5Scratch S)
{
    __shared__ K5Lds L;
    const int s = blockIdx.x, lane = threadIdx.x;
    uint32_t o0 = kept_off[s], o1 = kept_off[s + 1];
    o0 = o0 < in_cap ? o0 : in_cap; // an overflowed list: read only what was written (the caller redoes the batch)
    o1 = o1 < in_cap ? o1 : in_cap;
    o1 = o1 > o0 ? o1 : o0;
    const uint32_t npix = o1 - o0;
    if (WRITE) {
        if (status[s] != 0)
            return;
    } else if (npix > K5_MAX_PIX) {
        if (lane == 0) {
            status[s] = 1;
            ncont[s] = 0;
            S.tot[s] = 0;
        }
        return;
    }
    const int n = (int)npix;
    for (int i = lane; i < n; i += 64) {
        L.key[i] = kept_idx[o0 + i];
        L.mark[i] = 1;
    }
    __syncthreads();
    const uint32_t nc_all = WRITE ? ncont[s] : 0u, tot_all = WRITE ? S.tot[s] : 0u;
    const uint32_t cbase = WRITE ? cont_off[s] : 0u, pbase = WRITE ? pt_off[s] : 0u;
    uint32_t found = 0, cum = 0;
    bool declined = false;
    // the raster scan of ContourFinder::find as a walk over the list
    int prev = 0, lnbd = -1, lastx = -2, lasty = -1;
    for (int i = 0; i < n; ++i) {
        const uint32_t k = (uint32_t)k5_uni((int)L.key[i]);
        const int x = (int)(k % (uint32_t)W), y = (int)(k / (uint32_t)W);
        if (y != lasty) {
            prev = 0;
            lnbd = -1;
        } else if (x != lastx + 1) { // the empty position behind the previous run
            if (prev >= 1 && (prev & -2))
                lnbd = i - 1;
            prev = 0;
        }
        lastx = x;
        lasty = y;
        int p = (int)(signed char)k5_uni((int)L.mark[i]);
        if (p == prev)
            continue;
        if (prev == 0 && p == 1) {
            const bool inside = lnbd >= 0 && (signed char)k5_uni((int)L.mark[lnbd]) > 0;
            if (!inside) { // not inside an already traced outer border
                const int len = k5_trace(L, n, W, H, i, lane);
                if (len < 0) {
                    declined = true;
                    break;
                }
                __syncthreads();
                uint32_t *out = nullptr;
                uint32_t room = 0;
                if (WRITE) {
                    const uint32_t nd = S.cstage[o0 + found];
                    cum += nd;
                    const uint32_t at = pbase + (tot_all - cum); // later contours come first
                    if (at < pts_cap) {
                        out = pts + at;
                        room = pts_cap - at;
                    }
                    const uint32_t ci = cbase + (nc_all - 1u - found);
                    if (lane == 0 && found < nc_all && ci < cont_cap)
                        cont_npts[ci] = nd;
                }
                const uint32_t nv = k5_approx<WRITE>(L, len, (uint32_t)x | ((uint32_t)y << 16), lane, out, room);
                if (!WRITE) {
                    if (lane == 0)
                        S.cstage[o0 + found] = nv; // (found < n: every trace starts at another pixel)
                    cum += nv;
                }
                ++found;
                __syncthreads();
                p = (int)(signed char)k5_uni((int)L.mark[i]);
            }
        }
        prev = p;
        if (prev & -2)
            lnbd = i;
    }
    if (!WRITE && lane == 0) {
        status[s] = declined ? 1u : 0u;
        ncont[s] = declined ? 0u : found;
        S.tot[s] = declined ? 0u : cum;
    }
}

// single block: cont_off / pt_off = exclusive scans of the per-slot counts, and the four statistics
__global__ __launch_bounds__(1024) void k5_scan(const uint32_t *__restrict__ status, const uint32_t *__restrict__ ncont,
                                                const uint32_t *__restrict__ tot, uint32_t nslots, uint32_t *__restrict__ cont_off,
                                                uint32_t *__restrict__ pt_off, uint32_t *__restrict__ stats)
{
    __shared__ uint32_t wa[16], wb[16], wc[16];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6, per = (nslots + 1023) / 1024;
    const uint32_t lo = t * per < nslots ? t * per : nslots, hi = lo + per < nslots ? lo + per : nslots;
    uint32_t a = 0, b = 0, c = 0;
    for (uint32_t i = lo; i < hi; ++i) {
        a += ncont[i];
        b += tot[i];
        c += status[i] != 0;
    }
    uint32_t ia = a, ib = b, ic = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t xa = __shfl_up(ia, o), xb = __shfl_up(ib, o), xc = __shfl_up(ic, o);
        if (lane >= (uint32_t)o) {
            ia += xa;
            ib += xb;
            ic += xc;
        }
    }
    if (lane == 63) {
        wa[w] = ia;
        wb[w] = ib;
        wc[w] = ic;
    }
    __syncthreads();
    uint32_t pa = ia - a, pb = ib - b, ta = 0, tb = 0, tc = 0;
    for (uint32_t k = 0; k < 16; ++k) {
        if (k < w) {
            pa += wa[k];
            pb += wb[k];
        }
        ta += wa[k];
        tb += wb[k];
        tc += wc[k];
    }
    for (uint32_t i = lo; i < hi; ++i) {
        cont_off[i] = pa;
        pt_off[i] = pb;
        pa += ncont[i];
        pb += tot[i];
    }
    if (t == 0) {
        cont_off[nslots] = ta;
        pt_off[nslots] = tb;
        stats[0] = nslots - tc;
        stats[1] = tc;
        stats[2] = ta;
        stats[3] = tb;
    }
}

extern "C" int abub_trace_contours_limits(int *max_pixels, int *max_chain)
{
    if (max_pixels)
        *max_pixels = K5_MAX_PIX;
    if (max_chain)
        *max_chain = K5_MAX_CHAIN;
    return ABUB_OK;
}

extern "C" size_t abub_trace_contours_scratch_bytes(int nslots, uint32_t in_cap)
{
    if (nslots <= 0 || in_cap == 0)
        return 0;
    return k5_layout(nslots, in_cap, nullptr, nullptr);
}

extern "C" int abub_trace_contours_dev(const uint32_t *kept_off, const uint32_t *kept_idx, uint32_t in_cap, int nslots, int W,
                                       int H, uint32_t *status, uint32_t *ncont, uint32_t *cont_off, uint32_t *cont_npts,
                                       uint32_t cont_cap, uint32_t *pt_off, uint32_t *pts, uint32_t pts_cap, uint32_t *stats,
                                       void *scratch, size_t scratch_bytes, void *stream)
{
    if (!kept_off || !kept_idx || !status || !ncont || !cont_off || !cont_npts || !pt_off || !pts || !stats || !scratch ||
        nslots <= 0 || W <= 0 || H <= 0 || W > 65535 || H > 65535 || in_cap == 0 || cont_cap == 0 || pts_cap == 0)
        return set_err(ABUB_E_INVALID, "abub_trace_contours_dev: bad arguments");
    const size_t need = abub_trace_contours_scratch_bytes(nslots, in_cap);
    if (need == 0 || scratch_bytes < need || ((uintptr_t)scratch & 255))
        return set_err(ABUB_E_INVALID, "abub_trace_contours_dev: scratch too small or not 256-byte aligned");
    K5Scratch S;
    k5_layout(nslots, in_cap, (char *)scratch, &S);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k5_trace_slots<false>, dim3(nslots), dim3(64), 0, st, kept_off, kept_idx, in_cap, W, H, status, ncont,
                       (const uint32_t *)cont_off, cont_npts, cont_cap, (const uint32_t *)pt_off, pts, pts_cap, S);
    hipLaunchKernelGGL(k5_scan, dim3(1), dim3(1024), 0, st, (const uint32_t *)status, (const uint32_t *)ncont,
                       (const uint32_t *)S.tot, (uint32_t)nslots, cont_off, pt_off, stats);
    hipLaunchKernelGGL(k5_trace_slots<true>, dim3(nslots), dim3(64), 0, st, kept_off, kept_idx, in_cap, W, H, status, ncont,
                       (const uint32_t *)cont_off, cont_npts, cont_cap, (const uint32_t *)pt_off, pts, pts_cap, S);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}
