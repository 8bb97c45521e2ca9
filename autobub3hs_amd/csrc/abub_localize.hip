// abub_localize.hip -- K7: what L3Localizer::LocalizeOMatic does behind findContours, on K5's polygons, for gfx950.
// K7a (k7_describe) is host/hostlogic.cpp boundingRectOf / contourAreaOf / momentsOf and host/L3Localizer.cpp describe
// (L3Localizer.cpp:401-418, 808-823); K7b (k7_localize) is CalculateInitialBubbleParams, CalculatePostTriggerFrameParams
// and isInMask (L3Localizer.cpp:215-460, 764-869, 971-1012) up to the bellows veto, which stays on the host.  Bit for bit
// the host code; built with -ffp-contract=off, hipcc's correctly rounded double divide and sqrt stay on.
//
// Why it is exact.  Every sum of K7a runs over the vertices of one polygon in their order, in one lane, with the host's
// operand types: the area in double from products of float-cast coordinates, the moments in double.  Products and sums of
// 16-bit coordinates stay far below 2^53 until the third-order terms, where the order of the additions decides the last
// bit -- hence one lane per contour and no tree.  K7b decides on integers (boxes, mask bytes) and on float comparisons of
// centroids K7a rounded once.
//
// Mapping.  K7a: one wave per slot, one lane per contour, 64 contours at a time; the vertex offset of a contour is the
// slot's pt_off plus a wave scan of the vertex counts.  K7b: one wave per stack.  The lanes go across the contours of a
// slot for the mask look-ups and the ordered compaction (ballot + mbcnt, so a list keeps the contour order); lane 0 walks
// the association of a frame's sightings with the stack's bubbles, a handful of each.  A stack's boxes and tracks go to
// shared lists; lane 0 reserves the stack's part with one atomic add per list, and the counters keep counting past the
// capacities.
#include "abub_dev.hpp"

#include <cfloat>

#define LOC_MAXC 256 /* contours per slot */
#define LOC_MAXB 32  /* bubbles per stack */
#define LOC_TRACK (ABUB_LOC_MAXTRACK + 1)

namespace {

__device__ __forceinline__ uint32_t lanes_below(unsigned long long b)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

__device__ __forceinline__ uint32_t wave_scan_incl_u32(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= d)
            v += o;
    }
    return v;
}

__device__ __forceinline__ int wave_max_i32(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// one polygon, its vertices in order (n >= 1)
__device__ __forceinline__ void describe_polygon(const uint32_t *__restrict__ p, uint32_t n, abub_contour_desc &d)
{
    const uint32_t last = p[n - 1];
    const int lx = (int)(last & 0xffffu), ly = (int)(last >> 16);
    int x0 = lx, x1 = lx, y0 = ly, y1 = ly;
    float px = (float)lx, py = (float)ly; // contourAreaOf: cv::contourArea converts the points to float
    double xp = lx, yp = ly;              // momentsOf
    double a = 0, a00 = 0, a10 = 0, a01 = 0, sx = 0, sy = 0, cnt = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t v = p[i];
        const int xi = (int)(v & 0xffffu), yi = (int)(v >> 16);
        x0 = min(x0, xi);
        x1 = max(x1, xi);
        y0 = min(y0, yi);
        y1 = max(y1, yi);
        const float qx = (float)xi, qy = (float)yi;
        a += (double)px * qy - (double)py * qx;
        px = qx;
        py = qy;
        const double x = xi, y = yi;
        const double cross = xp * y - x * yp;
        a00 += cross;
        a10 += cross * (xp + x);
        a01 += cross * (yp + y);
        xp = x;
        yp = y;
        sx += xi;
        sy += yi;
        cnt++;
    }
    d.x = x0;
    d.y = y0;
    d.w = x1 - x0 + 1;
    d.h = y1 - y0 + 1;
    d.area = fabs(a * 0.5);
    d.radius = sqrt(d.area / 3.14159);
    double m00 = 0, m10 = 0, m01 = 0;
    if (fabs(a00) > FLT_EPSILON) {
        const double half = a00 > 0 ? 0.5 : -0.5;
        const double sixth = a00 > 0 ? 0.16666666666666666666666666666667 : -0.16666666666666666666666666666667;
        m00 = a00 * half;
        m10 = a10 * sixth;
        m01 = a01 * sixth;
    }
    d.m00 = m00;
    d.m10 = m10;
    d.m01 = m01;
    d.cx = (float)(m10 / m00); // 0 / 0 = NaN stays NaN in a tracking frame
    d.cy = (float)(m01 / m00);
    if (m00 > 0) {
        d.gx = d.cx;
        d.gy = d.cy;
    } else { // degenerate polygon in the genesis frame: mean of the vertices
        d.gx = (float)(sx / cnt);
        d.gy = (float)(sy / cnt);
    }
    d.npts = n;
    d.reserved = 0;
}

__global__ __launch_bounds__(64) void k7_describe(const uint32_t *__restrict__ status, const uint32_t *__restrict__ cont_off,
                                                  const uint32_t *__restrict__ cont_npts, uint32_t cont_cap,
                                                  const uint32_t *__restrict__ pt_off, const uint32_t *__restrict__ pts,
                                                  uint32_t pts_cap, abub_contour_desc *__restrict__ desc, uint32_t desc_cap)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    if (status[s] != 0)
        return; // declined by K5: nothing was traced
    const uint32_t c0 = cont_off[s], c1 = min(cont_off[s + 1], cont_cap);
    uint32_t vbase = pt_off[s];
    for (uint32_t b = c0; b < c1; b += 64) {
        const uint32_t k = b + lane;
        const bool in = k < c1;
        const uint32_t n = in ? cont_npts[k] : 0u;
        const uint32_t incl = wave_scan_incl_u32(n, lane);
        const uint32_t v0 = vbase + (incl - n);
        vbase += (uint32_t)__shfl((int)incl, 63, 64);
        if (!in || k >= desc_cap || (unsigned long long)v0 + n > pts_cap)
            continue;
        abub_contour_desc d;
        if (n == 0) { // (K5 traces none; the host's functions answer zeros for an empty contour)
            d.x = d.y = d.w = d.h = 0;
            d.area = d.radius = d.m00 = d.m10 = d.m01 = 0;
            d.cx = d.cy = d.gx = d.gy = __builtin_nanf("");
            d.npts = 0;
            d.reserved = 0;
        } else
            describe_polygon(pts + v0, n, d);
        desc[k] = d;
    }
}

// L3Localizer::isInMask on the box of a contour; mask == nullptr: no mask dir, or the file is not loadable
__device__ __forceinline__ bool in_mask(const uint8_t *__restrict__ mask, int mw, int mh, int x, int y, int w, int h, bool bellows)
{
    const int xpix = (int)(x + w / 2.);
    const int ypix = y + h / 2;
    if (!mask)
        return !bellows;
    if (xpix < 0 || ypix < 0 || xpix >= mw || ypix >= mh)
        return false; // unchecked upstream
    return mask[(size_t)ypix * mw + xpix] > 0;
}

struct LocShared {
    uint16_t rect[LOC_MAXC];            // contours of the genesis slot that go to bubbleRects, in order
    uint8_t inBellows[LOC_MAXC];        // genesis contours dropped by the bellows mask
    uint16_t sight[LOC_MAXC];           // sightings of the current tracking frame: contour of the slot, centroid
    float sightX[LOC_MAXC], sightY[LOC_MAXC];
    uint32_t track[LOC_MAXB][LOC_TRACK]; // per bubble the records of its descriptors
    int ntr[LOC_MAXB];
    float lastX[LOC_MAXB], lastY[LOC_MAXB];
    uint8_t lock[LOC_MAXB];
    uint32_t rectOff, trackOff, ntrack;
};

__global__ __launch_bounds__(64) void k7_localize(const abub_loc_stack *__restrict__ stacks, const abub_loc_mask *__restrict__ masks,
                                                  const uint32_t *__restrict__ slot_status, const uint32_t *__restrict__ cont_off,
                                                  const abub_contour_desc *__restrict__ desc, uint32_t ndesc,
                                                  abub_loc_result *__restrict__ out, int32_t *__restrict__ rects, uint32_t rect_cap,
                                                  uint32_t *__restrict__ tracks, uint32_t track_cap, uint32_t *__restrict__ totals)
{
    __shared__ LocShared sh;
    const int lane = threadIdx.x;
    const abub_loc_stack &sd = stacks[blockIdx.x]; // (read in place: a private copy indexed by the frame would live in scratch)
    const int ntrack = min(max(sd.ntrack, 0), ABUB_LOC_MAXTRACK); // (the entry refused anything else)
    abub_loc_result res;
    res.status = ABUB_LOC_DONE;
    res.nrects = res.rect_off = res.nbubbles = res.ntrack = res.track_off = 0;
    res.reserved[0] = res.reserved[1] = 0;

    // what declines the stack before anything is decided (every lane computes the same)
    bool anySlot = false, anyIncomplete = false, anyLimit = false;
    for (int j = 0; j <= ntrack; ++j) {
        const int slot = j == 0 ? sd.genesis : sd.track[j - 1];
        const uint32_t c0 = cont_off[slot], c1 = cont_off[slot + 1];
        if (slot_status[slot] != 0)
            anySlot = true;
        else if (c1 < c0 || c1 > ndesc)
            anyIncomplete = true;
        else if (c1 - c0 > LOC_MAXC)
            anyLimit = true;
    }
    int st = ABUB_LOC_DONE;
    if (sd.bad)
        st = ABUB_LOC_BAD_FRAME;
    else if (anySlot)
        st = ABUB_LOC_SLOT;
    else if (anyIncomplete)
        st = ABUB_LOC_INCOMPLETE;
    else if (anyLimit)
        st = ABUB_LOC_LIMIT;
    if (st != ABUB_LOC_DONE) {
        res.status = st;
        if (lane == 0)
            out[blockIdx.x] = res;
        return;
    }
    const abub_loc_mask mk = masks[sd.cam];

    // ---- genesis (CalculateInitialBubbleParams) ----
    const uint32_t g0 = cont_off[sd.genesis];
    const int gn = (int)(cont_off[sd.genesis + 1] - g0);
    int largest = 0;
    bool anyOutside = false;
    for (int b = 0; b < gn; b += 64) {
        const int i = b + lane;
        bool outside = false;
        int boxArea = 0;
        if (i < gn) {
            const abub_contour_desc &d = desc[g0 + i];
            const bool inB = in_mask(mk.bel, mk.bw, mk.bh, d.x, d.y, d.w, d.h, true);
            sh.inBellows[i] = inB;
            outside = !inB;
            boxArea = outside ? d.w * d.h : 0;
        }
        anyOutside = anyOutside || __ballot(outside) != 0;
        largest = max(largest, wave_max_i32(boxArea));
    }
    if (gn > 0 && !anyOutside) { // allInBellowsMask: the veto round, or "template not loadable", is the host's
        res.status = ABUB_LOC_BELLOWS;
        if (lane == 0)
            out[blockIdx.x] = res;
        return;
    }
    int nrect = 0, nbub = 0;
    for (int b = 0; b < gn; b += 64) {
        const int i = b + lane;
        bool pass = false, starts = false;
        float gx = 0.f, gy = 0.f;
        if (i < gn && !sh.inBellows[i]) { // (written by this lane)
            const abub_contour_desc &d = desc[g0 + i];
            const int boxArea = d.w * d.h;
            pass = boxArea > 10 || boxArea >= largest;
            starts = pass && in_mask(mk.fid, mk.fw, mk.fh, d.x, d.y, d.w, d.h, false);
            gx = d.gx;
            gy = d.gy;
        }
        const unsigned long long bp = __ballot(pass), bs = __ballot(starts);
        if (pass)
            sh.rect[nrect + lanes_below(bp)] = (uint16_t)i;
        if (starts) {
            const int k = nbub + (int)lanes_below(bs);
            if (k < LOC_MAXB) { // a new bubble starts locked; the first tracking frame clears that
                sh.track[k][0] = g0 + (uint32_t)i;
                sh.ntr[k] = 1;
                sh.lastX[k] = gx;
                sh.lastY[k] = gy;
            }
        }
        nrect += __popcll(bp);
        nbub += __popcll(bs);
    }
    if (nbub > LOC_MAXB) {
        res.status = ABUB_LOC_LIMIT;
        if (lane == 0)
            out[blockIdx.x] = res;
        return;
    }
    __syncthreads();

    // ---- tracking frames in order (CalculatePostTriggerFrameParams) ----
    for (int f = 0; f < ntrack; ++f) {
        const uint32_t t0 = cont_off[sd.track[f]];
        const int tn = (int)(cont_off[sd.track[f] + 1] - t0);
        int nsight = 0;
        for (int b = 0; b < tn; b += 64) {
            const int i = b + lane;
            bool sighting = false;
            float x = 0.f, y = 0.f;
            if (i < tn) {
                const abub_contour_desc &d = desc[t0 + i];
                sighting = d.w * d.h > 10 /* kTrackMinBoxArea */ && in_mask(mk.fid, mk.fw, mk.fh, d.x, d.y, d.w, d.h, false);
                x = d.cx;
                y = d.cy;
            }
            const unsigned long long bs = __ballot(sighting);
            if (sighting) {
                const int k = nsight + (int)lanes_below(bs);
                sh.sight[k] = (uint16_t)i;
                sh.sightX[k] = x;
                sh.sightY[k] = y;
            }
            nsight += __popcll(bs);
        }
        __syncthreads();
        if (lane == 0 && nbub > 0) {
            for (int k = 0; k < nbub; ++k)
                sh.lock[k] = 0;
            // the first bubble whose last position is close enough takes the sighting; the search stops there even if
            // that bubble was already served this frame
            for (int q = 0; q < nsight; ++q) {
                const float x = sh.sightX[q], y = sh.sightY[q];
                for (int k = 0; k < nbub; ++k) {
                    const float bx = sh.lastX[k], by = sh.lastY[k];
                    if ((bx - x < 5) && (fabsf(by - y) < 5)) {
                        if (!sh.lock[k] && sh.ntr[k] < LOC_TRACK) {
                            sh.track[k][sh.ntr[k]++] = t0 + sh.sight[q];
                            sh.lastX[k] = x;
                            sh.lastY[k] = y;
                            sh.lock[k] = 1;
                        }
                        break;
                    }
                }
            }
        }
        __syncthreads();
    }

    // ---- the stack's part of the lists ----
    const uint32_t mine = lane < nbub ? (uint32_t)sh.ntr[lane] + 1u : 0u; // LOC_MAXB <= 64: one lane per bubble
    const uint32_t incl = wave_scan_incl_u32(mine, lane);
    const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
    if (lane == 0) {
        sh.rectOff = atomicAdd(&totals[0], (uint32_t)nrect);
        sh.trackOff = atomicAdd(&totals[1], total);
    }
    __syncthreads();
    const uint32_t roff = sh.rectOff, toff = sh.trackOff;
    if ((unsigned long long)roff + (uint32_t)nrect <= rect_cap)
        for (int r = lane; r < nrect; r += 64) {
            const abub_contour_desc &d = desc[g0 + sh.rect[r]];
            int32_t *o = rects + 4 * ((size_t)roff + r);
            o[0] = d.x;
            o[1] = d.y;
            o[2] = d.w;
            o[3] = d.h;
        }
    if ((unsigned long long)toff + total <= track_cap && lane < nbub) {
        uint32_t *o = tracks + (size_t)toff + (incl - mine);
        const int n = sh.ntr[lane];
        o[0] = (uint32_t)n;
        for (int j = 0; j < n; ++j)
            o[1 + j] = sh.track[lane][j];
    }
    if (lane == 0) {
        res.nrects = (uint32_t)nrect;
        res.rect_off = roff;
        res.nbubbles = (uint32_t)nbub;
        res.ntrack = total;
        res.track_off = toff;
        out[blockIdx.x] = res;
    }
}

constexpr size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

} // namespace

extern "C" int abub_describe_contours_dev(const uint32_t *status, const uint32_t *cont_off, const uint32_t *cont_npts,
                                          uint32_t cont_cap, const uint32_t *pt_off, const uint32_t *pts, uint32_t pts_cap,
                                          int nslots, abub_contour_desc *desc, uint32_t desc_cap, void *stream)
{
    static_assert(sizeof(abub_contour_desc) == 80, "record layout");
    if (!status || !cont_off || !cont_npts || !pt_off || !pts || !desc || nslots < 0 || cont_cap == 0 || pts_cap == 0 ||
        desc_cap == 0 || cont_cap > 0x7fffffffu || pts_cap > 0x7fffffffu || desc_cap > 0x7fffffffu)
        return set_err(ABUB_E_INVALID, "abub_describe_contours_dev: bad arguments");
    if (nslots == 0)
        return ABUB_OK;
    hipLaunchKernelGGL(k7_describe, dim3(nslots), dim3(64), 0, (hipStream_t)stream, status, cont_off, cont_npts, cont_cap, pt_off,
                       pts, pts_cap, desc, desc_cap);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}

extern "C" int abub_localize_limits(int *max_contours, int *max_bubbles)
{
    if (max_contours)
        *max_contours = LOC_MAXC;
    if (max_bubbles)
        *max_bubbles = LOC_MAXB;
    return ABUB_OK;
}

extern "C" size_t abub_localize_scratch_bytes(int nstacks, int ncams)
{
    if (nstacks <= 0 || ncams <= 0)
        return 0;
    return align256((size_t)nstacks * sizeof(abub_loc_stack)) + align256((size_t)ncams * sizeof(abub_loc_mask));
}

extern "C" int abub_localize_stacks_dev(const abub_loc_stack *stacks, int nstacks, const abub_loc_mask *masks, int ncams,
                                        const uint32_t *slot_status, const uint32_t *cont_off, int nslots,
                                        const abub_contour_desc *desc, uint32_t ndesc, void *scratch, size_t scratch_bytes,
                                        abub_loc_result *out, int32_t *rects, uint32_t rect_cap, uint32_t *tracks,
                                        uint32_t track_cap, uint32_t *totals, void *stream)
{
    static_assert(sizeof(abub_loc_stack) == 64 && sizeof(abub_loc_mask) == 32 && sizeof(abub_loc_result) == 32, "record layout");
    static_assert(LOC_MAXB <= 64 && LOC_MAXC <= 65536, "one lane per bubble; 16-bit contour indices");
    if (!stacks || !masks || !slot_status || !cont_off || !desc || !scratch || !out || !rects || !tracks || !totals ||
        nstacks < 0 || ncams <= 0 || nslots <= 0 || rect_cap == 0 || track_cap == 0 || rect_cap > 0x1fffffffu ||
        track_cap > 0x7fffffffu)
        return set_err(ABUB_E_INVALID, "abub_localize_stacks_dev: bad arguments");
    if (nstacks == 0)
        return ABUB_OK;
    if (((uintptr_t)scratch & 255) || scratch_bytes < abub_localize_scratch_bytes(nstacks, ncams))
        return set_err(ABUB_E_INVALID, "abub_localize_stacks_dev: descriptor scratch too small or not 256-byte aligned");
    for (int c = 0; c < ncams; ++c) {
        const abub_loc_mask &m = masks[c];
        if ((m.fid && (m.fw <= 0 || m.fh <= 0 || (size_t)m.fw * m.fh > 0x7fffffffu)) ||
            (m.bel && (m.bw <= 0 || m.bh <= 0 || (size_t)m.bw * m.bh > 0x7fffffffu)))
            return set_err(ABUB_E_INVALID, "abub_localize_stacks_dev: bad mask descriptor");
    }
    for (int s = 0; s < nstacks; ++s) {
        const abub_loc_stack &t = stacks[s];
        if (t.ntrack < 0 || t.ntrack > ABUB_LOC_MAXTRACK)
            return set_err(ABUB_E_INVALID, "abub_localize_stacks_dev: a stack has more tracking slots than ABUB_LOC_MAXTRACK");
        bool ok = t.cam >= 0 && t.cam < ncams && t.genesis >= 0 && t.genesis < nslots;
        for (int k = 0; ok && k < t.ntrack; ++k)
            ok = t.track[k] >= 0 && t.track[k] < nslots;
        if (!ok)
            return set_err(ABUB_E_INVALID, "abub_localize_stacks_dev: bad stack descriptor");
    }
    hipStream_t st = (hipStream_t)stream;
    abub_loc_stack *dst = (abub_loc_stack *)scratch;
    abub_loc_mask *dmk = (abub_loc_mask *)((uint8_t *)scratch + align256((size_t)nstacks * sizeof(abub_loc_stack)));
    HIPCHK(hipMemcpyAsync(dst, stacks, (size_t)nstacks * sizeof(abub_loc_stack), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dmk, masks, (size_t)ncams * sizeof(abub_loc_mask), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(totals, 0, 2 * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k7_localize, dim3(nstacks), dim3(64), 0, st, dst, dmk, slot_status, cont_off, desc, ndesc, out, rects,
                       rect_cap, tracks, track_cap, totals);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}
