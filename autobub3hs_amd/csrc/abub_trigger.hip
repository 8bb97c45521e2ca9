// abub_trigger.hip -- K6: the trigger-frame search of AnalyzerUnit::FindTriggerFrame (AnalyzerUnit.cpp:119-324) with
// calculateSignificanceFrame (:435-504) and CalcMean / CalcStdDev (:514-532) on finished histograms, for gfx950.  Bit for
// bit host/AnalyzerUnit.cpp FindTriggerFrame + host/hostlogic.cpp significanceFromHist; built with -ffp-contract=off.
//
// Why frames are independent.  The search stores every main-loop frame and a retry continues behind the trigger without
// clearing, so the history seen at main-loop frame i is always the pushed counts of frames 1 .. i, and a look-ahead at
// i + 1 / i + 2 (store = false) sees that same history with n0 = i.  A frame pushes the bins up to the one at which its
// `remaining` runs out; a bin it did not push adds nothing to either sum.  The sums are of integers far below 2^53:
//   mean = (double)S / n0,  sd = sqrt((double)S2 / n0 - mean * mean),  S = sum of counts,  S2 = sum of the 32-bit wrapped squares
// so S and S2 are int64 prefix sums over the frames.  What stays serial is the clamp recurrence over the bins of one
// frame (sig = max(0, sig + term), double, not associative) and the trivial state machine over the frames.
//
// Mapping: one wave per stack, one frame per lane, 64-frame tiles with the prefix sums carried in LDS.  A tile's histograms
// are staged through LDS in chunks of 64 bins (one coalesced 256-byte row load per frame; pitch 65 dwords, so the per-bin
// column read has no bank conflict); per bin one wave-wide inclusive scan of S and S2; each lane runs its own clamp loop.
// Lane j evaluates frame j three ways: against history j (main loop), j - 1 (first look-ahead of main frame j - 1) and
// j - 2 (second look-ahead of main frame j - 2).  Pass 0 computes the main values of every frame; pass 1 runs only when
// some frame's main value exceeds the threshold, and only the lanes behind such a frame do its double arithmetic.
// A chunk is skipped once every lane's `remaining` has run out, which real histograms reach within the first chunk.
#include "abub_dev.hpp"

#define TRIG_MAXF 512  /* frames per stack (LDS: 26 bytes per frame of results + 8 of row pointers) */
#define TRIG_MAXSEG 32 /* segments per stack (BatchEventData::MAXB) */
#define TRIG_BC 64     /* bins per staged chunk */
#define TRIG_PITCH 65  /* dwords per staged row */

namespace {

struct TrigShared {
    uint32_t tile[64 * TRIG_PITCH];       // [frame of the tile][bin of the chunk]
    long long baseS[256], baseS2[256];    // prefix sums at the end of the previous tile, per bin
    int prevM[256];                       // pushed count of the previous tile's last frame (history j - 2 of lane 0)
    long long prevQ[256];                 // ... and its wrapped square
    const uint32_t *row[TRIG_MAXF];       // histogram of frame j (NULL: not readable)
    double sig[3][TRIG_MAXF];             // significance of frame j against history j, j - 1, j - 2
    int8_t loc[TRIG_MAXF];                // loc_thres after the store = true evaluation of frame j
    uint8_t rd[TRIG_MAXF];                // 0 readable, 1 no segment covers it, 2 covered but pending
};

// one bin of significanceFromHist: the term of `count` against a history with sums S, S2 over n0 frames, then the clamp
__device__ __forceinline__ double trig_term(double sig, float count, long long S, long long S2, int n0)
{
    const double mean = (double)S / n0;
    const double sd = sqrt((double)S2 / n0 - mean * mean);
    if ((double)count != mean || sd > 0)
        sig += ((double)count - mean) / sd;
    if (sig < 0)
        sig = 0;
    return sig;
}

__device__ __forceinline__ long long wave_scan_incl(long long v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(v, d, 64);
        if (lane >= d)
            v += o;
    }
    return v;
}

// PASS 0: main values and loc_thres of frames 1 .. nf - 1.  PASS 1: the look-ahead values of the frames that need them.
template <int PASS>
__device__ __forceinline__ void trig_pass(TrigShared &sh, int nf, int P, int tss, int n, float thr, int lane)
{
    for (int b = lane; b < 256; b += 64) {
        sh.baseS[b] = 0;
        sh.baseS2[b] = 0;
        sh.prevM[b] = 0;
        sh.prevQ[b] = 0;
    }
    __syncthreads();
    for (int base = 1; base < nf; base += 64) {
        const int j = base + lane;
        const bool active = j < nf;
        bool need1 = false, need2 = false;
        if (PASS == 1) {
            // main frame i is a candidate when its value exceeds the threshold (FindTriggerFrame's test)
            if (active && j - 1 >= 2 && j - 1 != n - 1)
                need1 = (float)sh.sig[0][j - 1] > thr;
            if (active && j - 2 >= 2)
                need2 = (float)sh.sig[0][j - 2] > thr;
        }
        int rem = P, firstOver = -1, lastbin = 0;
        double s0 = 0, s1 = 0, s2 = 0;
        bool done = !active || rem <= 0;
        int visited = 0; // bins this tile went through (wave-uniform)
        for (int cb = 0; cb < 256 / TRIG_BC; ++cb) {
            if (__ballot(!done) == 0)
                break;
            __syncthreads(); // the previous chunk's reads are over
#pragma unroll 8
            for (int r = 0; r < 64; ++r) {
                const uint32_t *p = base + r < nf ? sh.row[base + r] : nullptr;
                sh.tile[r * TRIG_PITCH + lane] = p ? p[cb * TRIG_BC + lane] : 0u;
            }
            __syncthreads();
            for (int bb = 0; bb < TRIG_BC; ++bb) {
                if (__ballot(!done) == 0)
                    break;
                const int bin = cb * TRIG_BC + bb;
                visited = bin + 1;
                const bool live = !done;
                const float count = live ? (float)sh.tile[lane * TRIG_PITCH + bb] : 0.f; // cv::calcHist output is CV_32F
                const int ci = (int)count;                                               // what the frame pushes
                const long long m = ci, q = (long long)(int)((unsigned)ci * (unsigned)ci);
                const long long S = sh.baseS[bin] + wave_scan_incl(m, lane);
                const long long S2 = sh.baseS2[bin] + wave_scan_incl(q, lane);
                long long mp = __shfl_up(m, 1, 64), qp = __shfl_up(q, 1, 64);
                if (lane == 0) {
                    mp = sh.prevM[bin];
                    qp = sh.prevQ[bin];
                }
                if (lane == 63) { // (read above by every lane before this store: one wave, program order)
                    sh.baseS[bin] = S;
                    sh.baseS2[bin] = S2;
                    sh.prevM[bin] = ci;
                    sh.prevQ[bin] = q;
                }
                if (live) {
                    if (bin > 1) {
                        if (PASS == 0)
                            s0 = trig_term(s0, count, S, S2, j);
                        else {
                            if (need1)
                                s1 = trig_term(s1, count, S - m, S2 - q, j - 1);
                            if (need2)
                                s2 = trig_term(s2, count, S - m - mp, S2 - q - qp, j - 2);
                        }
                    }
                    if (PASS == 0) {
                        if (s0 > 3.5 && firstOver < 0)
                            firstOver = bin;
                        lastbin = bin; // maxAdc
                    }
                    rem = (int)((float)rem - count);
                    done = rem <= 0;
                }
            }
        }
        for (int b = visited + lane; b < 256; b += 64) { // bins the tile's last frame did not push
            sh.prevM[b] = 0;
            sh.prevQ[b] = 0;
        }
        if (active) {
            if (PASS == 0) {
                int t = max(firstOver - 1, lastbin - 1);
                if (t < 2)
                    t = 2;
                if (t > 3 || tss < 6) // loc_thres_max = 3
                    t = 3;
                sh.sig[0][j] = s0;
                sh.loc[j] = (int8_t)t;
            } else {
                sh.sig[1][j] = s1;
                sh.sig[2][j] = s2;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_trigger_search(const abub_trig_stack *__restrict__ stacks,
                                                       const abub_trig_seg *__restrict__ segs, int nsegs, int P,
                                                       abub_trig_result *__restrict__ out, double *__restrict__ sig_main,
                                                       int sig_pitch)
{
    __shared__ TrigShared sh;
    const int lane = threadIdx.x;
    const abub_trig_stack sd = stacks[blockIdx.x];
    const int n = min(max(sd.F, 0), TRIG_MAXF); // (the entry refused anything larger)
    abub_trig_result res;
    res.state = ABUB_TRIG_DONE;
    res.status = -3;
    res.trig = 0;
    res.loc_thres = -1;
    res.need_frame = 0;
    res.evaluated = 0;
    res.sig = 0.f;
    res.reserved = 0;
    if (n < 5) { // malformed sequence
        res.status = -9;
        if (lane == 0)
            out[blockIdx.x] = res;
        return;
    }
    const int start = max(sd.start, 1), tss = sd.tss;
    const int firstBad = min(max(sd.first_bad, 0), n);
    float thr = 3.5f;
    if (tss < 6)
        thr = (float)((double)thr * (5 / 3.5)); // `entropyThreshold *= 5 / 3.5` on a float

    // which frames can be read
    for (int j = lane; j < n; j += 64) {
        sh.rd[j] = 1;
        sh.row[j] = nullptr;
    }
    __syncthreads();
    const uint32_t seg1 = min(sd.seg0 + min(sd.nseg, (uint32_t)TRIG_MAXSEG), (uint32_t)nsegs);
    for (uint32_t k = sd.seg0; k < seg1; ++k) {
        const abub_trig_seg sg = segs[k];
        for (int q = lane; q < sg.count; q += 64) {
            const int j = sg.first + q;
            if (j < 1 || j >= n || j >= firstBad || !sg.hist)
                continue;
            const bool pend = sg.pending && sg.pending[q];
            sh.rd[j] = pend ? 2 : 0;
            sh.row[j] = pend ? nullptr : sg.hist + (size_t)q * 256;
        }
    }
    __syncthreads();
    // The search touches frames in rising order (a look-ahead reaches at most two frames past the main loop), and the
    // history of a frame is every frame before it: so the first frame it cannot read is the lowest unreadable one, and
    // nothing behind that frame, or at or behind the first undecodable one, is ever evaluated.
    int u = n;
    for (int b0 = 1; b0 < n && u == n; b0 += 64) {
        const int j = b0 + lane;
        const unsigned long long bad = __ballot(j < n && j < firstBad && sh.rd[j] != 0);
        if (bad)
            u = b0 + __ffsll((long long)bad) - 1;
    }
    const int nf = min(u, max(firstBad, 1));

    trig_pass<0>(sh, nf, P, tss, n, thr, lane);
    bool any = false;
    for (int b0 = 2; b0 < nf; b0 += 64) {
        const int i = b0 + lane;
        any = any || __ballot(i < nf && i != n - 1 && (float)sh.sig[0][i] > thr) != 0;
    }
    if (any)
        trig_pass<1>(sh, nf, P, tss, n, thr, lane);
    if (lane != 0)
        return;

    // ---- FindTriggerFrame's state machine (one lane; a handful of double operations per candidate frame) ----
    auto needs = [&](int frame) {
        res.state = sh.rd[frame] == 2 ? ABUB_TRIG_NEED_FINAL : ABUB_TRIG_NEED_FRAMES;
        res.status = -3;
        res.trig = 0;
        res.loc_thres = -1;
        res.need_frame = frame;
        res.evaluated = 0;
        res.sig = 0.f;
    };
    double *sm = sig_main ? sig_main + (size_t)blockIdx.x * sig_pitch : nullptr;
    bool stop = false;
    if (u < n && u < start) { // a frame of the history itself
        needs(u);
        stop = true;
    }
    for (int i = start; i < n && !stop; ++i) {
        if (i >= firstBad) { // Parser::GetImage == -1 on the frame under evaluation
            res.status = -9;
            break;
        }
        if (i >= u) {
            needs(i);
            break;
        }
        float single = (float)sh.sig[0][i];
        res.loc_thres = sh.loc[i];
        res.sig = single;
        ++res.evaluated;
        if (single > thr && i >= 2 && i != n - 1) {
            double maxSoFar = single;
            for (int ii = 1; ii <= 2 && ii + i < n; ++ii) {
                if (i + ii >= firstBad) {
                    res.state = ABUB_TRIG_BAD_LOOKAHEAD;
                    stop = true;
                    break;
                }
                if (i + ii >= u) {
                    needs(i + ii);
                    stop = true;
                    break;
                }
                single = (float)sh.sig[ii][i + ii];
                if (single / (thr / 3.5 * 5) + single / maxSoFar <= 3)
                    break;
                else if (ii == 2) {
                    res.status = 0;
                    res.trig = i;
                }
                if (single > maxSoFar)
                    maxSoFar = single;
            }
            if (res.status == 0)
                break;
        }
    }
    // the main-loop values of a search that ran to its end (a search that needs frames reports nothing else)
    for (int i = start; sm && i < start + res.evaluated && i < sig_pitch; ++i)
        sm[i] = sh.sig[0][i];
    out[blockIdx.x] = res;
}

// pending[j] = 0 where done[j] != 0
__global__ __launch_bounds__(256) void k_trigger_clear_pending(uint8_t *__restrict__ pending, const uint8_t *__restrict__ done, size_t n)
{
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j < n && done[j])
        pending[j] = 0;
}

} // namespace

extern "C" int abub_trigger_clear_pending_dev(uint8_t *pending, const uint8_t *done, size_t n, void *stream)
{
    if (!pending || !done || n > 0x7fffffffu * (size_t)256)
        return set_err(ABUB_E_INVALID, "abub_trigger_clear_pending_dev: bad arguments");
    if (n == 0)
        return ABUB_OK;
    hipLaunchKernelGGL(k_trigger_clear_pending, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pending, done, n);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}

extern "C" int abub_trigger_search_limits(int *max_frames, int *max_segs)
{
    if (max_frames)
        *max_frames = TRIG_MAXF;
    if (max_segs)
        *max_segs = TRIG_MAXSEG;
    return ABUB_OK;
}

extern "C" size_t abub_trigger_search_desc_bytes(int nstacks, int nsegs)
{
    if (nstacks <= 0 || nsegs < 0)
        return 0;
    return (((size_t)nstacks * sizeof(abub_trig_stack) + 255) & ~(size_t)255) + (size_t)nsegs * sizeof(abub_trig_seg) + 256;
}

extern "C" int abub_trigger_search_dev(const abub_trig_stack *stacks, const abub_trig_seg *segs, int nstacks, int nsegs, int W,
                                       int H, void *desc, size_t desc_bytes, abub_trig_result *out, double *sig_main,
                                       int sig_pitch, void *stream)
{
    static_assert(sizeof(abub_trig_result) == 32 && sizeof(abub_trig_stack) == 24 && sizeof(abub_trig_seg) == 24, "record layout");
    if (!stacks || !out || !desc || nstacks < 0 || nsegs < 0 || (nsegs > 0 && !segs) || W <= 0 || H <= 0 ||
        (size_t)W * H > 0x7fffffffu || (sig_main && sig_pitch <= 0))
        return set_err(ABUB_E_INVALID, "abub_trigger_search_dev: bad arguments");
    // (int)count and (int)((float)rem - count) are defined only while the float is below 2^31.  A bin holds at most W * H
    // pixels and `rem` never rises, so both floats are at most (float)(W * H): 2^31 - 128 up to W * H = 2^31 - 65, and
    // 2^31 from 2^31 - 64 on (the tie goes to the even mantissa) -- undefined on the host, saturating on the device.
    static_assert(ABUB_TRIG_MAX_PIXELS == 0x7fffffff - 64, "the largest int whose float is below 2^31");
    if ((size_t)W * H > (size_t)ABUB_TRIG_MAX_PIXELS)
        return set_err(ABUB_E_INVALID, "abub_trigger_search_dev: W * H above ABUB_TRIG_MAX_PIXELS (a float count would leave the int range)");
    if (nstacks == 0)
        return ABUB_OK;
    if (((uintptr_t)desc & 255) || desc_bytes < abub_trigger_search_desc_bytes(nstacks, nsegs))
        return set_err(ABUB_E_INVALID, "abub_trigger_search_dev: descriptor scratch too small or not 256-byte aligned");
    for (int s = 0; s < nstacks; ++s) {
        const abub_trig_stack &t = stacks[s];
        if (t.F < 0 || t.F > TRIG_MAXF)
            return set_err(ABUB_E_INVALID, "abub_trigger_search_dev: a stack has more frames than abub_trigger_search_limits allows");
        if (t.nseg > TRIG_MAXSEG)
            return set_err(ABUB_E_INVALID, "abub_trigger_search_dev: a stack has more segments than abub_trigger_search_limits allows");
        if ((uint64_t)t.seg0 + t.nseg > (uint64_t)nsegs || (sig_main && t.F > sig_pitch))
            return set_err(ABUB_E_INVALID, "abub_trigger_search_dev: bad stack descriptor");
        int end = 0;
        for (uint32_t k = t.seg0; k < t.seg0 + t.nseg; ++k) {
            const abub_trig_seg &g = segs[k];
            if (g.count < 0 || g.first < end || g.count > 0x7fffffff - g.first || (g.count > 0 && !g.hist))
                return set_err(ABUB_E_INVALID, "abub_trigger_search_dev: segments must be ascending and must not overlap");
            end = g.first + g.count;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    abub_trig_stack *dst = (abub_trig_stack *)desc;
    abub_trig_seg *dsg = (abub_trig_seg *)((uint8_t *)desc + (((size_t)nstacks * sizeof(abub_trig_stack) + 255) & ~(size_t)255));
    HIPCHK(hipMemcpyAsync(dst, stacks, (size_t)nstacks * sizeof(abub_trig_stack), hipMemcpyHostToDevice, st));
    if (nsegs > 0)
        HIPCHK(hipMemcpyAsync(dsg, segs, (size_t)nsegs * sizeof(abub_trig_seg), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_trigger_search, dim3(nstacks), dim3(64), 0, st, dst, dsg, nsegs, (int)((size_t)W * H), out, sig_main,
                       sig_pitch);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}
