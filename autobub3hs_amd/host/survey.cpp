// survey.cpp -- a run measured frame by frame ("Surveying a run"): abub3hs --survey.  No analysis.
// One path: SurveyRun plans the run (one row per frame, the models, one grid of cells), fills every row on one of two
// routes, and writes what the request asks for through one writer per kind of file, the same for both routes.  The host
// route (device < 0) is the definition: per frame cv::imdecode of the frame and of its reference frame, then the plain loops
// of this file.  The device route (--survey-gpu) reads the frames of the run's size through the FileBatch protocol into a
// resident slab and runs one launch per batch and product; what is not in place in the slab gets its row from the host
// route's per-frame function, of which there is one copy.
// What each product adds to that path is its definition, its kernel entry and what its numbers mean:
//   the record      frameStatsHost     abub_frame_stats_dev          SurveyReport
//   planes          activityAddHost    abub_pixel_activity_dev       writePlanes; summed per pixel and camera, not kept per row
//   shift           frameShiftHost     abub_frame_shift_dev          shiftBest reads a surface; ShiftReport
//   field           fieldCellsHost     abub_frame_shift_cells_dev    fieldCell reads a cell's surface; FieldReport
//   light           lightCellsHost     abub_frame_light_cells_dev    lightModelHost once per camera; lightCell, lightFrame; LightReport
//   focus           focusCellsHost     abub_frame_focus_cells_dev    focusModelHost once per camera; focusCell, focusFrame; FocusReport
//   noise           noiseCellsHost     abub_frame_noise_cells_dev    the row against its reference frame, not mu; noiseModelHost once
//                                                                    per camera after the rows; noiseCell, noiseFrame; NoiseReport
//   lines           linesHost          abub_frame_lines_dev          per image row and column, no grid; linesModelHost once per
//                                                                    camera; lineRate, linesFrame; LinesReport, writeLines
// Shift, field, light, focus and noise are made of the ok rows of a camera with a model and share the rest: one two-bit state per
// row, one ProductStats, one timing wrapper on the host, one device leg over one job list (deviceFrames), and for the three
// per-cell products one grid, one report skeleton (cellReport) and one writer (writeCells).
#include <algorithm>
#include <type_traits>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>

#include "AlgorithmTraining/Trainer.hpp"
#include "driver.hpp"
#include "framefiles.hpp"
#include "runbatch.hpp"
#include "runframes.hpp"

#include <sys/stat.h>

namespace abub {

FrameStats frameStatsHost(const unsigned char *cur, const unsigned char *ref, const unsigned char *mu, const unsigned char *sigma6,
                          size_t n)
{
    FrameStats s;
    s.min = n ? 255u : 0u;
    s.flags = (mu ? ABUB_STAT_F_MODEL : 0u) | (mu && ref ? ABUB_STAT_F_REF : 0u);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t p = cur[i];
        s.min = std::min(s.min, p);
        s.max = std::max(s.max, p);
        s.nZero += p == 0;
        s.nSat += p == 255;
        s.sum += p;
        s.sumsq += (uint64_t)p * p;
        if (!mu)
            continue;
        const int lim = sigma6[i];
        const int out = std::abs((int)p - (int)mu[i]) - lim;
        if (out > 0) {
            ++s.nOut;
            s.sumOut += (uint64_t)out;
        }
        if (!ref)
            continue;
        const int moved = std::abs((int)p - (int)ref[i]) - lim;
        if (moved > 0) {
            ++s.nMoved;
            s.sumMoved += (uint64_t)moved;
        }
    }
    return s;
}

void activityAddHost(uint32_t *planes, const unsigned char *cur, const unsigned char *ref, const unsigned char *mu,
                     const unsigned char *sigma6, size_t n)
{
    const auto add = [&](int k, size_t i, uint32_t v) {
        if (v)
            __atomic_fetch_add(planes + (size_t)k * n + i, v, __ATOMIC_RELAXED);
    };
    for (size_t i = 0; i < n; ++i) {
        const int p = cur[i];
        add(0, i, p == 0);
        add(1, i, p == 255);
        if (!mu)
            continue;
        const int lim = sigma6[i];
        const int out = std::max(std::abs(p - (int)mu[i]) - lim, 0);
        add(2, i, out > 0);
        add(3, i, (uint32_t)out);
        if (!ref)
            continue;
        const int moved = std::max(std::abs(p - (int)ref[i]) - lim, 0);
        add(4, i, moved > 0);
        add(5, i, (uint32_t)moved);
    }
}

void frameShiftHost(const unsigned char *p, const unsigned char *m, int W, int H, int R, uint64_t *sad)
{
    const int D = 2 * R + 1;
    for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx) {
            uint64_t s = 0;
            for (int y = R; y < H - R; ++y) {
                const unsigned char *pr = p + (size_t)(y + dy) * W + dx, *mr = m + (size_t)y * W;
                uint32_t row = 0; // (at most 65535 * 255)
                for (int x = R; x < W - R; ++x)
                    row += (uint32_t)std::abs((int)pr[x] - (int)mr[x]);
                s += row;
            }
            sad[(size_t)(dy + R) * D + (dx + R)] = s;
        }
}

template <class T> static ShiftBest shiftBestOf(const T *sad, int R)
{
    const int D = 2 * R + 1;
    ShiftBest b;
    b.sad0 = b.sadBest = sad[(size_t)R * D + R];
    for (int dy = -R; dy <= R; ++dy) // (in the tie rule's last two orders: a later equal one wins only when it is nearer)
        for (int dx = -R; dx <= R; ++dx) {
            const uint64_t v = sad[(size_t)(dy + R) * D + (dx + R)];
            if (v < b.sadBest || (v == b.sadBest && dx * dx + dy * dy < b.dx * b.dx + b.dy * b.dy)) {
                b.sadBest = v;
                b.dx = dx;
                b.dy = dy;
            }
        }
    b.atEdge = std::abs(b.dx) == R || std::abs(b.dy) == R;
    return b;
}
ShiftBest shiftBest(const uint64_t *sad, int R) { return shiftBestOf(sad, R); }
ShiftBest shiftBest(const uint32_t *sad, int R) { return shiftBestOf(sad, R); }

size_t fieldCellsHost(const unsigned char *p, const unsigned char *m, int W, int H, int R, uint32_t *sad)
{
    int ncx = 0, ncy = 0, x0 = 0, y0 = 0;
    if (abub_frame_cells_grid(W, H, R, &ncx, &ncy, &x0, &y0) != ABUB_OK)
        return 0;
    const int C = ABUB_FIELD_CELL, D = 2 * R + 1;
    for (int cy = 0; cy < ncy; ++cy)
        for (int cx = 0; cx < ncx; ++cx) {
            uint32_t *out = sad + ((size_t)cy * ncx + cx) * D * D;
            const int xa = x0 + C * cx, ya = y0 + C * cy;
            for (int dy = -R; dy <= R; ++dy)
                for (int dx = -R; dx <= R; ++dx) {
                    uint32_t s = 0; // (at most 16384 * 255)
                    for (int y = ya; y < ya + C; ++y) {
                        const unsigned char *pr = p + (size_t)(y + dy) * W + dx, *mr = m + (size_t)y * W;
                        for (int x = xa; x < xa + C; ++x)
                            s += (uint32_t)std::abs((int)pr[x] - (int)mr[x]);
                    }
                    out[(size_t)(dy + R) * D + (dx + R)] = s;
                }
        }
    return (size_t)ncx * ncy;
}

void fieldCell(const uint32_t *sad, int R, int32_t *rec)
{
    const ShiftBest b = shiftBest(sad, R);
    const size_t N = (size_t)(2 * R + 1) * (2 * R + 1);
    rec[0] = b.dx;
    rec[1] = b.dy;
    rec[2] = (int32_t)b.sad0;
    rec[3] = (int32_t)b.sadBest;
    rec[4] = (int32_t)*std::max_element(sad, sad + N);
}

void lightCellsHost(const unsigned char *p, const unsigned char *m, int W, int H, int x0, int y0, int ncx, int ncy, uint32_t *rec)
{
    (void)H;
    const int C = ABUB_FIELD_CELL;
    for (int cy = 0; cy < ncy; ++cy)
        for (int cx = 0; cx < ncx; ++cx) {
            uint32_t sp = 0, spp = 0, spm = 0, sad = 0, nZero = 0, nSat = 0; // (at most 16384 * 255^2 < 2^31)
            for (int y = y0 + C * cy; y < y0 + C * (cy + 1); ++y) {
                const unsigned char *pr = p + (size_t)y * W, *mr = m + (size_t)y * W;
                for (int x = x0 + C * cx; x < x0 + C * (cx + 1); ++x) {
                    const uint32_t a = pr[x], b = mr[x];
                    sp += a;
                    spp += a * a;
                    spm += a * b;
                    sad += a > b ? a - b : b - a;
                    nZero += a == 0;
                    nSat += a == 255;
                }
            }
            uint32_t *out = rec + ((size_t)cy * ncx + cx) * LightRecordWords;
            out[0] = sp;
            out[1] = spp;
            out[2] = spm;
            out[3] = sad;
            out[4] = nZero;
            out[5] = nSat;
        }
}

void lightModelHost(const unsigned char *mu, const unsigned char *sigma6, int W, int H, int x0, int y0, int ncx, int ncy, uint32_t *rec)
{
    (void)H;
    const int C = ABUB_FIELD_CELL;
    for (int cy = 0; cy < ncy; ++cy)
        for (int cx = 0; cx < ncx; ++cx) {
            uint32_t sm = 0, smm = 0, ss6 = 0;
            for (int y = y0 + C * cy; y < y0 + C * (cy + 1); ++y)
                for (int x = x0 + C * cx; x < x0 + C * (cx + 1); ++x) {
                    const uint32_t b = mu[(size_t)y * W + x];
                    sm += b;
                    smm += b * b;
                    ss6 += sigma6[(size_t)y * W + x];
                }
            uint32_t *out = rec + ((size_t)cy * ncx + cx) * LightModelWords;
            out[0] = sm;
            out[1] = smm;
            out[2] = ss6;
        }
}

long long lightRdiv(__int128 a, __int128 b)
{
    const __int128 n = 2 * a + b, d = 2 * b;
    __int128 q = n / d; // (truncates toward 0: one less where the remainder is negative)
    if (n % d < 0)
        --q;
    return (long long)q;
}

LightCell lightCell(const uint32_t *rec, const uint32_t *model)
{
    const long long N = (long long)ABUB_FIELD_CELL * ABUB_FIELD_CELL, sp = rec[0], sm = model[0], ss6 = model[2];
    LightCell c;
    if (sm < N)
        return c;
    c.clipped = (long long)rec[4] + rec[5] > N / 16;
    if (c.clipped)
        return c;
    c.rated = true;
    c.ratio = lightRdiv((__int128)1000 * sp, sm);
    c.changed = std::llabs(sp - sm) > ss6;
    c.up = c.changed && sp > sm;
    return c;
}

LightFrame lightFrame(const uint32_t *rec, const uint32_t *model, size_t cells)
{
    LightFrame f;
    __int128 Ssp = 0, Sspm = 0, Ssm = 0, Ssmm = 0;
    for (size_t k = 0; k < cells; ++k) {
        const uint32_t *r = rec + k * LightRecordWords, *m = model + k * LightModelWords;
        const LightCell c = lightCell(r, m);
        f.clipped += c.clipped;
        if (!c.rated)
            continue;
        f.ratioMin = f.rated ? std::min(f.ratioMin, c.ratio) : c.ratio;
        f.ratioMax = f.rated ? std::max(f.ratioMax, c.ratio) : c.ratio;
        ++f.rated;
        f.changed += c.changed;
        f.up += c.up;
        f.down += c.changed && !c.up;
        Ssp += r[0];
        Sspm += r[2];
        Ssm += m[0];
        Ssmm += m[1];
    }
    if (!f.rated)
        return f;
    const __int128 n = (__int128)ABUB_FIELD_CELL * ABUB_FIELD_CELL * f.rated;
    f.levelMilli = lightRdiv(1000 * (Ssp - Ssm), n);
    const __int128 var = n * Ssmm - Ssm * Ssm, cov = n * Sspm - Ssp * Ssm;
    if (var > 0) {
        f.hasGain = true;
        f.gainMilli = lightRdiv(1000 * cov, var);
        f.offsetMilli = lightRdiv(1000 * Ssp - (__int128)f.gainMilli * Ssm, n);
    }
    f.kind = !f.changed ? LightFrame::Steady : f.changed == f.rated && (f.up == 0 || f.down == 0) ? LightFrame::Level : LightFrame::Uneven;
    return f;
}

void focusCellsHost(const unsigned char *p, const unsigned char *m, int W, int H, int x0, int y0, int ncx, int ncy, int32_t *rec)
{
    (void)H;
    const int C = ABUB_FIELD_CELL;
    for (int cy = 0; cy < ncy; ++cy)
        for (int cx = 0; cx < ncx; ++cx) {
            int32_t gxx = 0, gyy = 0, gxm = 0, gym = 0, nClip = 0; // (a magnitude of at most 16384 * 255^2 < 2^31)
            for (int y = y0 + C * cy; y < y0 + C * (cy + 1); ++y) {
                const unsigned char *pr = p + (size_t)y * W, *mr = m + (size_t)y * W;
                for (int x = x0 + C * cx; x < x0 + C * (cx + 1); ++x) {
                    const int32_t gx = (int32_t)pr[x + 1] - pr[x - 1], gy = (int32_t)pr[x + W] - pr[x - W];
                    const int32_t hx = (int32_t)mr[x + 1] - mr[x - 1], hy = (int32_t)mr[x + W] - mr[x - W];
                    gxx += gx * gx;
                    gyy += gy * gy;
                    gxm += gx * hx;
                    gym += gy * hy;
                    nClip += pr[x] == 0 || pr[x] == 255;
                }
            }
            int32_t *out = rec + ((size_t)cy * ncx + cx) * FocusRecordWords;
            out[0] = gxx;
            out[1] = gyy;
            out[2] = gxm;
            out[3] = gym;
            out[4] = nClip;
        }
}

void focusModelHost(const unsigned char *mu, const unsigned char *sigma6, int W, int H, int x0, int y0, int ncx, int ncy, int64_t *rec)
{
    (void)H;
    const int C = ABUB_FIELD_CELL;
    for (int cy = 0; cy < ncy; ++cy)
        for (int cx = 0; cx < ncx; ++cx) {
            const int xa = x0 + C * cx, xb = xa + C, ya = y0 + C * cy, yb = ya + C; // K = [xa, xb) x [ya, yb)
            auto inK = [&](int x, int y) { return x >= xa && x < xb && y >= ya && y < yb; };
            auto hx = [&](int x, int y) { return (int64_t)mu[(size_t)y * W + x + 1] - mu[(size_t)y * W + x - 1]; };
            auto hy = [&](int x, int y) { return (int64_t)mu[(size_t)(y + 1) * W + x] - mu[(size_t)(y - 1) * W + x]; };
            int64_t mxx = 0, myy = 0, nv = 0; // (nv <= 16900 * (255 * 1020)^2 < 2^63)
            for (int y = ya - 1; y <= yb; ++y)
                for (int x = xa - 1; x <= xb; ++x) {
                    if (inK(x, y)) {
                        mxx += hx(x, y) * hx(x, y);
                        myy += hy(x, y) * hy(x, y);
                    }
                    int64_t c = 0; // the coefficient of p(x, y) in G
                    if (inK(x - 1, y))
                        c += hx(x - 1, y);
                    if (inK(x + 1, y))
                        c -= hx(x + 1, y);
                    if (inK(x, y - 1))
                        c += hy(x, y - 1);
                    if (inK(x, y + 1))
                        c -= hy(x, y + 1);
                    const int64_t t = (int64_t)sigma6[(size_t)y * W + x] * c;
                    nv += t * t;
                }
            int64_t *out = rec + ((size_t)cy * ncx + cx) * FocusModelWords;
            out[0] = mxx;
            out[1] = myy;
            out[2] = nv;
        }
}

FocusCell focusCell(const int32_t *rec, const int64_t *model)
{
    const long long N = (long long)ABUB_FIELD_CELL * ABUB_FIELD_CELL;
    const __int128 G = (__int128)rec[2] + rec[3], M = (__int128)model[0] + model[1], nv = model[2];
    FocusCell c;
    c.clipped = rec[4] > N / 16;
    if (c.clipped || !(M * M > nv))
        return c;
    c.rated = true;
    c.keep = lightRdiv(1000 * G, M);
    c.energy = lightRdiv(1000 * ((__int128)rec[0] + rec[1]), M);
    c.changed = (M - G) * (M - G) > nv;
    c.softer = c.changed && G < M;
    return c;
}

FocusFrame focusFrame(const int32_t *rec, const int64_t *model, size_t cells)
{
    FocusFrame f;
    __int128 SG = 0, SM = 0, SE = 0;
    for (size_t k = 0; k < cells; ++k) {
        const int32_t *r = rec + k * FocusRecordWords;
        const int64_t *m = model + k * FocusModelWords;
        const FocusCell c = focusCell(r, m);
        f.clipped += c.clipped;
        if (!c.rated)
            continue;
        f.keepMin = f.rated ? std::min(f.keepMin, c.keep) : c.keep;
        f.keepMax = f.rated ? std::max(f.keepMax, c.keep) : c.keep;
        ++f.rated;
        f.changed += c.changed;
        f.softer += c.softer;
        f.harder += c.changed && !c.softer;
        SG += (__int128)r[2] + r[3];
        SE += (__int128)r[0] + r[1];
        SM += (__int128)m[0] + m[1];
    }
    if (!f.rated)
        return f;
    f.keepMilli = lightRdiv(1000 * SG, SM); // (SM > 0: every rated cell has M^2 > nv >= 0)
    f.energyMilli = lightRdiv(1000 * SE, SM);
    f.kind = !f.changed ? FocusFrame::Steady : f.changed == f.rated && f.harder == 0 ? FocusFrame::Soft : FocusFrame::Uneven;
    return f;
}

void noiseCellsHost(const unsigned char *p, const unsigned char *r, const unsigned char *sigma6, int W, int H, int x0, int y0, int ncx,
                    int ncy, int32_t *rec)
{
    (void)H;
    const int C = ABUB_FIELD_CELL;
    for (int cy = 0; cy < ncy; ++cy)
        for (int cx = 0; cx < ncx; ++cx) {
            int32_t nOver = 0, nClip = 0, s1In = 0, s2In = 0, sad = 0, s2All = 0; // (a magnitude of at most 16384 * 255^2 < 2^31)
            for (int y = y0 + C * cy; y < y0 + C * (cy + 1); ++y) {
                const unsigned char *pr = p + (size_t)y * W, *rr = r + (size_t)y * W, *sr = sigma6 + (size_t)y * W;
                for (int x = x0 + C * cx; x < x0 + C * (cx + 1); ++x) {
                    const int32_t d = (int32_t)pr[x] - rr[x], a = std::abs(d);
                    nClip += pr[x] == 0 || pr[x] == 255 || rr[x] == 0 || rr[x] == 255;
                    sad += a;
                    s2All += d * d;
                    if (a > sr[x]) {
                        ++nOver;
                        continue;
                    }
                    s1In += d;
                    s2In += d * d;
                }
            }
            int32_t *out = rec + ((size_t)cy * ncx + cx) * NoiseRecordWords;
            out[0] = nOver;
            out[1] = nClip;
            out[2] = s1In;
            out[3] = s2In;
            out[4] = sad;
            out[5] = s2All;
        }
}

void noiseModelHost(const unsigned char *sigma6, int W, int H, int x0, int y0, int ncx, int ncy, const int32_t *const *recs, size_t nrecs,
                    int64_t *rec)
{
    (void)H;
    const int C = ABUB_FIELD_CELL;
    for (int cy = 0; cy < ncy; ++cy)
        for (int cx = 0; cx < ncx; ++cx) {
            const size_t k = (size_t)cy * ncx + cx;
            int64_t BE = 0, BN = 0, B = 0, ss = 0, zero = 0; // (ss <= 16384 * 255^2)
            for (size_t q = 0; q < nrecs; ++q) {
                const int32_t *r = recs[q] + k * NoiseRecordWords;
                if (noiseClipped(r) || noiseBusy(r))
                    continue;
                BE += noiseE(r);
                BN += noiseNIn(r);
                ++B;
            }
            for (int y = y0 + C * cy; y < y0 + C * (cy + 1); ++y)
                for (int x = x0 + C * cx; x < x0 + C * (cx + 1); ++x) {
                    const int64_t s = sigma6[(size_t)y * W + x];
                    ss += s * s;
                    zero += s == 0;
                }
            int64_t *out = rec + k * NoiseModelWords;
            out[0] = BE;
            out[1] = BN;
            out[2] = B;
            out[3] = ss;
            out[4] = zero;
        }
}

NoiseCell noiseCell(const int32_t *rec, const int64_t *model)
{
    typedef unsigned __int128 u128;
    const long long N = NoiseCellPixels, BE = model[0], BN = model[1], B = model[2];
    const bool base = BE > 0 && B > 0;
    NoiseCell c;
    if (base)
        c.allMilli = (long long)((u128)1000 * (u128)rec[5] * (u128)BN / ((u128)N * (u128)BE));
    if (noiseClipped(rec))
        c.state = NoiseCell::Clipped;
    else if (noiseBusy(rec))
        c.state = NoiseCell::Busy;
    else if (!base)
        c.state = NoiseCell::NoBase;
    else { // (n_in >= 3 N / 4 > 0: the cell is not busy)
        c.qMilli = (long long)((u128)1000 * (u128)noiseE(rec) * (u128)BN / ((u128)noiseNIn(rec) * (u128)BE));
        c.state = c.qMilli > NoiseNoisyMilli ? NoiseCell::Noisy : c.qMilli < NoiseQuietMilli ? NoiseCell::Quiet : NoiseCell::Same;
    }
    return c;
}

long long noiseModelMilli(const int64_t *model)
{
    typedef unsigned __int128 u128;
    if (model[1] <= 0 || model[3] <= 0)
        return 0;
    return (long long)((u128)(1000 * 18) * (u128)model[0] * (u128)NoiseCellPixels / ((u128)model[1] * (u128)model[3]));
}

NoiseFrame noiseFrame(const int32_t *rec, const int64_t *model, size_t cells)
{
    typedef unsigned __int128 u128;
    NoiseFrame f;
    u128 qNum = 0, qDen = 0, aNum = 0, aDen = 0;
    for (size_t k = 0; k < cells; ++k) {
        const int32_t *r = rec + k * NoiseRecordWords;
        const int64_t *m = model + k * NoiseModelWords;
        const NoiseCell c = noiseCell(r, m);
        f.clipped += c.state == NoiseCell::Clipped;
        f.busy += c.state == NoiseCell::Busy;
        if (c.state != NoiseCell::Clipped && m[0] > 0 && m[2] > 0) {
            aNum += (u128)r[5] * (u128)m[1];
            aDen += (u128)NoiseCellPixels * (u128)m[0];
        }
        if (!c.rated())
            continue;
        f.qMin = f.rated ? std::min(f.qMin, c.qMilli) : c.qMilli;
        f.qMax = f.rated ? std::max(f.qMax, c.qMilli) : c.qMilli;
        ++f.rated;
        f.noisy += c.state == NoiseCell::Noisy;
        f.quiet += c.state == NoiseCell::Quiet;
        qNum += (u128)noiseE(r) * (u128)m[1];
        qDen += (u128)noiseNIn(r) * (u128)m[0];
    }
    if (f.rated)
        f.qMilli = (long long)((u128)1000 * qNum / qDen);
    if (aDen)
        f.allMilli = (long long)((u128)1000 * aNum / aDen);
    const long long U = (long long)cells - f.clipped;
    f.kind = (long long)(f.rated + f.busy) * 4 < (long long)cells ? NoiseFrame::Blind
             : f.busy * 2 > U                                      ? NoiseFrame::Busy
             : !f.noisy && !f.quiet                                ? NoiseFrame::Steady
             : !f.quiet && f.noisy * 2 >= f.rated                  ? NoiseFrame::Noisy
             : !f.noisy && f.quiet * 2 >= f.rated                  ? NoiseFrame::Quiet
                                                                   : NoiseFrame::Uneven;
    return f;
}

void linesHost(const unsigned char *p, const unsigned char *r, const unsigned char *mu, int W, int H, uint32_t *rows, uint32_t *cols)
{
    std::fill(rows, rows + (size_t)H * LinesRowWords, 0u);
    std::fill(cols, cols + (size_t)W * LinesColWords, 0u);
    for (int y = 0; y < H; ++y) {
        const unsigned char *pr = p + (size_t)y * W, *mr = mu + (size_t)y * W, *rr = r ? r + (size_t)y * W : nullptr;
        uint32_t *row = rows + (size_t)y * LinesRowWords;
        for (int x = 0; x < W; ++x) {
            const uint32_t v = pr[x], dev = (uint32_t)std::abs((int)pr[x] - (int)mr[x]), clip = v == 0 || v == 255;
            uint32_t *col = cols + (size_t)x * LinesColWords;
            row[0] += v;
            row[1] += dev;
            row[2] += clip;
            col[0] += v;
            col[1] += dev;
            col[2] += clip;
            if (rr) {
                row[3] += (uint32_t)std::abs((int)pr[x] - (int)rr[x]);
                row[4] += pr[x] == rr[x];
            }
        }
    }
}

void linesModelHost(const unsigned char *mu, const unsigned char *sigma6, int W, int H, uint32_t *rows, uint32_t *cols)
{
    std::fill(rows, rows + (size_t)H * LinesModelWords, 0u);
    std::fill(cols, cols + (size_t)W * LinesModelWords, 0u);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const uint32_t m = mu[(size_t)y * W + x], s = sigma6[(size_t)y * W + x];
            uint32_t *row = rows + (size_t)y * LinesModelWords, *col = cols + (size_t)x * LinesModelWords;
            row[0] += m;
            row[1] += s;
            row[2] += s == 0;
            col[0] += m;
            col[1] += s;
            col[2] += s == 0;
        }
}

bool lineRated(const uint32_t *rec, const uint32_t *model, long long N)
{
    return (long long)LinesShare * rec[2] <= N && (long long)LinesShare * model[2] <= N;
}

int lineRate(const uint32_t *rec, const uint32_t *model, long long N, long long n, long long S, unsigned __int128 *num, unsigned __int128 *den)
{
    typedef unsigned __int128 u128;
    if (!lineRated(rec, model, N))
        return LineUnrated;
    const __int128 e = (__int128)n * ((long long)rec[0] - (long long)model[0]) - (__int128)S;
    const u128 a = (u128)(e < 0 ? -e : e), nT = (u128)n * (u128)model[1]; // (a < 2^41 and nT < 2^40 with sides of at most 65535)
    const u128 lhs = a * a * (u128)N, rhs = nT * nT;
    if (num)
        *num = lhs;
    if (den)
        *den = rhs;
    return lhs > (u128)LinesFactor * rhs ? LineOff : LineRated;
}

LinesFrame linesFrame(const uint32_t *rows, const uint32_t *cols, const uint32_t *modelRows, const uint32_t *modelCols, int W, int H,
                      bool hasRef, uint8_t *rowState, uint8_t *colState)
{
    LinesFrame f;
    // one direction: the rated lines, their number and their sum of D first, then every rated line against them
    const auto direction = [](const uint32_t *rec, size_t words, const uint32_t *model, int lines, long long N, int &rated, int &off,
                              int &firstOff, int &lastOff, long long &S, uint8_t *state) {
        long long n = 0;
        S = 0;
        for (int k = 0; k < lines; ++k)
            if (lineRated(rec + (size_t)k * words, model + (size_t)k * LinesModelWords, N)) {
                ++n;
                S += (long long)rec[(size_t)k * words] - (long long)model[(size_t)k * LinesModelWords];
            }
        rated = (int)n;
        for (int k = 0; k < lines; ++k) {
            const int s = lineRate(rec + (size_t)k * words, model + (size_t)k * LinesModelWords, N, n, S);
            if (state)
                state[k] = (uint8_t)s;
            if (s != LineOff)
                continue;
            ++off;
            firstOff = firstOff < 0 ? k : firstOff;
            lastOff = k;
        }
    };
    long long S = 0, Sc = 0;
    direction(rows, LinesRowWords, modelRows, H, W, f.ratedRows, f.offRows, f.firstOffRow, f.lastOffRow, S, rowState);
    direction(cols, LinesColWords, modelCols, W, H, f.ratedCols, f.offCols, f.firstOffCol, f.lastOffCol, Sc, colState);
    if (f.ratedRows) {
        const long long num = 1000 * S, den = (long long)f.ratedRows * W; // (|S| < 2^40)
        f.levelMilli = num >= 0 ? num / den : -((-num + den - 1) / den);   // (the floor)
    }
    int run = 0, longest = 0;
    for (int y = 0; y < H; ++y) {
        const uint32_t *row = rows + (size_t)y * LinesRowWords;
        const bool stale = hasRef && row[4] == (uint32_t)W && lineRated(row, modelRows + (size_t)y * LinesModelWords, W);
        run = stale ? run + 1 : 0;
        longest = std::max(longest, run);
        if (!stale)
            continue;
        ++f.staleRows;
        f.firstStale = f.firstStale < 0 ? y : f.firstStale;
        f.lastStale = y;
        if (rowState)
            rowState[y] = LineStale;
    }
    f.kind = 4ll * f.ratedRows < H                   ? LinesFrame::Blind
             : hasRef && f.staleRows == f.ratedRows  ? LinesFrame::Repeated
             : longest >= LinesTornRun               ? LinesFrame::Torn
             : f.offRows >= LinesOffLines            ? LinesFrame::Banded
             : f.offCols >= LinesOffLines            ? LinesFrame::Striped
                                                     : LinesFrame::Steady;
    return f;
}

// the columns every table of a survey begins with
static void rowPrefix(std::string &text, const SurveyRow &r)
{
    char buf[512];
    snprintf(buf, sizeof buf, "%s\t%d\t%d\t%s\t%s", r.event.c_str(), r.cam, r.frame, r.name.c_str(), r.stateName());
    text += buf;
}

namespace {

// What differs between field.txt, light.txt and focus.txt; cellReport is the rest
struct CellReport {
    const char *tag;                 // of "# abub3hs <tag> 1" and of the `<tag> cam` lines
    const char *columns;             // the table's column names between `index` and `kind`; a row without a record has a dash in each
    std::vector<const char *> kinds; // the kinds' names, blind first
    const char *mapWord;             // `moved` or `changed`: what the per-cell map's lines count the frames of
    const char *firstLabel;          // of the `<tag> cam` lines: first_..._event
    // One row: -1 if it has no record.  Else its columns are appended to `cols`, `first` says whether the row counts as its
    // camera's first event, hit[k] is raised for every cell that counts in the map; returns the row's kind
    std::function<int(const SurveyRow &r, size_t cells, std::string &cols, bool &first, std::vector<long long> &hit)> row;
    std::function<std::string(size_t cam, size_t cells)> camTail; // (may be empty) what a trained camera's `<tag> cam` line ends with
};

std::string cellReport(const CellReport &d, int radius, int W, int H, const std::vector<SurveyModel> &models,
                       const std::vector<SurveyRow> &rows)
{
    int ncx = 0, ncy = 0, x0 = 0, y0 = 0;
    if (W > 0 && H > 0)
        abub_frame_cells_grid(W, H, radius, &ncx, &ncy, &x0, &y0);
    const size_t cells = (size_t)ncx * ncy, K = d.kinds.size();
    std::string text = std::string("# abub3hs ") + d.tag + " 1\n";
    char buf[512];
    snprintf(buf, sizeof buf, "radius %d cell %d grid %d %d origin %d %d\n", radius, (int)ABUB_FIELD_CELL, ncx, ncy, x0, y0);
    text += buf;
    text += std::string("event\tcam\tframe\tname\tstate\tindex\t") + d.columns + "\tkind\n";
    std::string dashes = "\t-\t-\t-"; // index, the first column, kind; one more per further column
    for (const char *c = d.columns; *c; ++c)
        if (*c == '\t')
            dashes += "\t-";
    struct Cam {
        long long frames = 0;
        std::vector<long long> kind;
        const std::string *first = nullptr;
        std::vector<long long> perCell; // per cell: the frames in which it counted in the map
    };
    std::vector<Cam> cams(models.size());
    std::vector<long long> hit;
    for (const SurveyRow &r : rows) {
        rowPrefix(text, r);
        std::string cols;
        bool first = false;
        hit.assign(cells, 0);
        const int kind = d.row(r, cells, cols, first, hit);
        if (kind < 0) {
            text += dashes + "\n";
            continue;
        }
        Cam &c = cams[(size_t)r.cam];
        c.kind.resize(K, 0);
        c.perCell.resize(cells, 0);
        for (size_t k = 0; k < cells; ++k)
            c.perCell[k] += hit[k];
        snprintf(buf, sizeof buf, "\t%lld", c.frames);
        text += buf + cols + "\t" + d.kinds[(size_t)kind] + "\n";
        ++c.frames;
        ++c.kind[(size_t)kind];
        if (first && !c.first)
            c.first = &r.event;
    }
    long long frames = 0;
    std::vector<long long> kind(K, 0);
    for (size_t c = 0; c < cams.size(); ++c) {
        if (!models[c].trained) {
            snprintf(buf, sizeof buf, "%s cam %zu none\n", d.tag, c);
            text += buf;
            continue;
        }
        Cam &k = cams[c];
        k.kind.resize(K, 0);
        snprintf(buf, sizeof buf, "%s cam %zu frames %lld", d.tag, c, k.frames);
        text += buf;
        for (size_t q = 0; q < K; ++q) {
            snprintf(buf, sizeof buf, " %s %lld", d.kinds[q], k.kind[q]);
            text += buf;
            kind[q] += k.kind[q];
        }
        text += std::string(" ") + d.firstLabel + " " + (k.first ? *k.first : std::string("-")) + (d.camTail ? d.camTail(c, cells) : "") + "\n";
        frames += k.frames;
    }
    for (size_t c = 0; c < cams.size(); ++c) {
        if (!models[c].trained)
            continue;
        for (int y = 0; y < ncy; ++y) {
            snprintf(buf, sizeof buf, "%s cam %zu y %d", d.mapWord, c, y);
            text += buf;
            for (int x = 0; x < ncx; ++x) {
                const size_t k = (size_t)y * ncx + x;
                snprintf(buf, sizeof buf, " %lld", k < cams[c].perCell.size() ? cams[c].perCell[k] : 0ll);
                text += buf;
            }
            text += "\n";
        }
    }
    snprintf(buf, sizeof buf, "run frames %lld", frames);
    text += buf;
    for (size_t q = 0; q < K; ++q) {
        snprintf(buf, sizeof buf, " %s %lld", d.kinds[q], kind[q]);
        text += buf;
    }
    return text + "\n";
}

} // namespace

std::string FieldReport(int radius, int W, int H, const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows)
{
    enum { Blind, Still, Rigid, Warped, Local };
    const auto row = [](const SurveyRow &r, size_t cells, std::string &cols, bool &first, std::vector<long long> &hit) -> int {
        if (r.state != SurveyRow::Ok || !r.has(SurveyFieldProduct) || r.field.size() != cells * FieldRecordWords)
            return -1;
        int rated = 0, moved = 0, dxMin = 0, dxMax = 0, dyMin = 0, dyMax = 0;
        std::map<std::pair<int, int>, int> seen; // (dy, dx) of the rated cells -> how many
        for (size_t k = 0; k < cells; ++k) {
            const int32_t *rec = r.field.data() + k * FieldRecordWords;
            if (!fieldRated(rec))
                continue;
            const int dx = rec[0], dy = rec[1];
            dxMin = rated ? std::min(dxMin, dx) : dx;
            dxMax = rated ? std::max(dxMax, dx) : dx;
            dyMin = rated ? std::min(dyMin, dy) : dy;
            dyMax = rated ? std::max(dyMax, dy) : dy;
            ++rated;
            ++seen[{dy, dx}];
            if (dx != 0 || dy != 0) {
                ++moved;
                ++hit[k];
            }
        }
        // the most frequent displacement; among equally frequent ones shiftBest's order: the nearer, the smaller dy, the smaller dx
        int mdx = 0, mdy = 0, mn = 0;
        for (const auto &kv : seen) { // (in (dy, dx) order: a later equal one wins only when it is nearer)
            const int dy = kv.first.first, dx = kv.first.second;
            if (kv.second > mn || (kv.second == mn && dx * dx + dy * dy < mdx * mdx + mdy * mdy)) {
                mn = kv.second;
                mdx = dx;
                mdy = dy;
            }
        }
        const int kind = !rated ? Blind : !moved ? Still : moved < rated ? Local : seen.size() == 1 ? Rigid : Warped;
        char buf[512];
        if (kind == Blind)
            snprintf(buf, sizeof buf, "\t%d\t%d\t-\t-\t-\t-\t-\t-\t-", rated, moved);
        else
            snprintf(buf, sizeof buf, "\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d", rated, moved, mdx, mdy, mn, dxMin, dxMax, dyMin, dyMax);
        cols += buf;
        first = moved != 0;
        return kind;
    };
    return cellReport({"field", "rated\tmoved\tmodal_dx\tmodal_dy\tmodal_n\tdx_min\tdx_max\tdy_min\tdy_max",
                       {"blind", "still", "rigid", "warped", "local"}, "moved", "first_moved_event", row, nullptr},
                      radius, W, H, models, rows);
}

std::string LightReport(int radius, int W, int H, const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows)
{
    const auto row = [&](const SurveyRow &r, size_t cells, std::string &cols, bool &first, std::vector<long long> &hit) -> int {
        const std::vector<uint32_t> *model = (size_t)r.cam < models.size() ? &models[(size_t)r.cam].light : nullptr;
        if (r.state != SurveyRow::Ok || !r.has(SurveyLightProduct) || r.light.size() != cells * LightRecordWords || !model ||
            model->size() != cells * LightModelWords)
            return -1;
        const LightFrame f = lightFrame(r.light.data(), model->data(), cells);
        for (size_t k = 0; k < cells; ++k) {
            const LightCell lc = lightCell(r.light.data() + k * LightRecordWords, model->data() + k * LightModelWords);
            hit[k] += lc.rated && lc.changed;
        }
        char buf[512];
        snprintf(buf, sizeof buf, "\t%d\t%d\t%d\t%d\t%d", f.rated, f.clipped, f.changed, f.up, f.down);
        cols += buf;
        if (f.kind == LightFrame::Blind)
            snprintf(buf, sizeof buf, "\t-\t-\t-\t-\t-");
        else if (f.hasGain)
            snprintf(buf, sizeof buf, "\t%lld\t%lld\t%lld\t%lld\t%lld", f.levelMilli, f.ratioMin, f.ratioMax, f.gainMilli, f.offsetMilli);
        else
            snprintf(buf, sizeof buf, "\t%lld\t%lld\t%lld\t-\t-", f.levelMilli, f.ratioMin, f.ratioMax);
        cols += buf;
        first = f.changed != 0;
        return f.kind;
    };
    return cellReport({"light", "rated\tclipped\tchanged\tup\tdown\tlevel_milli\tratio_min\tratio_max\tgain_milli\toffset_milli",
                       {"blind", "steady", "level", "uneven"}, "changed", "first_changed_event", row, nullptr},
                      radius, W, H, models, rows);
}

std::string FocusReport(int radius, int W, int H, const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows)
{
    const auto row = [&](const SurveyRow &r, size_t cells, std::string &cols, bool &first, std::vector<long long> &hit) -> int {
        const std::vector<int64_t> *model = (size_t)r.cam < models.size() ? &models[(size_t)r.cam].focus : nullptr;
        if (r.state != SurveyRow::Ok || !r.has(SurveyFocusProduct) || r.focus.size() != cells * FocusRecordWords || !model ||
            model->size() != cells * FocusModelWords)
            return -1;
        const FocusFrame f = focusFrame(r.focus.data(), model->data(), cells);
        for (size_t k = 0; k < cells; ++k) {
            const FocusCell fc = focusCell(r.focus.data() + k * FocusRecordWords, model->data() + k * FocusModelWords);
            hit[k] += fc.rated && fc.changed;
        }
        char buf[512];
        snprintf(buf, sizeof buf, "\t%d\t%d\t%d\t%d\t%d", f.rated, f.clipped, f.changed, f.softer, f.harder);
        cols += buf;
        if (f.kind == FocusFrame::Blind)
            snprintf(buf, sizeof buf, "\t-\t-\t-\t-");
        else
            snprintf(buf, sizeof buf, "\t%lld\t%lld\t%lld\t%lld", f.keepMilli, f.keepMin, f.keepMax, f.energyMilli);
        cols += buf;
        first = f.changed != 0;
        return f.kind;
    };
    return cellReport({"focus", "rated\tclipped\tchanged\tsofter\tharder\tkeep_milli\tkeep_min\tkeep_max\tenergy_milli",
                       {"blind", "steady", "soft", "uneven"}, "changed", "first_changed_event", row, nullptr},
                      radius, W, H, models, rows);
}

std::string NoiseReport(int radius, int W, int H, const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows)
{
    const auto modelOf = [&](size_t cam, size_t cells) -> const std::vector<int64_t> * {
        return cam < models.size() && models[cam].noise.size() == cells * NoiseModelWords ? &models[cam].noise : nullptr;
    };
    const auto row = [&](const SurveyRow &r, size_t cells, std::string &cols, bool &first, std::vector<long long> &hit) -> int {
        const std::vector<int64_t> *model = modelOf((size_t)r.cam, cells);
        if (r.state != SurveyRow::Ok || !r.has(SurveyNoiseProduct) || r.noise.size() != cells * NoiseRecordWords || !model)
            return -1;
        const NoiseFrame f = noiseFrame(r.noise.data(), model->data(), cells);
        for (size_t k = 0; k < cells; ++k) {
            const NoiseCell nc = noiseCell(r.noise.data() + k * NoiseRecordWords, model->data() + k * NoiseModelWords);
            hit[k] += nc.state == NoiseCell::Noisy || nc.state == NoiseCell::Quiet;
        }
        char buf[512];
        snprintf(buf, sizeof buf, "\t%d\t%d\t%d\t%d\t%d", f.rated, f.clipped, f.busy, f.noisy, f.quiet);
        cols += buf;
        if (f.rated)
            snprintf(buf, sizeof buf, "\t%lld\t%lld\t%lld\t%lld", f.qMilli, f.qMin, f.qMax, f.allMilli);
        else
            snprintf(buf, sizeof buf, "\t-\t-\t-\t%lld", f.allMilli);
        cols += buf;
        first = f.noisy + f.quiet != 0;
        return f.kind;
    };
    const auto camTail = [&](size_t cam, size_t cells) {
        std::string tail = " model_milli";
        const std::vector<int64_t> *model = modelOf(cam, cells);
        for (size_t k = 0; k < cells; ++k)
            tail += " " + std::to_string(model ? noiseModelMilli(model->data() + k * NoiseModelWords) : 0ll);
        return tail;
    };
    return cellReport({"noise", "rated\tclipped\tbusy\tnoisy\tquiet\tq_milli\tq_min\tq_max\tall_milli",
                       {"blind", "busy", "steady", "noisy", "quiet", "uneven"}, "changed", "first_changed_event", row, camTail},
                      radius, W, H, models, rows);
}

std::string LinesReport(int W, int H, const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows)
{
    static const char *const kinds[] = {"blind", "repeated", "torn", "banded", "striped", "steady"};
    enum : size_t { K = sizeof kinds / sizeof *kinds };
    std::string text = "# abub3hs lines 1\n";
    char buf[512];
    snprintf(buf, sizeof buf, "size %d %d\n", W, H);
    text += buf;
    text += "event\tcam\tframe\tname\tstate\tindex\trated_rows\toff_rows\tstale_rows\tfirst_stale\tlast_stale\trated_cols\toff_cols\t"
            "first_off_row\tlast_off_row\tfirst_off_col\tlast_off_col\tlevel_milli\tkind\n";
    struct Cam {
        long long frames = 0, kind[K] = {};
        const std::string *first = nullptr;
        std::vector<long long> perRow, perCol; // the frames in which the line was off or stale
    };
    std::vector<Cam> cams(models.size());
    std::vector<uint8_t> rowState((size_t)std::max(H, 0)), colState((size_t)std::max(W, 0));
    const auto orDash = [](int v) { return v < 0 ? std::string("-") : std::to_string(v); };
    for (const SurveyRow &r : rows) {
        rowPrefix(text, r);
        const SurveyModel *m = (size_t)r.cam < models.size() ? &models[(size_t)r.cam] : nullptr;
        if (r.state != SurveyRow::Ok || !r.has(SurveyLinesProduct) || !m || r.linesRows.size() != (size_t)H * LinesRowWords ||
            r.linesCols.size() != (size_t)W * LinesColWords || m->linesRows.size() != (size_t)H * LinesModelWords ||
            m->linesCols.size() != (size_t)W * LinesModelWords) {
            text += "\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\n";
            continue;
        }
        const LinesFrame f = linesFrame(r.linesRows.data(), r.linesCols.data(), m->linesRows.data(), m->linesCols.data(), W, H, r.linesRef,
                                        rowState.data(), colState.data());
        Cam &c = cams[(size_t)r.cam];
        c.perRow.resize((size_t)H, 0);
        c.perCol.resize((size_t)W, 0);
        for (int y = 0; y < H; ++y)
            c.perRow[(size_t)y] += rowState[(size_t)y] >= LineOff;
        for (int x = 0; x < W; ++x)
            c.perCol[(size_t)x] += colState[(size_t)x] >= LineOff;
        snprintf(buf, sizeof buf, "\t%lld\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%s\t%s\t%s\t%s\t%lld\t%s\n", c.frames, f.ratedRows, f.offRows, f.staleRows,
                 orDash(f.firstStale).c_str(), orDash(f.lastStale).c_str(), f.ratedCols, f.offCols, orDash(f.firstOffRow).c_str(),
                 orDash(f.lastOffRow).c_str(), orDash(f.firstOffCol).c_str(), orDash(f.lastOffCol).c_str(), f.levelMilli, kinds[f.kind]);
        text += buf;
        ++c.frames;
        ++c.kind[f.kind];
        if (f.kind != LinesFrame::Steady && f.kind != LinesFrame::Blind && !c.first)
            c.first = &r.event;
    }
    long long frames = 0, kind[K] = {};
    for (size_t c = 0; c < cams.size(); ++c) {
        if (!models[c].trained) {
            snprintf(buf, sizeof buf, "lines cam %zu none\n", c);
            text += buf;
            continue;
        }
        snprintf(buf, sizeof buf, "lines cam %zu frames %lld", c, cams[c].frames);
        text += buf;
        for (size_t q = 0; q < K; ++q) {
            snprintf(buf, sizeof buf, " %s %lld", kinds[q], cams[c].kind[q]);
            text += buf;
            kind[q] += cams[c].kind[q];
        }
        text += std::string(" first_changed_event ") + (cams[c].first ? *cams[c].first : std::string("-")) + "\n";
        frames += cams[c].frames;
    }
    for (size_t c = 0; c < cams.size(); ++c) {
        if (!models[c].trained)
            continue;
        const auto changed = [&](const char *word, const std::vector<long long> &per) {
            for (size_t k = 0; k < per.size(); ++k)
                if (per[k]) {
                    snprintf(buf, sizeof buf, "changed cam %zu %s %zu frames %lld\n", c, word, k, per[k]);
                    text += buf;
                }
        };
        changed("row", cams[c].perRow);
        changed("col", cams[c].perCol);
    }
    snprintf(buf, sizeof buf, "run frames %lld", frames);
    text += buf;
    for (size_t q = 0; q < K; ++q) {
        snprintf(buf, sizeof buf, " %s %lld", kinds[q], kind[q]);
        text += buf;
    }
    return text + "\n";
}

std::string ShiftReport(int radius, const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows)
{
    std::string text = "# abub3hs shift 1\n";
    char buf[512];
    snprintf(buf, sizeof buf, "radius %d\n", radius);
    text += buf;
    text += "event\tcam\tframe\tname\tstate\tdx\tdy\tat_edge\tsad0\tsad_best\tgain\n";
    struct Cam {
        long long frames = 0, atZero = 0, shifted = 0, atEdge = 0;
        int maxDx = 0, maxDy = 0;
        const std::string *first = nullptr;
    };
    std::vector<Cam> cams(models.size());
    for (const SurveyRow &r : rows) {
        rowPrefix(text, r);
        if (r.state != SurveyRow::Ok || !r.has(SurveyShiftProduct)) {
            text += "\t-\t-\t-\t-\t-\t-\n";
            continue;
        }
        const ShiftBest &b = r.shift;
        const double gain = b.sad0 ? 1.0 - (double)b.sadBest / (double)b.sad0 : 0.0;
        snprintf(buf, sizeof buf, "\t%d\t%d\t%d\t%" PRIu64 "\t%" PRIu64 "\t%.6f\n", b.dx, b.dy, b.atEdge ? 1 : 0, b.sad0, b.sadBest, gain);
        text += buf;
        Cam &c = cams[(size_t)r.cam];
        ++c.frames;
        const bool moved = b.dx != 0 || b.dy != 0;
        ++(moved ? c.shifted : c.atZero);
        c.atEdge += b.atEdge;
        c.maxDx = std::max(c.maxDx, std::abs(b.dx));
        c.maxDy = std::max(c.maxDy, std::abs(b.dy));
        if (moved && !c.first)
            c.first = &r.event;
    }
    long long frames = 0, shifted = 0, atEdge = 0;
    for (size_t c = 0; c < cams.size(); ++c) {
        if (!models[c].trained) {
            snprintf(buf, sizeof buf, "shift cam %zu none\n", c);
            text += buf;
            continue;
        }
        const Cam &k = cams[c];
        snprintf(buf, sizeof buf, "shift cam %zu frames %lld at_zero %lld shifted %lld at_edge %lld max_abs_dx %d max_abs_dy %d first_shifted_event %s\n",
                 c, k.frames, k.atZero, k.shifted, k.atEdge, k.maxDx, k.maxDy, k.first ? k.first->c_str() : "-");
        text += buf;
        frames += k.frames;
        shifted += k.shifted;
        atEdge += k.atEdge;
    }
    snprintf(buf, sizeof buf, "run frames %lld shifted %lld at_edge %lld\n", frames, shifted, atEdge);
    text += buf;
    return text;
}

const char *SurveyRow::stateName() const
{
    static const char *const names[] = {"ok", "undecodable", "missing", "other_size"};
    return names[state];
}

std::string SurveyReport(const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows)
{
    std::string text = "# abub3hs survey 1\n";
    char buf[512];
    long long modelPixels = 0, sigmaZero = 0;
    for (size_t c = 0; c < models.size(); ++c) {
        const SurveyModel &m = models[c];
        if (!m.trained) {
            snprintf(buf, sizeof buf, "model cam %zu none\n", c);
            text += buf;
            continue;
        }
        snprintf(buf, sizeof buf, "model cam %zu trained %d sigma_zero %lld sigma6_sat %lld sigma_max %d mu_mean %.6f\n", c,
                 m.trainingSetSize, m.sigmaZero, m.sigma6Sat, m.sigmaMax, m.muMean);
        text += buf;
        modelPixels += m.pixels;
        sigmaZero += m.sigmaZero;
    }
    text += "event\tcam\tframe\tname\tstate\tw\th\tmin\tmax\tsum\tsumsq\tn_zero\tn_sat\tn_out\tsum_out\tn_moved\tsum_moved\tmean\tsd\n";
    long long perState[4] = {0, 0, 0, 0};
    std::vector<double> movedShare;
    for (const SurveyRow &r : rows) {
        ++perState[r.state];
        rowPrefix(text, r);
        if (r.state != SurveyRow::Ok && r.state != SurveyRow::OtherSize) {
            text += "\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\n";
            continue;
        }
        const FrameStats &s = r.s;
        snprintf(buf, sizeof buf, "\t%d\t%d\t%u\t%u\t%" PRIu64 "\t%" PRIu64 "\t%u\t%u", r.w, r.h, s.min, s.max, s.sum, s.sumsq, s.nZero,
                 s.nSat);
        text += buf;
        if (r.state == SurveyRow::Ok && (s.flags & ABUB_STAT_F_MODEL))
            snprintf(buf, sizeof buf, "\t%u\t%" PRIu64, s.nOut, s.sumOut);
        else
            snprintf(buf, sizeof buf, "\t-\t-");
        text += buf;
        const double n = (double)r.w * (double)r.h;
        if (r.state == SurveyRow::Ok && (s.flags & ABUB_STAT_F_REF)) {
            snprintf(buf, sizeof buf, "\t%u\t%" PRIu64, s.nMoved, s.sumMoved);
            movedShare.push_back((double)s.nMoved / n);
        } else
            snprintf(buf, sizeof buf, "\t-\t-");
        text += buf;
        const double mean = (double)s.sum / n;
        snprintf(buf, sizeof buf, "\t%.6f\t%.6f\n", mean, std::sqrt(std::max(0.0, (double)s.sumsq / n - mean * mean)));
        text += buf;
    }
    snprintf(buf, sizeof buf, "run frames %zu ok %lld undecodable %lld missing %lld other_size %lld", rows.size(), perState[0], perState[1],
             perState[2], perState[3]);
    text += buf;
    if (modelPixels)
        snprintf(buf, sizeof buf, " sigma_zero_share %.6f", (double)sigmaZero / (double)modelPixels);
    else
        snprintf(buf, sizeof buf, " sigma_zero_share -");
    text += buf;
    if (!movedShare.empty()) { // the median; of an even count the mean of the two in the middle
        std::sort(movedShare.begin(), movedShare.end());
        const size_t k = movedShare.size();
        snprintf(buf, sizeof buf, " moved_share_median %.6f\n", k & 1 ? movedShare[k / 2] : (movedShare[k / 2 - 1] + movedShare[k / 2]) / 2);
    } else
        snprintf(buf, sizeof buf, " moved_share_median -\n");
    text += buf;
    return text;
}

namespace {

// The per-pixel planes of a survey on the host: per camera six u32 planes of P words, there only once a host thread has a
// row of the camera to add (the device route keeps its own on the device and adds these at the end)
struct HostPlanes {
    size_t P = 0;
    std::vector<std::vector<uint32_t>> cam;
    std::unique_ptr<std::once_flag[]> once;
    std::atomic<long long> rows{0};
    HostPlanes(size_t cams, size_t pixels) : P(pixels), cam(cams), once(new std::once_flag[cams]) {}
    void add(int c, const uint8_t *cur, const uint8_t *ref, const uint8_t *mu, const uint8_t *sigma6)
    {
        std::call_once(once[c], [&] { cam[c].assign(6 * P, 0u); });
        activityAddHost(cam[c].data(), cur, ref, mu, sigma6, P);
        ++rows;
    }
};

// The part of a survey that is not its frames' pixels
struct CellGrid { // abub_frame_cells_grid's answer
    int ncx = 0, ncy = 0, x0 = 0, y0 = 0;
    size_t cells() const { return (size_t)ncx * ncy; }
};
struct Plan {
    HostPlanes *planes = nullptr;   // with a planes directory: where surveyFrame adds its ok rows
    bool want[SurveyProducts] = {false, false, false, false, false, false}; // the products surveyFrame makes of its ok rows with a model
    int shiftR = 0, cellR = 0;      // the shift search's radius; the radius of the grid and of the field's per-cell search
    CellGrid grid;                  // the one grid of the field, the light, the focus and the noise (all zero: none asked for, or no size)
    std::atomic<long long> *hostUs = nullptr; // [SurveyProducts]: where surveyFrame adds the microseconds it spent in a definition
    std::vector<std::string> events;
    std::vector<SurveyRow> rows;    // in event, camera and frame order
    std::vector<size_t> ref;        // ref[i]: the row frame i is measured against (frame max(i - 2, 0) of its stack)
    std::vector<uint8_t> listed;    // listed[i]: the run lists the frame (0: a missing row); fixed once the plan is made
    int W = 0, H = 0;               // the run's size: that of the first frame that decodes (0: none does)
    std::vector<SurveyModel> models;
    std::vector<const uint8_t *> mu; // per camera: the model's mean plane, null without a model of the run's size
    std::vector<std::vector<uint8_t>> sigma6;
};

// is the format one %d (the camera) followed by one %u (the frame number), with no other conversion?
bool formatTakesCamAndNumber(const std::string &format)
{
    const size_t d = format.find("%d"), u = format.find("%u");
    return d != std::string::npos && u != std::string::npos && d < u && std::count(format.begin(), format.end(), '%') == 2 &&
           format.size() < 128;
}

// the number the name carries for camera `cam`, -1 if it is not of the run's format
long long frameNumberOf(const std::string &name, const std::string &format, int cam)
{
    int c = -1;
    unsigned k = 0;
    if (!formatTakesCamAndNumber(format) || sscanf(name.c_str(), format.c_str(), &c, &k) != 2 || c != cam)
        return -1;
    char back[256];
    snprintf(back, sizeof back, format.c_str(), c, k);
    return name == back ? (long long)k : -1;
}

Plan planRun(Parser *parser, const std::vector<Trainer *> &trainers, int numCams, const std::string &format)
{
    Plan pl;
    pl.events = sortedEvents(*parser);
    struct Stack {
        size_t ev;
        int cam;
        std::vector<std::string> names;
    };
    std::vector<Stack> stacks;
    std::set<long long> numbers; // every frame number a stack of the run has
    for (size_t e = 0; e < pl.events.size(); ++e)
        for (int c = 0; c < numCams; ++c) {
            Stack st{e, c, {}};
            parser->ParseAndSortFramesInFolder(pl.events[e], c, st.names);
            for (const std::string &n : st.names)
                if (frameNumberOf(n, format, c) >= 0)
                    numbers.insert(frameNumberOf(n, format, c));
            stacks.push_back(std::move(st));
        }
    for (Stack &st : stacks) {
        if (st.names.empty())
            continue;
        const std::set<std::string> listed(st.names.begin(), st.names.end());
        std::set<std::string> all = listed; // (sorted as the parsers sort: by name)
        for (long long k : numbers) {
            char name[256];
            snprintf(name, sizeof name, format.c_str(), st.cam, (unsigned)k);
            all.insert(name);
        }
        const size_t first = pl.rows.size();
        int at = 0;
        for (const std::string &n : all) {
            SurveyRow r;
            r.ev = st.ev;
            r.event = pl.events[st.ev];
            r.name = n;
            r.cam = st.cam;
            r.frame = at;
            r.state = listed.count(n) ? SurveyRow::Ok : SurveyRow::Missing;
            pl.listed.push_back(r.state == SurveyRow::Ok);
            pl.rows.push_back(std::move(r));
            pl.ref.push_back(first + (size_t)std::max(at - 2, 0));
            ++at;
        }
    }
    std::vector<FrameTask> tasks;
    for (const SurveyRow &r : pl.rows)
        if (r.state != SurveyRow::Missing)
            tasks.push_back(FrameTask{r.ev, r.name});
    if (!firstFrameSize(parser, pl.events, tasks, pl.W, pl.H))
        pl.W = pl.H = 0;
    pl.models.resize((size_t)numCams);
    pl.mu.assign((size_t)numCams, nullptr);
    pl.sigma6.resize((size_t)numCams);
    const size_t P = (size_t)pl.W * pl.H;
    for (int c = 0; c < numCams && c < (int)trainers.size(); ++c) {
        const Trainer *t = trainers[c];
        if (!t || t->StatusCode || !P || t->TrainedAvgImage.cols != pl.W || t->TrainedAvgImage.rows != pl.H ||
            t->TrainedSigmaImage.cols != pl.W || t->TrainedSigmaImage.rows != pl.H)
            continue;
        SurveyModel &m = pl.models[c];
        m.trained = true;
        m.trainingSetSize = t->TrainingSetSize;
        m.pixels = (long long)P;
        pl.mu[c] = t->TrainedAvgImage.data;
        pl.sigma6[c].resize(P);
        unsigned long long muSum = 0;
        for (size_t i = 0; i < P; ++i) {
            const int sg = t->TrainedSigmaImage.data[i];
            pl.sigma6[c][i] = (uint8_t)std::min(6 * sg, 255);
            m.sigmaZero += sg == 0;
            m.sigma6Sat += 6 * sg >= 255;
            m.sigmaMax = std::max(m.sigmaMax, sg);
            muSum += t->TrainedAvgImage.data[i];
        }
        m.muMean = (double)muSum / (double)P;
    }
    return pl;
}

// a listed frame decoded by the host decoder; empty if it does not decode
cv::Mat decodeRow(Parser &p, const Plan &pl, size_t i)
{
    static thread_local std::vector<unsigned char> file;
    readWhole(p, pl.events[pl.rows[i].ev], pl.rows[i].name, file);
    return file.empty() ? cv::Mat() : cv::imdecode(file.data(), file.size(), 0);
}

// a row's records from its cells' surfaces ([cells][(2 R + 1)^2]), whichever route made them
void fieldRecords(const Plan &pl, const uint32_t *sad, SurveyRow &row)
{
    const size_t N = (2 * (size_t)pl.cellR + 1) * (2 * (size_t)pl.cellR + 1);
    row.field.resize(pl.grid.cells() * FieldRecordWords);
    for (size_t k = 0; k < pl.grid.cells(); ++k)
        fieldCell(sad + k * N, pl.cellR, row.field.data() + k * FieldRecordWords);
}

// The products of an ok row of a camera with a model on this thread: each one's definition and where its result goes, under
// one clock
// (other: the row's decoded reference frame where that is another row, ok and of the run's size, else null: no noise record)
void productsHost(const Plan &pl, const uint8_t *cur, const uint8_t *other, const uint8_t *mu, SurveyRow &row)
{
    const auto timed = [&](SurveyProduct p, auto make) {
        if (!pl.want[p])
            return;
        const double t0 = nowMs();
        make();
        row.set(p, SurveyRow::Host);
        pl.hostUs[p] += (long long)((nowMs() - t0) * 1e3);
    };
    const CellGrid &g = pl.grid;
    timed(SurveyShiftProduct, [&] {
        const size_t D = 2 * (size_t)pl.shiftR + 1;
        std::vector<uint64_t> sad(D * D);
        frameShiftHost(cur, mu, pl.W, pl.H, pl.shiftR, sad.data());
        row.shift = shiftBest(sad.data(), pl.shiftR); // (the one tie rule)
    });
    timed(SurveyFieldProduct, [&] {
        const size_t N = (2 * (size_t)pl.cellR + 1) * (2 * (size_t)pl.cellR + 1);
        std::vector<uint32_t> sad(g.cells() * N);
        fieldCellsHost(cur, mu, pl.W, pl.H, pl.cellR, sad.data());
        fieldRecords(pl, sad.data(), row);
    });
    timed(SurveyLightProduct, [&] {
        row.light.resize(g.cells() * LightRecordWords);
        lightCellsHost(cur, mu, pl.W, pl.H, g.x0, g.y0, g.ncx, g.ncy, row.light.data());
    });
    timed(SurveyFocusProduct, [&] {
        row.focus.resize(g.cells() * FocusRecordWords);
        focusCellsHost(cur, mu, pl.W, pl.H, g.x0, g.y0, g.ncx, g.ncy, row.focus.data());
    });
    if (other)
        timed(SurveyNoiseProduct, [&] {
            row.noise.resize(g.cells() * NoiseRecordWords);
            noiseCellsHost(cur, other, pl.sigma6[row.cam].data(), pl.W, pl.H, g.x0, g.y0, g.ncx, g.ncy, row.noise.data());
        });
    timed(SurveyLinesProduct, [&] { // (without the other frame: no reference, words 3 and 4 are 0)
        row.linesRows.resize((size_t)pl.H * LinesRowWords);
        row.linesCols.resize((size_t)pl.W * LinesColWords);
        row.linesRef = other != nullptr;
        linesHost(cur, other, mu, pl.W, pl.H, row.linesRows.data(), row.linesCols.data());
    });
}

// The host route's per-frame function: row i on this thread, its state and its record.  It asks nothing of the other rows:
// the reference frame is decoded here as well, and is there iff its own row is ok
void surveyFrame(Parser &p, const Plan &pl, size_t i, SurveyRow &row)
{
    row.onKernel = false;
    row.made = 0;
    row.s = FrameStats();
    row.w = row.h = 0;
    if (row.state == SurveyRow::Missing)
        return;
    const cv::Mat cur = decodeRow(p, pl, i);
    if (cur.empty()) {
        row.state = SurveyRow::Undecodable;
        return;
    }
    row.w = cur.cols;
    row.h = cur.rows;
    const size_t n = (size_t)cur.cols * cur.rows;
    if (cur.cols != pl.W || cur.rows != pl.H) {
        row.state = SurveyRow::OtherSize;
        row.s = frameStatsHost(cur.data, nullptr, nullptr, nullptr, n);
        return;
    }
    row.state = SurveyRow::Ok;
    const uint8_t *mu = pl.mu[row.cam];
    cv::Mat ref;
    const size_t ri = pl.ref[i];
    if (mu && ri != i && pl.listed[ri]) {
        ref = decodeRow(p, pl, ri);
        if (!ref.empty() && (ref.cols != pl.W || ref.rows != pl.H))
            ref = cv::Mat();
    }
    const uint8_t *r = ri == i ? cur.data : ref.empty() ? nullptr : ref.data;
    row.s = frameStatsHost(cur.data, r, mu, mu ? pl.sigma6[row.cam].data() : nullptr, n);
    if (pl.planes)
        pl.planes->add(row.cam, cur.data, r, mu, mu ? pl.sigma6[row.cam].data() : nullptr);
    if (mu)
        productsHost(pl, cur.data, ri != i && !ref.empty() ? ref.data : nullptr, mu, row);
}

void hostFrames(Parser *parser, Plan &pl, int nthreads)
{
    forEachTask(parser, nthreads, pl.rows.size(), [&](Parser &p, size_t i) { surveyFrame(p, pl, i, pl.rows[i]); });
}

FrameStats fromRecord(const abub_stat_result &r)
{
    FrameStats s;
    s.min = r.min;
    s.max = r.max;
    s.nZero = r.n_zero;
    s.nSat = r.n_sat;
    s.nOut = r.n_out;
    s.nMoved = r.n_moved;
    s.flags = r.flags;
    s.sum = r.sum;
    s.sumsq = r.sumsq;
    s.sumOut = r.sum_out;
    s.sumMoved = r.sum_moved;
    return s;
}

// The device route: the rows in batches, every leg on the one stream and synchronised before the next.  Per batch: the
// reference frames of its first rows that lie in front of it take the first slots (they are read again), then the rows; the
// pool reads the files into a pinned buffer; upload; the decoders into the slab, slot s at s * align16(W * H).  A row that is
// not in place goes to surveyFrame.  Every row in place is in the slab, whichever decoder or thread put it there, so the
// legs below take all of them.  In order:
// * stats: one abub_frame_stats_dev launch over the rows in place, [jobs][records] in the meta buffer, the records back in
//   one copy.  The list of the jobs that have a model is made from them once, as one abub_shift_job array, and uploaded once
//   (mu is resident already); the four product legs read it.
// * shift, field, light, focus, each only if asked for: one helper (`leg`) launches the product's entry over that list
//   (the noise's over a list of its own, the stats jobs as they are of the rows whose reference frame is another frame in place),
//   copies [status words][payloads] back from the one buffer pair the legs share, checks the status words and hands every
//   row its payload.  The shift's payload is a u64 surface, read by shiftBest; the field's are the cells' u32 surfaces, read
//   by fieldRecords, in calls of as many jobs as keep them below 64 MiB (ABUB_FIELD_CHUNK=n: of n jobs), a call reading the
//   list from its first job on; the light's and the focus' are the cells' records as they are (24 and 20 bytes per cell).
// * activity, with pl.planes: the rows in place are added to the per-pixel planes on the device, [camera][6][stride] u32
//   cleared once: one abub_pixel_activity_dev call per camera that has rows in place, its jobs behind the records in the
//   meta buffer; the planes come back in one copy at the end, into devPlanes.  A row in place whose file no GPU decoder reads
//   was decoded by a reading thread; its pixels are on the host, and it is added to the host planes there, not by the kernel.
void deviceFrames(Parser *parser, Plan &pl, int nthreads, int device, SurveyStats &st, std::vector<uint32_t> &devPlanes)
{
    HIPOK(hipSetDevice(device));
    size_t perBatch = framesPerBatch(device);
    if (const char *e = getenv("ABUB_SURVEY_BATCH"))
        if (atoi(e) > 0)
            perBatch = (size_t)atoi(e);
    const int W = pl.W, H = pl.H;
    const size_t P = (size_t)W * H, stride = (P + 15) & ~(size_t)15, C = pl.mu.size();
    FileBatch B;
    B.sizer.reset(parser->clone());
    PinnedBuffer h_meta, h_jobs, h_leg;
    DeviceBuffer d_meta, d_jobsBuf, d_leg, d_model; // d_model: [mu of every camera][sigma6 of every camera], camera c at c * stride
    Stream stream;
    hipStream_t cs = stream.get();
    bool anyModel = false;
    d_model.grow(2 * C * stride + 16);
    for (size_t c = 0; c < C; ++c)
        if (pl.mu[c]) {
            anyModel = true;
            HIPOK(hipMemcpyAsync(d_model.get() + c * stride, pl.mu[c], P, hipMemcpyHostToDevice, cs));
            HIPOK(hipMemcpyAsync(d_model.get() + (C + c) * stride, pl.sigma6[c].data(), P, hipMemcpyHostToDevice, cs));
        }
    const bool wantPlanes = pl.planes != nullptr;
    DeviceBuffer d_planes;
    if (wantPlanes) {
        d_planes.allocate(C * 6 * stride * sizeof(uint32_t));
        HIPOK(hipMemsetAsync(d_planes.get(), 0, C * 6 * stride * sizeof(uint32_t), cs));
    }
    HIPOK(hipStreamSynchronize(cs));

    for (size_t i0 = 0; i0 < pl.rows.size(); i0 += perBatch) {
        const size_t n = std::min(perBatch, pl.rows.size() - i0);
        // ---- read -------------------------------------------------------------------------------------------------------
        double t0 = nowMs();
        std::vector<size_t> again; // rows in front of the batch that rows of it refer to and that were ok: at most two
        for (size_t i = i0; i < i0 + n; ++i)
            if (pl.ref[i] < i0 && pl.rows[pl.ref[i]].state == SurveyRow::Ok && (again.empty() || again.back() != pl.ref[i]))
                again.push_back(pl.ref[i]);
        const size_t k = again.size(), slots = k + n;
        const auto rowOf = [&](size_t s) { return s < k ? again[s] : i0 + (s - k); };
        B.begin();
        B.reset(slots, slots * stride);
        for (size_t s = 0; s < slots; ++s) {
            const SurveyRow &r = pl.rows[rowOf(s)];
            B.plan((int)s, 0, r.event, r.name, pl.listed[rowOf(s)] != 0);
        }
        B.ready();
        const auto readOne = [&](Parser &p, size_t s) {
            const SurveyRow &r = pl.rows[rowOf(s)];
            B.read(p, s, r.event, r.name, W, H);
        };
        forEachTask(parser, nthreads, slots, readOne);
        B.inflate(parser, nthreads, cs, readOne);
        st.gpuUnzipped += B.unzip.unzipped;
        st.reread += (long long)k;
        st.read_s += (nowMs() - t0) * 1e-3;

        // ---- upload and decode ------------------------------------------------------------------------------------------
        t0 = nowMs();
        B.upload(cs);
        B.launch(0, slots, W, H, [&](int s, int) { return (uint64_t)s * stride; }, cs);
        HIPOK(hipStreamSynchronize(cs));
        B.finish(W, H, cs);
        HIPOK(hipStreamSynchronize(cs));
        st.gpuPngDecoded = B.decodedBy[GpuPng];
        st.gpuUnpacked = B.decodedBy[GpuPacked];
        st.gpuBmpDecoded = B.decodedBy[GpuBmp];
        st.hostDecoded = B.hostDecoded;
        st.decode_s += (nowMs() - t0) * 1e-3;

        // ---- measure: [jobs][results] in one buffer ----------------------------------------------------------------------
        t0 = nowMs();
        std::vector<size_t> slot; // the slots of the batch's rows that are in place
        for (size_t s = k; s < slots; ++s)
            if (B.good[s])
                slot.push_back(s);
        const size_t nj = slot.size();
        if (nj) {
            // [stat jobs][records]; with planes behind them [activity jobs, camera by camera][one status word per camera]
            const size_t statBytes = nj * (sizeof(abub_stat_job) + sizeof(abub_stat_result));
            const size_t metaBytes = statBytes + (wantPlanes ? nj * sizeof(abub_act_job) + C * sizeof(uint32_t) : 0);
            h_meta.grow(metaBytes);
            d_meta.grow(metaBytes);
            abub_stat_job *jobs = (abub_stat_job *)h_meta.get();
            for (size_t g = 0; g < nj; ++g) {
                const size_t i = rowOf(slot[g]), ri = pl.ref[i];
                // the reference frame's slot: in the batch, or among the frames read again
                size_t rs = slots;
                if (ri >= i0)
                    rs = k + (ri - i0);
                else
                    for (size_t a = 0; a < k; ++a)
                        if (again[a] == ri)
                            rs = a;
                jobs[g].cur = (uint64_t)slot[g] * stride;
                jobs[g].ref = rs < slots && B.good[rs] ? (uint64_t)rs * stride : UINT64_MAX;
                jobs[g].model = pl.mu[pl.rows[i].cam] ? (uint64_t)pl.rows[i].cam * stride : UINT64_MAX;
            }
            HIPOK(hipMemcpyAsync(d_meta.get(), h_meta.get(), nj * sizeof(abub_stat_job), hipMemcpyHostToDevice, cs));
            abub_stat_result *d_res = (abub_stat_result *)(d_meta.get() + nj * sizeof(abub_stat_job));
            const abub_stat_result *res = (const abub_stat_result *)(h_meta.get() + nj * sizeof(abub_stat_job));
            check(abub_frame_stats_dev(B.slab.get(), slots * stride, anyModel ? d_model.get() : nullptr, d_model.get() + C * stride,
                                       C * stride, (const abub_stat_job *)d_meta.get(), (int)nj, P, d_res, cs),
                  "abub_frame_stats_dev");
            HIPOK(hipMemcpyAsync(h_meta.get() + nj * sizeof(abub_stat_job), d_res, nj * sizeof(abub_stat_result), hipMemcpyDeviceToHost, cs));
            HIPOK(hipStreamSynchronize(cs));
            // ---- the products of the jobs that have a model: one job list, one leg per product ------------------------------
            std::vector<size_t> with; // the jobs that have a model
            for (size_t g = 0; g < nj; ++g)
                if (jobs[g].model != UINT64_MAX)
                    with.push_back(g);
            // (the noise pairs a row with its reference frame: of those, the jobs whose reference is another frame, in place; the
            // offsets are the stats jobs' own, the reference among the batch's rows or among the frames read again)
            std::vector<size_t> paired;
            if (pl.want[SurveyNoiseProduct])
                for (size_t g : with)
                    if (jobs[g].ref != UINT64_MAX && jobs[g].ref != jobs[g].cur)
                        paired.push_back(g);
            // (the lines take every job that has a model, its reference where that is another frame in place, else none)
            const size_t ns = with.size(), nn = paired.size(), nl = pl.want[SurveyLinesProduct] ? ns : 0;
            const abub_shift_job *d_jobs = nullptr;
            const abub_stat_job *d_pairs = nullptr; // behind the with-model list in the same buffer
            const abub_stat_job *d_lines = nullptr; // behind the pairs
            if (ns && (pl.want[SurveyShiftProduct] || pl.want[SurveyFieldProduct] || pl.want[SurveyLightProduct] || pl.want[SurveyFocusProduct] ||
                       nn || nl)) {
                const size_t bytes = ns * sizeof(abub_shift_job) + (nn + nl) * sizeof(abub_stat_job);
                h_jobs.grow(bytes);
                d_jobsBuf.grow(bytes);
                abub_shift_job *sj = (abub_shift_job *)h_jobs.get();
                for (size_t q = 0; q < ns; ++q)
                    sj[q] = abub_shift_job{jobs[with[q]].cur, jobs[with[q]].model};
                abub_stat_job *nj3 = (abub_stat_job *)(h_jobs.get() + ns * sizeof(abub_shift_job));
                for (size_t q = 0; q < nn; ++q)
                    nj3[q] = jobs[paired[q]];
                for (size_t q = 0; q < nl; ++q) {
                    nj3[nn + q] = jobs[with[q]];
                    if (nj3[nn + q].ref == nj3[nn + q].cur)
                        nj3[nn + q].ref = UINT64_MAX;
                }
                HIPOK(hipMemcpyAsync(d_jobsBuf.get(), h_jobs.get(), bytes, hipMemcpyHostToDevice, cs));
                d_jobs = (const abub_shift_job *)d_jobsBuf.get();
                d_pairs = (const abub_stat_job *)(d_jobsBuf.get() + ns * sizeof(abub_shift_job));
                d_lines = d_pairs + nn;
            }
            const auto rowWith = [&](size_t q) -> SurveyRow & { return pl.rows[rowOf(slot[with[q]])]; };
            // One leg: `entry` over the `ns` jobs of `list` (indices into the stats jobs) in calls of `chunk` (0: all of them in
            // one; no job: no call), each call's status words and payloads ([status, padded to 8 bytes][payloadBytes per job], the
            // one buffer pair of all legs, which synchronise one after another) back in one copy; launch(q0, n, ...) runs the
            // entry over the list's jobs from q0 on, take(q, payload) gets what job q's row is given (a take of four arguments:
            // (q, the call's payloads, the job's place in the call, the call's jobs), for an entry whose payloads are not one run per job)
            const auto leg = [&](SurveyProduct p, const char *entry, const std::vector<size_t> &list, size_t payloadBytes, size_t chunk,
                                 auto launch, auto take) {
                if (!pl.want[p])
                    return;
                const size_t ns = list.size();
                st.stats_s += (nowMs() - t0) * 1e-3;
                t0 = nowMs();
                for (size_t q0 = 0; q0 < ns; q0 += chunk ? chunk : ns) {
                    const size_t n = std::min(chunk ? chunk : ns, ns - q0);
                    const size_t statusBytes = (n * sizeof(uint32_t) + 7) & ~(size_t)7, bytes = statusBytes + n * payloadBytes;
                    h_leg.grow(bytes);
                    d_leg.grow(bytes);
                    check(launch(q0, (int)n, (uint32_t *)d_leg.get(), d_leg.get() + statusBytes), entry);
                    HIPOK(hipMemcpyAsync(h_leg.get(), d_leg.get(), bytes, hipMemcpyDeviceToHost, cs));
                    HIPOK(hipStreamSynchronize(cs));
                    for (size_t q = 0; q < n; ++q) {
                        if (((const uint32_t *)h_leg.get())[q] != 0)
                            throw std::runtime_error(std::string("survey: ") + entry + " refused a frame of its own slab");
                        // (a take of four arguments gets the call's payloads whole, the job's place in the call and the call's size)
                        if constexpr (std::is_invocable_v<decltype(take), size_t, const uint8_t *, size_t, size_t>)
                            take(q0 + q, (const uint8_t *)h_leg.get() + statusBytes, q, n);
                        else
                            take(q0 + q, h_leg.get() + statusBytes + q * payloadBytes);
                        pl.rows[rowOf(slot[list[q0 + q]])].set(p, SurveyRow::Kernel);
                    }
                    ++st.product[p].launches;
                }
                st.product[p].leg_s += (nowMs() - t0) * 1e-3;
                t0 = nowMs();
            };
            const uint8_t *slab = B.slab.get(), *d_mu = d_model.get();
            const size_t slabBytes = slots * stride, muBytes = C * stride;
            const CellGrid &cg = pl.grid;
            const size_t shiftN = (2 * (size_t)pl.shiftR + 1) * (2 * (size_t)pl.shiftR + 1);
            leg(SurveyShiftProduct, "abub_frame_shift_dev", with, shiftN * sizeof(uint64_t), 0,
                [&](size_t q0, int n, uint32_t *status, uint8_t *sad) {
                    return abub_frame_shift_dev(slab, slabBytes, d_mu, muBytes, d_jobs + q0, n, W, H, pl.shiftR, status, (uint64_t *)sad, cs);
                },
                [&](size_t q, const uint8_t *sad) { rowWith(q).shift = shiftBest((const uint64_t *)sad, pl.shiftR); });
            // (a job's surfaces depend on nothing but the job, so the split cannot show in the result)
            const size_t fieldWords = cg.cells() * (2 * (size_t)pl.cellR + 1) * (2 * (size_t)pl.cellR + 1);
            size_t fieldChunk = std::max<size_t>(1, ((size_t)64 << 20) / std::max<size_t>(1, fieldWords * sizeof(uint32_t)));
            if (const char *e = getenv("ABUB_FIELD_CHUNK")) // (a test knob)
                if (atoi(e) > 0)
                    fieldChunk = (size_t)atoi(e);
            leg(SurveyFieldProduct, "abub_frame_shift_cells_dev", with, fieldWords * sizeof(uint32_t), fieldChunk,
                [&](size_t q0, int n, uint32_t *status, uint8_t *sad) {
                    return abub_frame_shift_cells_dev(slab, slabBytes, d_mu, muBytes, d_jobs + q0, n, W, H, pl.cellR, status, (uint32_t *)sad,
                                                      cs);
                },
                [&](size_t q, const uint8_t *sad) { fieldRecords(pl, (const uint32_t *)sad, rowWith(q)); });
            leg(SurveyLightProduct, "abub_frame_light_cells_dev", with, cg.cells() * LightRecordWords * sizeof(uint32_t), 0,
                [&](size_t q0, int n, uint32_t *status, uint8_t *rec) {
                    return abub_frame_light_cells_dev(slab, slabBytes, d_mu, muBytes, d_jobs + q0, n, W, H, cg.x0, cg.y0, cg.ncx, cg.ncy,
                                                      status, (uint32_t *)rec, cs);
                },
                [&](size_t q, const uint8_t *rec) {
                    rowWith(q).light.assign((const uint32_t *)rec, (const uint32_t *)rec + cg.cells() * LightRecordWords);
                });
            leg(SurveyFocusProduct, "abub_frame_focus_cells_dev", with, cg.cells() * FocusRecordWords * sizeof(int32_t), 0,
                [&](size_t q0, int n, uint32_t *status, uint8_t *rec) {
                    return abub_frame_focus_cells_dev(slab, slabBytes, d_mu, muBytes, d_jobs + q0, n, W, H, cg.x0, cg.y0, cg.ncx, cg.ncy,
                                                      status, (int32_t *)rec, cs);
                },
                [&](size_t q, const uint8_t *rec) {
                    rowWith(q).focus.assign((const int32_t *)rec, (const int32_t *)rec + cg.cells() * FocusRecordWords);
                });
            leg(SurveyNoiseProduct, "abub_frame_noise_cells_dev", paired, cg.cells() * NoiseRecordWords * sizeof(int32_t), 0,
                [&](size_t q0, int n, uint32_t *status, uint8_t *rec) { // (sigma6 lies behind mu: camera c at (C + c) * stride)
                    return abub_frame_noise_cells_dev(slab, slabBytes, d_mu + C * stride, muBytes, d_pairs + q0, n, W, H, cg.x0, cg.y0, cg.ncx,
                                                      cg.ncy, status, (int32_t *)rec, cs);
                },
                [&](size_t q, const uint8_t *rec) {
                    pl.rows[rowOf(slot[paired[q]])].noise.assign((const int32_t *)rec, (const int32_t *)rec + cg.cells() * NoiseRecordWords);
                });
            // (as the field: in calls of as many jobs as keep the payloads below 64 MiB, or of the field's knob)
            const size_t linesBytes = ((size_t)H * LinesRowWords + (size_t)W * LinesColWords) * sizeof(uint32_t);
            size_t linesChunk = std::max<size_t>(1, ((size_t)64 << 20) / linesBytes);
            if (const char *e = getenv("ABUB_FIELD_CHUNK"))
                if (atoi(e) > 0)
                    linesChunk = (size_t)atoi(e);
            leg(SurveyLinesProduct, "abub_frame_lines_dev", with, linesBytes, linesChunk,
                [&](size_t q0, int n, uint32_t *status, uint8_t *rec) { // ([rows of all n jobs][cols of all n jobs] behind the status words)
                    return abub_frame_lines_dev(slab, slabBytes, d_mu, muBytes, d_lines + q0, n, W, H, status, (uint32_t *)rec,
                                                (uint32_t *)rec + (size_t)n * H * LinesRowWords, cs);
                },
                [&](size_t q, const uint8_t *call, size_t in, size_t n) { // (job `in` of a call of n: the rows of all, then the columns)
                    const uint32_t *all = (const uint32_t *)call;
                    const uint32_t *rws = all + in * H * LinesRowWords, *cls = all + n * H * LinesRowWords + in * W * LinesColWords;
                    SurveyRow &row = rowWith(q);
                    row.linesRows.assign(rws, rws + (size_t)H * LinesRowWords);
                    row.linesCols.assign(cls, cls + (size_t)W * LinesColWords);
                    row.linesRef = jobs[with[q]].ref != UINT64_MAX && jobs[with[q]].ref != jobs[with[q]].cur;
                });
            if (wantPlanes) {
                st.stats_s += (nowMs() - t0) * 1e-3;
                t0 = nowMs();
                // A frame that no GPU decoder reads was decoded by a reading thread, and its pixels are still on the host
                // (B.fd.hostPix): its row is the device route's host share and is added there; every other row is a job
                std::vector<int> hostOf(slots, -1);
                for (size_t q = 0; q < B.fd.host.size(); ++q)
                    if (B.fd.hostPix[q].size() == P)
                        hostOf[(size_t)B.fd.host[q].s] = (int)q;
                std::vector<size_t> onHost;
                abub_act_job *aj = (abub_act_job *)(h_meta.get() + statBytes);
                std::vector<size_t> first(C + 1, 0), at(C);
                for (size_t g = 0; g < nj; ++g)
                    if (hostOf[slot[g]] >= 0)
                        onHost.push_back(g);
                    else
                        ++first[(size_t)pl.rows[rowOf(slot[g])].cam + 1];
                for (size_t c = 0; c < C; ++c)
                    at[c] = first[c + 1] += first[c];
                for (size_t g = nj; g-- > 0;) // (backwards: a camera's jobs keep the order of the rows)
                    if (hostOf[slot[g]] < 0)
                        aj[--at[(size_t)pl.rows[rowOf(slot[g])].cam]] = abub_act_job{jobs[g].cur, jobs[g].ref};
                HIPOK(hipMemcpyAsync(d_meta.get() + statBytes, aj, nj * sizeof(abub_act_job), hipMemcpyHostToDevice, cs));
                const size_t statusAt = statBytes + nj * sizeof(abub_act_job);
                for (size_t c = 0; c < C; ++c) {
                    ((uint32_t *)(h_meta.get() + statusAt))[c] = 0;
                    if (first[c + 1] == first[c])
                        continue;
                    check(abub_pixel_activity_dev(B.slab.get(), slots * stride, pl.mu[c] ? d_model.get() + c * stride : nullptr,
                                                  pl.mu[c] ? d_model.get() + (C + c) * stride : nullptr,
                                                  (const abub_act_job *)(d_meta.get() + statBytes) + first[c], (int)(first[c + 1] - first[c]),
                                                  P, (uint32_t *)d_planes.get() + c * 6 * stride, stride,
                                                  (uint32_t *)(d_meta.get() + statusAt) + c, cs),
                          "abub_pixel_activity_dev");
                    HIPOK(hipMemcpyAsync(h_meta.get() + statusAt + c * sizeof(uint32_t), d_meta.get() + statusAt + c * sizeof(uint32_t),
                                         sizeof(uint32_t), hipMemcpyDeviceToHost, cs));
                }
                HIPOK(hipStreamSynchronize(cs));
                for (size_t c = 0; c < C; ++c)
                    if (((const uint32_t *)(h_meta.get() + statusAt))[c] != 0)
                        throw std::runtime_error("survey: abub_pixel_activity_dev refused a frame of its own slab");
                st.planeRowsKernel += (long long)first[C];
                // the host share: the reference frame from the host where it was decoded there too, else back from the slab
                std::atomic<int> copyFailed{0};
                forEachTask(parser, nthreads, onHost.size(), [&](Parser &, size_t q) {
                    static thread_local std::vector<uint8_t> back;
                    const size_t g = onHost[q];
                    const int cam = pl.rows[rowOf(slot[g])].cam;
                    const uint8_t *mu = pl.mu[cam], *ref = nullptr;
                    if (mu && jobs[g].ref != UINT64_MAX) {
                        const size_t rs = (size_t)(jobs[g].ref / stride);
                        if (hostOf[rs] >= 0)
                            ref = B.fd.hostPix[(size_t)hostOf[rs]].data();
                        else {
                            back.resize(P);
                            if (hipSetDevice(device) != hipSuccess ||
                                hipMemcpy(back.data(), B.slab.get() + jobs[g].ref, P, hipMemcpyDeviceToHost) != hipSuccess) {
                                copyFailed = 1;
                                return;
                            }
                            ref = back.data();
                        }
                    }
                    pl.planes->add(cam, B.fd.hostPix[(size_t)hostOf[slot[g]]].data(), ref, mu, mu ? pl.sigma6[cam].data() : nullptr);
                });
                if (copyFailed)
                    throw std::runtime_error("survey: a reference frame could not be copied back from the slab");
                st.activity_s += (nowMs() - t0) * 1e-3;
                t0 = nowMs();
            }
            for (size_t g = 0; g < nj; ++g) {
                if (res[g].status != 0)
                    throw std::runtime_error("survey: abub_frame_stats_dev refused a frame of its own slab");
                SurveyRow &row = pl.rows[rowOf(slot[g])];
                row.state = SurveyRow::Ok;
                row.w = W;
                row.h = H;
                row.s = fromRecord(res[g]);
                row.onKernel = true;
            }
        }
        st.stats_s += (nowMs() - t0) * 1e-3;

        // ---- what is not in place (missing, no decoder reads it, another size): the host route's answer ---------------------
        t0 = nowMs();
        std::vector<size_t> left;
        for (size_t s = k; s < slots; ++s)
            if (!B.good[s])
                left.push_back(rowOf(s));
        forEachTask(parser, nthreads, left.size(), [&](Parser &p, size_t q) { surveyFrame(p, pl, left[q], pl.rows[left[q]]); });
        st.read_s += (nowMs() - t0) * 1e-3;
        ++st.batches;
    }
    if (wantPlanes) {
        const double t0 = nowMs();
        devPlanes.resize(C * 6 * stride);
        HIPOK(hipMemcpyAsync(devPlanes.data(), d_planes.get(), devPlanes.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, cs));
        HIPOK(hipStreamSynchronize(cs));
        st.planes_copy_s += (nowMs() - t0) * 1e-3;
    }
}

// The head of a NumPy format 1.0 file of `descr` values in C order, `shape` as Python writes a tuple: the data that follows
// it begins at a multiple of 64
std::string npyHead(const char *descr, const std::string &shape)
{
    std::string head = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': " + shape + ", }";
    head.resize((10 + head.size() + 1 + 63) / 64 * 64 - 10 - 1, ' ');
    head += '\n';
    std::string file("\x93NUMPY\x01\x00", 8);
    file += (char)(head.size() & 0xff);
    file += (char)(head.size() >> 8);
    return file + head;
}

// The files of a per-cell product, one writer for both routes: the directory; per camera with a model cam<c>_<tag>.npy, the
// records (`words` 4-byte values per cell, the row's `rec`) of its rows that have the product in survey order (the `index`
// column of the text), and with modelDescr cam<c>_<tag>_model.npy, the camera's `model` ([ncy][ncx][modelWords]); then
// <tag>.txt.  The records' descr is <i4, for the light's u32 too (none reaches 2^31).
template <class T, class M>
void writeCells(const std::string &dir, const char *tag, SurveyProduct p, const Plan &pl, size_t words, std::vector<T> SurveyRow::*rec,
                const char *modelDescr, size_t modelWords, std::vector<M> SurveyModel::*model, const std::string &text)
{
    static_assert(sizeof(T) == 4, "the records are <i4");
    std::string failed;
    if (!makeDirs(dir, &failed))
        throw std::runtime_error("survey: cannot make the directory " + failed);
    const auto write = [](const std::string &path, const std::string &bytes) {
        if (!writeFile(path, (const unsigned char *)bytes.data(), bytes.size()))
            throw std::runtime_error("survey: cannot write " + path);
    };
    const CellGrid &g = pl.grid;
    for (size_t c = 0; c < pl.models.size(); ++c) {
        if (!pl.models[c].trained)
            continue;
        std::string data;
        size_t n = 0;
        for (const SurveyRow &r : pl.rows)
            if ((size_t)r.cam == c && r.state == SurveyRow::Ok && r.has(p) && (r.*rec).size() == g.cells() * words) {
                data.append((const char *)(r.*rec).data(), (r.*rec).size() * sizeof(T));
                ++n;
            }
        char shape[96];
        snprintf(shape, sizeof shape, "(%zu, %d, %d, %zu)", n, g.ncy, g.ncx, words);
        const std::string stem = dir + "/cam" + std::to_string(c) + "_" + tag;
        write(stem + ".npy", npyHead("<i4", shape) + data);
        if (!modelDescr)
            continue;
        snprintf(shape, sizeof shape, "(%d, %d, %zu)", g.ncy, g.ncx, modelWords);
        const std::vector<M> &m = pl.models[c].*model;
        write(stem + "_model.npy", npyHead(modelDescr, shape) + std::string((const char *)m.data(), m.size() * sizeof(M)));
    }
    write(dir + "/" + tag + ".txt", text);
}

// The files of the per-line product, one writer for both routes: per camera with a model cam<c>_lines_rows.npy and
// cam<c>_lines_cols.npy, the records of its rows that have the product in survey order (the `index` column of the text),
// cam<c>_lines_model_rows.npy and cam<c>_lines_model_cols.npy; then lines.txt.  All <i4 (no value reaches 2^31)
void writeLines(const std::string &dir, const Plan &pl, const std::string &text)
{
    std::string failed;
    if (!makeDirs(dir, &failed))
        throw std::runtime_error("survey: cannot make the directory " + failed);
    const auto write = [](const std::string &path, const std::string &bytes) {
        if (!writeFile(path, (const unsigned char *)bytes.data(), bytes.size()))
            throw std::runtime_error("survey: cannot write " + path);
    };
    const auto bytesOf = [](const std::vector<uint32_t> &v) { return std::string((const char *)v.data(), v.size() * sizeof(uint32_t)); };
    for (size_t c = 0; c < pl.models.size(); ++c) {
        const SurveyModel &m = pl.models[c];
        if (!m.trained)
            continue;
        std::string rowData, colData;
        size_t n = 0;
        for (const SurveyRow &r : pl.rows)
            if ((size_t)r.cam == c && r.state == SurveyRow::Ok && r.has(SurveyLinesProduct) &&
                r.linesRows.size() == (size_t)pl.H * LinesRowWords && r.linesCols.size() == (size_t)pl.W * LinesColWords) {
                rowData += bytesOf(r.linesRows);
                colData += bytesOf(r.linesCols);
                ++n;
            }
        char shape[96];
        const std::string stem = dir + "/cam" + std::to_string(c) + "_lines_";
        snprintf(shape, sizeof shape, "(%zu, %d, %d)", n, pl.H, (int)LinesRowWords);
        write(stem + "rows.npy", npyHead("<i4", shape) + rowData);
        snprintf(shape, sizeof shape, "(%zu, %d, %d)", n, pl.W, (int)LinesColWords);
        write(stem + "cols.npy", npyHead("<i4", shape) + colData);
        snprintf(shape, sizeof shape, "(%d, %d)", pl.H, (int)LinesModelWords);
        write(stem + "model_rows.npy", npyHead("<i4", shape) + bytesOf(m.linesRows));
        snprintf(shape, sizeof shape, "(%d, %d)", pl.W, (int)LinesModelWords);
        write(stem + "model_cols.npy", npyHead("<i4", shape) + bytesOf(m.linesCols));
    }
    write(dir + "/lines.txt", text);
}

// The files of the per-pixel planes, one writer for both routes ("Surveying a run per pixel"): per camera
// with a listed row the sum of the host's planes and the device's (dev: [camera][6][stride], or empty) as
// cam<c>_activity.npy, with a model cam<c>_moved.png, and the cameras' lines of activity.txt
void writePlanes(const std::string &dir, const Plan &pl, const HostPlanes &hp, const std::vector<uint32_t> &dev)
{
    std::string failed;
    if (!makeDirs(dir, &failed))
        throw std::runtime_error("survey: cannot make the directory " + failed);
    const size_t P = (size_t)pl.W * pl.H, stride = (P + 15) & ~(size_t)15;
    std::string text = "# abub3hs activity 1\n";
    char buf[512];
    for (size_t c = 0; c < pl.mu.size(); ++c) {
        bool listed = false;
        unsigned long long frames = 0, framesModel = 0, framesMoved = 0;
        for (size_t i = 0; i < pl.rows.size(); ++i) {
            const SurveyRow &r = pl.rows[i];
            if ((size_t)r.cam != c)
                continue;
            listed = listed || pl.listed[i];
            if (r.state != SurveyRow::Ok)
                continue;
            ++frames;
            framesModel += (r.s.flags & ABUB_STAT_F_MODEL) != 0;
            framesMoved += (r.s.flags & ABUB_STAT_F_REF) != 0;
        }
        if (!listed)
            continue;
        std::vector<uint32_t> v(6 * P, 0u);
        if (!hp.cam[c].empty())
            v = hp.cam[c];
        if (!dev.empty())
            for (size_t k = 0; k < 6; ++k)
                for (size_t i = 0; i < P; ++i)
                    v[k * P + i] += dev[(c * 6 + k) * stride + i];
        const uint32_t *nZero = v.data(), *nSat = nZero + P, *nOut = nSat + P, *sumOut = nOut + P, *nMoved = sumOut + P,
                       *sumMoved = nMoved + P;

        // ---- cam<c>_activity.npy: NumPy format 1.0, the data at a multiple of 64 --------------------------------------------
        snprintf(buf, sizeof buf, "(6, %d, %d)", pl.H, pl.W);
        std::string file = npyHead("<u4", buf);
        file.append((const char *)v.data(), v.size() * sizeof(uint32_t));
        const std::string stem = dir + "/cam" + std::to_string(c);
        if (!writeFile(stem + "_activity.npy", (const unsigned char *)file.data(), file.size()))
            throw std::runtime_error("survey: cannot write " + stem + "_activity.npy");

        // ---- cam<c>_moved.png: the share of the counted rows in which the pixel moved, 255 = all of them --------------------
        if (pl.mu[c]) {
            cv::Mat img(pl.H, pl.W, CV_8U);
            for (size_t i = 0; i < P; ++i)
                img.data[i] = (uint8_t)(framesMoved ? (255ull * nMoved[i] + framesMoved - 1) / framesMoved : 0);
            if (!cv::imwrite(stem + "_moved.png", img))
                throw std::runtime_error("survey: cannot write " + stem + "_moved.png");
        }

        // ---- activity.txt -----------------------------------------------------------------------------------------------------
        snprintf(buf, sizeof buf, "cam %zu w %d h %d frames %llu frames_model %llu frames_moved %llu\n", c, pl.W, pl.H, frames, framesModel,
                 framesMoved);
        text += buf;
        unsigned long long dead = 0, stuck = 0, everOut = 0, everMoved = 0, moved10 = 0, moved50 = 0;
        std::vector<uint32_t> hot;
        for (size_t i = 0; i < P; ++i) {
            dead += frames && nZero[i] == frames;
            stuck += frames && nSat[i] == frames;
            everOut += nOut[i] > 0;
            everMoved += nMoved[i] > 0;
            moved10 += framesMoved && 10ull * nMoved[i] >= framesMoved;
            moved50 += framesMoved && 2ull * nMoved[i] >= framesMoved;
            if (nMoved[i] > 0)
                hot.push_back((uint32_t)i);
        }
        snprintf(buf, sizeof buf, "cam %zu dead %llu stuck_sat %llu ever_out %llu ever_moved %llu moved_10pct %llu moved_50pct %llu\n", c,
                 dead, stuck, everOut, everMoved, moved10, moved50);
        text += buf;
        const size_t nhot = std::min<size_t>(hot.size(), 16);
        std::partial_sort(hot.begin(), hot.begin() + nhot, hot.end(), [&](uint32_t a, uint32_t b) {
            if (nMoved[a] != nMoved[b])
                return nMoved[a] > nMoved[b];
            if (sumMoved[a] != sumMoved[b])
                return sumMoved[a] > sumMoved[b];
            return a < b;
        });
        for (size_t k = 0; k < nhot; ++k) {
            const uint32_t i = hot[k];
            snprintf(buf, sizeof buf, "hot %zu %zu %u %u %u %u %u %u %u %u\n", c, k + 1, i % (uint32_t)pl.W, i / (uint32_t)pl.W, nMoved[i],
                     sumMoved[i], nOut[i], sumOut[i], pl.mu[c][i], pl.sigma6[c][i]);
            text += buf;
        }
    }
    if (!writeFile(dir + "/activity.txt", (const unsigned char *)text.data(), text.size()))
        throw std::runtime_error("survey: cannot write " + dir + "/activity.txt");
}

bool sameDirectory(const std::string &path, const std::string &other)
{
    struct stat a, b;
    return !path.empty() && !other.empty() && stat(path.c_str(), &a) == 0 && stat(other.c_str(), &b) == 0 && a.st_dev == b.st_dev &&
           a.st_ino == b.st_ino;
}

// a directory to write to, trimmed; refused where it is the run that is being read
// (the files have names of their own, but a run directory is not the place for what was derived from it)
std::string outputDir(const std::string &dir, const std::string &srcRunDir)
{
    const std::string d = trimSlashes(dir);
    if (!d.empty() && sameDirectory(trimSlashes(srcRunDir), d))
        throw std::runtime_error("survey: " + d + " is the run that is being read");
    return d;
}

// refuses a run whose frames are too small for `what` ("a shift field", "needs") at `radius`, which takes sides of `need`; a
// run of which no frame decodes has no size to refuse
void needFrames(const Plan &pl, bool enough, const char *what, const char *needs, int radius, int need)
{
    if (pl.W > 0 && !enough)
        throw std::runtime_error(std::string("survey: ") + what + " at radius " + std::to_string(radius) + " " + needs +
                                 " frames of at least " + std::to_string(need) + "x" + std::to_string(need) + ", the run's are " +
                                 std::to_string(pl.W) + "x" + std::to_string(pl.H));
}

} // namespace

int SurveyRun(Parser *parser, const std::vector<Trainer *> &trainers, int numCams, const std::string &format, const SurveyRequest &rq,
              int nthreads, int device, SurveyStats *stats, std::vector<SurveyRow> *rows, std::vector<SurveyModel> *models)
{
    const double t0 = nowMs();
    SurveyStats st;
    if (device >= 0) // (before anything else)
        requireDevice(device, "survey", "; without --survey-gpu the run is surveyed on the host");
    const std::string planesDir = outputDir(rq.planesDir, rq.srcRunDir), fieldDir = outputDir(rq.fieldDir, rq.srcRunDir),
                      lightDir = outputDir(rq.lightDir, rq.srcRunDir), focusDir = outputDir(rq.focusDir, rq.srcRunDir),
                      noiseDir = outputDir(rq.noiseDir, rq.srcRunDir), linesDir = outputDir(rq.linesDir, rq.srcRunDir);
    const bool want[SurveyProducts] = {!rq.shiftPath.empty(), !fieldDir.empty(), !lightDir.empty(), !focusDir.empty(), !noiseDir.empty(),
                                       !linesDir.empty()};
    const bool wantCells = want[SurveyFieldProduct] || want[SurveyLightProduct] || want[SurveyFocusProduct] || want[SurveyNoiseProduct];
    if (wantCells && (rq.cellRadius < 1 || rq.cellRadius > 8))
        throw std::runtime_error("survey: the field radius must be in [1, 8], not " + std::to_string(rq.cellRadius));
    if (want[SurveyShiftProduct] && (rq.shiftRadius < 1 || rq.shiftRadius > 8))
        throw std::runtime_error("survey: the shift radius must be in [1, 8], not " + std::to_string(rq.shiftRadius));
    Plan pl = planRun(parser, trainers, numCams, format);
    std::atomic<long long> hostUs[SurveyProducts];
    for (int p = 0; p < SurveyProducts; ++p) {
        hostUs[p] = 0;
        pl.want[p] = want[p];
    }
    pl.hostUs = hostUs;
    if (want[SurveyShiftProduct]) {
        const int need = 2 * rq.shiftRadius + 1;
        needFrames(pl, pl.W >= need && pl.H >= need, "a shift search", "needs", rq.shiftRadius, need);
        pl.shiftR = rq.shiftRadius;
    }
    if (wantCells) {
        pl.cellR = rq.cellRadius;
        CellGrid &g = pl.grid;
        if (pl.W > 0)
            abub_frame_cells_grid(pl.W, pl.H, pl.cellR, &g.ncx, &g.ncy, &g.x0, &g.y0);
        static const char *const what[SurveyProducts][2] = {
            {nullptr, nullptr}, {"a shift field", "needs"}, {"the light records", "need"}, {"the focus records", "need"},
            {"the noise records", "need"}, {nullptr, nullptr}};
        for (int p = SurveyFieldProduct; p <= SurveyNoiseProduct; ++p) // (the per-cell products)
            if (want[p]) // (a frame without a whole cell)
                needFrames(pl, g.cells() > 0, what[p][0], what[p][1], pl.cellR, ABUB_FIELD_CELL + 2 * pl.cellR);
        // (the model's sums depend on the camera alone: once, here, for both routes)
        for (size_t c = 0; c < pl.models.size(); ++c) {
            SurveyModel &m = pl.models[c];
            if (m.trained && want[SurveyLightProduct]) {
                m.light.resize(g.cells() * LightModelWords);
                lightModelHost(pl.mu[c], pl.sigma6[c].data(), pl.W, pl.H, g.x0, g.y0, g.ncx, g.ncy, m.light.data());
            }
            if (m.trained && want[SurveyFocusProduct]) {
                m.focus.resize(g.cells() * FocusModelWords);
                focusModelHost(pl.mu[c], pl.sigma6[c].data(), pl.W, pl.H, g.x0, g.y0, g.ncx, g.ncy, m.focus.data());
            }
        }
    }
    if (want[SurveyLinesProduct] && pl.W > 0) // (the model's line sums: once per camera, here, for both routes)
        for (size_t c = 0; c < pl.models.size(); ++c) {
            SurveyModel &m = pl.models[c];
            if (!m.trained)
                continue;
            m.linesRows.resize((size_t)pl.H * LinesModelWords);
            m.linesCols.resize((size_t)pl.W * LinesModelWords);
            linesModelHost(pl.mu[c], pl.sigma6[c].data(), pl.W, pl.H, m.linesRows.data(), m.linesCols.data());
        }
    std::unique_ptr<HostPlanes> hostPlanes;
    std::vector<uint32_t> devPlanes;
    if (!planesDir.empty()) {
        std::vector<size_t> perCam((size_t)numCams, 0);
        for (const SurveyRow &r : pl.rows)
            if (++perCam[(size_t)r.cam] > 16777215) // (255 * 2^24 < 2^32: a u32 plane cannot overflow below that)
                throw std::runtime_error("survey: camera " + std::to_string(r.cam) + " has more than 16777215 frames: its planes could overflow");
        hostPlanes.reset(new HostPlanes((size_t)numCams, (size_t)pl.W * pl.H));
        pl.planes = hostPlanes.get();
    }
    st.events = (int)pl.events.size();
    st.W = pl.W;
    st.H = pl.H;
    for (const SurveyModel &m : pl.models)
        st.modelCams += m.trained;
    // (the products' kernels take sides of up to 65535: a larger run with one of them is the host route's whole)
    if (device >= 0 && pl.W > 0 && decodersTakeWidth(pl.W) && ((!want[SurveyShiftProduct] && !wantCells && !want[SurveyLinesProduct]) || (pl.W <= 65535 && pl.H <= 65535))) {
        st.device = device;
        deviceFrames(parser, pl, nthreads, device, st, devPlanes);
    } else
        hostFrames(parser, pl, nthreads);
    // (the noise's baseline is the run's own: per camera, once every row is there, from its rows at stack position 1)
    if (want[SurveyNoiseProduct])
        for (size_t c = 0; c < pl.models.size(); ++c) {
            SurveyModel &m = pl.models[c];
            if (!m.trained)
                continue;
            const CellGrid &g = pl.grid;
            std::vector<const int32_t *> base;
            for (const SurveyRow &r : pl.rows)
                if ((size_t)r.cam == c && r.frame == 1 && r.state == SurveyRow::Ok && r.has(SurveyNoiseProduct) &&
                    r.noise.size() == g.cells() * NoiseRecordWords)
                    base.push_back(r.noise.data());
            m.noise.resize(g.cells() * NoiseModelWords);
            noiseModelHost(pl.sigma6[c].data(), pl.W, pl.H, g.x0, g.y0, g.ncx, g.ncy, base.data(), base.size(), m.noise.data());
        }
    for (const SurveyRow &r : pl.rows) {
        long long *const counter[] = {&st.ok, &st.undecodable, &st.missing, &st.otherSize};
        ++*counter[r.state];
        ++st.frames;
        ++(r.onKernel ? st.framesKernel : st.framesHostRoute);
        for (int p = 0; p < SurveyProducts; ++p)
            if (r.state == SurveyRow::Ok && r.has((SurveyProduct)p))
                ++(r.has((SurveyProduct)p) == SurveyRow::Kernel ? st.product[p].framesKernel : st.product[p].framesHost);
    }
    for (int p = 0; p < SurveyProducts; ++p)
        st.product[p].host_s = (double)hostUs[p] * 1e-6;
    const auto writeText = [](const std::string &path, const std::string &text) {
        if (!writeFile(path, (const unsigned char *)text.data(), text.size()))
            throw std::runtime_error("survey: cannot write " + path);
    };
    if (!rq.reportPath.empty())
        writeText(rq.reportPath, SurveyReport(pl.models, pl.rows));
    if (want[SurveyShiftProduct])
        writeText(rq.shiftPath, ShiftReport(rq.shiftRadius, pl.models, pl.rows));
    if (want[SurveyFieldProduct]) // (no model file)
        writeCells(fieldDir, "field", SurveyFieldProduct, pl, FieldRecordWords, &SurveyRow::field, nullptr, 0, &SurveyModel::light,
                   FieldReport(pl.cellR, pl.W, pl.H, pl.models, pl.rows));
    if (want[SurveyLightProduct])
        writeCells(lightDir, "light", SurveyLightProduct, pl, LightRecordWords, &SurveyRow::light, "<i4", LightModelWords, &SurveyModel::light,
                   LightReport(pl.cellR, pl.W, pl.H, pl.models, pl.rows));
    if (want[SurveyFocusProduct])
        writeCells(focusDir, "focus", SurveyFocusProduct, pl, FocusRecordWords, &SurveyRow::focus, "<i8", FocusModelWords, &SurveyModel::focus,
                   FocusReport(pl.cellR, pl.W, pl.H, pl.models, pl.rows));
    if (want[SurveyNoiseProduct])
        writeCells(noiseDir, "noise", SurveyNoiseProduct, pl, NoiseRecordWords, &SurveyRow::noise, "<i8", NoiseModelWords, &SurveyModel::noise,
                   NoiseReport(pl.cellR, pl.W, pl.H, pl.models, pl.rows));
    if (want[SurveyLinesProduct])
        writeLines(linesDir, pl, LinesReport(pl.W, pl.H, pl.models, pl.rows));
    if (hostPlanes) {
        const double t1 = nowMs();
        st.planeRowsHost = hostPlanes->rows;
        writePlanes(planesDir, pl, *hostPlanes, devPlanes);
        st.planes_write_s = (nowMs() - t1) * 1e-3;
    }
    st.total_s = (nowMs() - t0) * 1e-3;
    const int rc = st.ok == st.frames ? 0 : 1;
    if (stats)
        *stats = st;
    if (models)
        *models = std::move(pl.models);
    if (rows)
        *rows = std::move(pl.rows);
    return rc;
}

} // namespace abub
