// survey.cpp -- a run measured frame by frame ("Surveying a run"): abub3hs --survey.  No analysis.
// frameStatsHost is the definition of the per-frame record, plain byte loops.  SurveyRun is host only: per frame
// cv::imdecode of the frame and of its reference frame, then frameStatsHost.  SurveyRunDevice (--survey-gpu) reads the
// frames of the run's size through the FileBatch protocol into a resident slab and fills the same records with one
// abub_frame_stats_dev launch per batch; what is not in place in the slab gets its row from the host route's per-frame
// function, of which there is one copy.  Both routes fill one row per frame and share everything behind that: the list of
// the rows, the models, the counters, the report's text, the exit status.
// With a planes directory (--survey-planes; DESIGN section 3, "Surveying a run per pixel") the ok rows are also summed per
// pixel and camera: activityAddHost is the definition, a host thread adds its row into the camera's one set of planes with
// relaxed atomic adds, the device route adds the rows in place in the slab with abub_pixel_activity_dev and keeps its planes
// on the device until the end; the result is their sum, and one writer puts the files on disk for both routes.
// With a shift file (--survey-shift; DESIGN section 3, "Surveying a run for movement") the ok rows of a camera with a model
// are also searched for their displacement against mu: frameShiftHost is the definition of the SAD surface, the device route
// gets the surfaces of the rows in place in the slab from abub_frame_shift_dev, shiftBest reads every surface on the host,
// and one writer (ShiftReport) makes the file for both routes.
// With a field directory (--survey-field; DESIGN section 3, "Surveying a run for local movement") the same rows are also
// searched per cell of 128 x 128 pixels: fieldCellsHost is the definition of the cells' surfaces, the device route gets them
// from abub_frame_shift_cells_dev, fieldCell reads every surface on the host into a record of five words, and one writer
// (writeField, with FieldReport for the text) makes the files for both routes.
// With a light directory (--survey-light; DESIGN section 3, "Surveying a run for lighting changes") the same rows also get
// six sums per cell of the field's grid: lightCellsHost is the definition, the device route gets the records from
// abub_frame_light_cells_dev, lightModelHost sums the model once per camera on the host, lightCell and lightFrame say what
// the sums mean, and one writer (writeLight, with LightReport for the text) makes the files for both routes.
// With a focus directory (--survey-focus; DESIGN section 3, "Surveying a run for lost focus") the same rows also get five
// sums of gradient products per cell of the same grid: focusCellsHost is the definition, the device route gets the records
// from abub_frame_focus_cells_dev, focusModelHost sums the model once per camera on the host, focusCell and focusFrame say
// what the sums mean, and one writer (writeFocus, with FocusReport for the text) makes the files for both routes.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
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

std::string LightReport(int radius, int W, int H, const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows)
{
    int ncx = 0, ncy = 0, x0 = 0, y0 = 0;
    if (W > 0 && H > 0)
        abub_frame_cells_grid(W, H, radius, &ncx, &ncy, &x0, &y0);
    const size_t cells = (size_t)ncx * ncy;
    std::string text = "# abub3hs light 1\n";
    char buf[512];
    snprintf(buf, sizeof buf, "radius %d cell %d grid %d %d origin %d %d\n", radius, (int)ABUB_FIELD_CELL, ncx, ncy, x0, y0);
    text += buf;
    text += "event\tcam\tframe\tname\tstate\tindex\trated\tclipped\tchanged\tup\tdown\tlevel_milli\tratio_min\tratio_max\tgain_milli\toffset_milli\tkind\n";
    static const char *const kinds[] = {"blind", "steady", "level", "uneven"};
    struct Cam {
        long long frames = 0, kind[4] = {0, 0, 0, 0};
        const std::string *first = nullptr;
        std::vector<long long> changed; // per cell: the frames in which it was rated and changed
    };
    std::vector<Cam> cams(models.size());
    for (const SurveyRow &r : rows) {
        snprintf(buf, sizeof buf, "%s\t%d\t%d\t%s\t%s", r.event.c_str(), r.cam, r.frame, r.name.c_str(), r.stateName());
        text += buf;
        const std::vector<uint32_t> *model = (size_t)r.cam < models.size() ? &models[(size_t)r.cam].light : nullptr;
        if (r.state != SurveyRow::Ok || !r.hasLight || r.light.size() != cells * LightRecordWords || !model ||
            model->size() != cells * LightModelWords) {
            text += "\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\n";
            continue;
        }
        Cam &c = cams[(size_t)r.cam];
        c.changed.resize(cells, 0);
        const LightFrame f = lightFrame(r.light.data(), model->data(), cells);
        for (size_t k = 0; k < cells; ++k) {
            const LightCell lc = lightCell(r.light.data() + k * LightRecordWords, model->data() + k * LightModelWords);
            c.changed[k] += lc.rated && lc.changed;
        }
        snprintf(buf, sizeof buf, "\t%lld\t%d\t%d\t%d\t%d\t%d", c.frames, f.rated, f.clipped, f.changed, f.up, f.down);
        text += buf;
        if (f.kind == LightFrame::Blind)
            snprintf(buf, sizeof buf, "\t-\t-\t-\t-\t-");
        else if (f.hasGain)
            snprintf(buf, sizeof buf, "\t%lld\t%lld\t%lld\t%lld\t%lld", f.levelMilli, f.ratioMin, f.ratioMax, f.gainMilli, f.offsetMilli);
        else
            snprintf(buf, sizeof buf, "\t%lld\t%lld\t%lld\t-\t-", f.levelMilli, f.ratioMin, f.ratioMax);
        text += buf;
        text += std::string("\t") + kinds[f.kind] + "\n";
        ++c.frames;
        ++c.kind[f.kind];
        if (f.changed && !c.first)
            c.first = &r.event;
    }
    long long frames = 0, kind[4] = {0, 0, 0, 0};
    for (size_t c = 0; c < cams.size(); ++c) {
        if (!models[c].trained) {
            snprintf(buf, sizeof buf, "light cam %zu none\n", c);
            text += buf;
            continue;
        }
        const Cam &k = cams[c];
        snprintf(buf, sizeof buf, "light cam %zu frames %lld blind %lld steady %lld level %lld uneven %lld first_changed_event %s\n", c, k.frames,
                 k.kind[0], k.kind[1], k.kind[2], k.kind[3], k.first ? k.first->c_str() : "-");
        text += buf;
        frames += k.frames;
        for (int q = 0; q < 4; ++q)
            kind[q] += k.kind[q];
    }
    for (size_t c = 0; c < cams.size(); ++c) {
        if (!models[c].trained)
            continue;
        for (int y = 0; y < ncy; ++y) {
            snprintf(buf, sizeof buf, "changed cam %zu y %d", c, y);
            text += buf;
            for (int x = 0; x < ncx; ++x) {
                const size_t k = (size_t)y * ncx + x;
                snprintf(buf, sizeof buf, " %lld", k < cams[c].changed.size() ? cams[c].changed[k] : 0ll);
                text += buf;
            }
            text += "\n";
        }
    }
    snprintf(buf, sizeof buf, "run frames %lld blind %lld steady %lld level %lld uneven %lld\n", frames, kind[0], kind[1], kind[2], kind[3]);
    text += buf;
    return text;
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

std::string FocusReport(int radius, int W, int H, const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows)
{
    int ncx = 0, ncy = 0, x0 = 0, y0 = 0;
    if (W > 0 && H > 0)
        abub_frame_cells_grid(W, H, radius, &ncx, &ncy, &x0, &y0);
    const size_t cells = (size_t)ncx * ncy;
    std::string text = "# abub3hs focus 1\n";
    char buf[512];
    snprintf(buf, sizeof buf, "radius %d cell %d grid %d %d origin %d %d\n", radius, (int)ABUB_FIELD_CELL, ncx, ncy, x0, y0);
    text += buf;
    text += "event\tcam\tframe\tname\tstate\tindex\trated\tclipped\tchanged\tsofter\tharder\tkeep_milli\tkeep_min\tkeep_max\tenergy_milli\tkind\n";
    static const char *const kinds[] = {"blind", "steady", "soft", "uneven"};
    struct Cam {
        long long frames = 0, kind[4] = {0, 0, 0, 0};
        const std::string *first = nullptr;
        std::vector<long long> changed; // per cell: the frames in which it was rated and changed
    };
    std::vector<Cam> cams(models.size());
    for (const SurveyRow &r : rows) {
        snprintf(buf, sizeof buf, "%s\t%d\t%d\t%s\t%s", r.event.c_str(), r.cam, r.frame, r.name.c_str(), r.stateName());
        text += buf;
        const std::vector<int64_t> *model = (size_t)r.cam < models.size() ? &models[(size_t)r.cam].focus : nullptr;
        if (r.state != SurveyRow::Ok || !r.hasFocus || r.focus.size() != cells * FocusRecordWords || !model ||
            model->size() != cells * FocusModelWords) {
            text += "\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\n";
            continue;
        }
        Cam &c = cams[(size_t)r.cam];
        c.changed.resize(cells, 0);
        const FocusFrame f = focusFrame(r.focus.data(), model->data(), cells);
        for (size_t k = 0; k < cells; ++k) {
            const FocusCell fc = focusCell(r.focus.data() + k * FocusRecordWords, model->data() + k * FocusModelWords);
            c.changed[k] += fc.rated && fc.changed;
        }
        snprintf(buf, sizeof buf, "\t%lld\t%d\t%d\t%d\t%d\t%d", c.frames, f.rated, f.clipped, f.changed, f.softer, f.harder);
        text += buf;
        if (f.kind == FocusFrame::Blind)
            snprintf(buf, sizeof buf, "\t-\t-\t-\t-");
        else
            snprintf(buf, sizeof buf, "\t%lld\t%lld\t%lld\t%lld", f.keepMilli, f.keepMin, f.keepMax, f.energyMilli);
        text += buf;
        text += std::string("\t") + kinds[f.kind] + "\n";
        ++c.frames;
        ++c.kind[f.kind];
        if (f.changed && !c.first)
            c.first = &r.event;
    }
    long long frames = 0, kind[4] = {0, 0, 0, 0};
    for (size_t c = 0; c < cams.size(); ++c) {
        if (!models[c].trained) {
            snprintf(buf, sizeof buf, "focus cam %zu none\n", c);
            text += buf;
            continue;
        }
        const Cam &k = cams[c];
        snprintf(buf, sizeof buf, "focus cam %zu frames %lld blind %lld steady %lld soft %lld uneven %lld first_changed_event %s\n", c, k.frames,
                 k.kind[0], k.kind[1], k.kind[2], k.kind[3], k.first ? k.first->c_str() : "-");
        text += buf;
        frames += k.frames;
        for (int q = 0; q < 4; ++q)
            kind[q] += k.kind[q];
    }
    for (size_t c = 0; c < cams.size(); ++c) {
        if (!models[c].trained)
            continue;
        for (int y = 0; y < ncy; ++y) {
            snprintf(buf, sizeof buf, "changed cam %zu y %d", c, y);
            text += buf;
            for (int x = 0; x < ncx; ++x) {
                const size_t k = (size_t)y * ncx + x;
                snprintf(buf, sizeof buf, " %lld", k < cams[c].changed.size() ? cams[c].changed[k] : 0ll);
                text += buf;
            }
            text += "\n";
        }
    }
    snprintf(buf, sizeof buf, "run frames %lld blind %lld steady %lld soft %lld uneven %lld\n", frames, kind[0], kind[1], kind[2], kind[3]);
    text += buf;
    return text;
}

std::string FieldReport(int radius, int W, int H, const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows)
{
    int ncx = 0, ncy = 0, x0 = 0, y0 = 0;
    if (W > 0 && H > 0)
        abub_frame_cells_grid(W, H, radius, &ncx, &ncy, &x0, &y0);
    const size_t cells = (size_t)ncx * ncy;
    std::string text = "# abub3hs field 1\n";
    char buf[512];
    snprintf(buf, sizeof buf, "radius %d cell %d grid %d %d origin %d %d\n", radius, (int)ABUB_FIELD_CELL, ncx, ncy, x0, y0);
    text += buf;
    text += "event\tcam\tframe\tname\tstate\tindex\trated\tmoved\tmodal_dx\tmodal_dy\tmodal_n\tdx_min\tdx_max\tdy_min\tdy_max\tkind\n";
    enum { Blind, Still, Rigid, Warped, Local };
    static const char *const kinds[] = {"blind", "still", "rigid", "warped", "local"};
    struct Cam {
        long long frames = 0, kind[5] = {0, 0, 0, 0, 0};
        const std::string *first = nullptr;
        std::vector<long long> moved; // per cell: the frames in which it was rated and off (0, 0)
    };
    std::vector<Cam> cams(models.size());
    for (const SurveyRow &r : rows) {
        snprintf(buf, sizeof buf, "%s\t%d\t%d\t%s\t%s", r.event.c_str(), r.cam, r.frame, r.name.c_str(), r.stateName());
        text += buf;
        if (r.state != SurveyRow::Ok || !r.hasField || r.field.size() != cells * FieldRecordWords) {
            text += "\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\t-\n";
            continue;
        }
        Cam &c = cams[(size_t)r.cam];
        c.moved.resize(cells, 0);
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
                ++c.moved[k];
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
        snprintf(buf, sizeof buf, "\t%lld\t%d\t%d", c.frames, rated, moved);
        text += buf;
        if (kind == Blind)
            snprintf(buf, sizeof buf, "\t-\t-\t-\t-\t-\t-\t-\t%s\n", kinds[kind]);
        else
            snprintf(buf, sizeof buf, "\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n", mdx, mdy, mn, dxMin, dxMax, dyMin, dyMax, kinds[kind]);
        text += buf;
        ++c.frames;
        ++c.kind[kind];
        if (moved && !c.first)
            c.first = &r.event;
    }
    long long frames = 0, kind[5] = {0, 0, 0, 0, 0};
    for (size_t c = 0; c < cams.size(); ++c) {
        if (!models[c].trained) {
            snprintf(buf, sizeof buf, "field cam %zu none\n", c);
            text += buf;
            continue;
        }
        const Cam &k = cams[c];
        snprintf(buf, sizeof buf, "field cam %zu frames %lld blind %lld still %lld rigid %lld warped %lld local %lld first_moved_event %s\n", c,
                 k.frames, k.kind[Blind], k.kind[Still], k.kind[Rigid], k.kind[Warped], k.kind[Local], k.first ? k.first->c_str() : "-");
        text += buf;
        frames += k.frames;
        for (int q = 0; q < 5; ++q)
            kind[q] += k.kind[q];
    }
    for (size_t c = 0; c < cams.size(); ++c) {
        if (!models[c].trained)
            continue;
        for (int y = 0; y < ncy; ++y) {
            snprintf(buf, sizeof buf, "moved cam %zu y %d", c, y);
            text += buf;
            for (int x = 0; x < ncx; ++x) {
                const size_t k = (size_t)y * ncx + x;
                snprintf(buf, sizeof buf, " %lld", k < cams[c].moved.size() ? cams[c].moved[k] : 0ll);
                text += buf;
            }
            text += "\n";
        }
    }
    snprintf(buf, sizeof buf, "run frames %lld blind %lld still %lld rigid %lld warped %lld local %lld\n", frames, kind[Blind], kind[Still],
             kind[Rigid], kind[Warped], kind[Local]);
    text += buf;
    return text;
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
        snprintf(buf, sizeof buf, "%s\t%d\t%d\t%s\t%s", r.event.c_str(), r.cam, r.frame, r.name.c_str(), r.stateName());
        text += buf;
        if (r.state != SurveyRow::Ok || !r.hasShift) {
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
        snprintf(buf, sizeof buf, "%s\t%d\t%d\t%s\t%s", r.event.c_str(), r.cam, r.frame, r.name.c_str(), r.stateName());
        text += buf;
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
struct Plan {
    HostPlanes *planes = nullptr;   // with a planes directory: where surveyFrame adds its ok rows
    int shiftR = 0;                 // with a shift file: the radius surveyFrame searches its ok rows with a model in (0: none)
    std::atomic<long long> *shiftHostUs = nullptr; // ... and where it adds the microseconds it spent in frameShiftHost
    int fieldR = 0;                 // with a field directory: the radius of the per-cell search (0: none) ...
    size_t fieldCells = 0;          // ... the run's cells (abub_frame_cells_grid) ...
    std::atomic<long long> *fieldHostUs = nullptr; // ... and where surveyFrame adds the microseconds it spent in fieldCellsHost
    bool light = false;             // with a light directory: surveyFrame gives its ok rows with a model their light records ...
    int lightNcx = 0, lightNcy = 0, lightX0 = 0, lightY0 = 0; // ... on this grid (abub_frame_cells_grid at the field's radius) ...
    std::atomic<long long> *lightHostUs = nullptr; // ... and adds the microseconds it spent in lightCellsHost here
    bool focus = false;             // with a focus directory: surveyFrame gives its ok rows with a model their focus records ...
    int focusNcx = 0, focusNcy = 0, focusX0 = 0, focusY0 = 0; // ... on this grid (the same rule) ...
    std::atomic<long long> *focusHostUs = nullptr; // ... and adds the microseconds it spent in focusCellsHost here
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

// The shift search of an ok row of a camera with a model on this thread: the definition, then the one tie rule
void shiftRowHost(const Plan &pl, const uint8_t *cur, const uint8_t *mu, SurveyRow &row)
{
    const double t0 = nowMs();
    const size_t D = 2 * (size_t)pl.shiftR + 1;
    std::vector<uint64_t> sad(D * D);
    frameShiftHost(cur, mu, pl.W, pl.H, pl.shiftR, sad.data());
    row.shift = shiftBest(sad.data(), pl.shiftR);
    row.hasShift = true;
    row.shiftOnKernel = false;
    if (pl.shiftHostUs)
        *pl.shiftHostUs += (long long)((nowMs() - t0) * 1e3);
}

// a row's records from its cells' surfaces ([cells][(2 R + 1)^2]), whichever route made them
void fieldRecords(const Plan &pl, const uint32_t *sad, SurveyRow &row, bool onKernel)
{
    const size_t N = (2 * (size_t)pl.fieldR + 1) * (2 * (size_t)pl.fieldR + 1);
    row.field.resize(pl.fieldCells * FieldRecordWords);
    for (size_t k = 0; k < pl.fieldCells; ++k)
        fieldCell(sad + k * N, pl.fieldR, row.field.data() + k * FieldRecordWords);
    row.hasField = true;
    row.fieldOnKernel = onKernel;
}

// The per-cell search of an ok row of a camera with a model on this thread: the definition, then the records
void fieldRowHost(const Plan &pl, const uint8_t *cur, const uint8_t *mu, SurveyRow &row)
{
    const double t0 = nowMs();
    const size_t N = (2 * (size_t)pl.fieldR + 1) * (2 * (size_t)pl.fieldR + 1);
    std::vector<uint32_t> sad(pl.fieldCells * N);
    fieldCellsHost(cur, mu, pl.W, pl.H, pl.fieldR, sad.data());
    fieldRecords(pl, sad.data(), row, false);
    if (pl.fieldHostUs)
        *pl.fieldHostUs += (long long)((nowMs() - t0) * 1e3);
}

// The light records of an ok row of a camera with a model on this thread: the definition
void lightRowHost(const Plan &pl, const uint8_t *cur, const uint8_t *mu, SurveyRow &row)
{
    const double t0 = nowMs();
    row.light.resize((size_t)pl.lightNcx * pl.lightNcy * LightRecordWords);
    lightCellsHost(cur, mu, pl.W, pl.H, pl.lightX0, pl.lightY0, pl.lightNcx, pl.lightNcy, row.light.data());
    row.hasLight = true;
    row.lightOnKernel = false;
    if (pl.lightHostUs)
        *pl.lightHostUs += (long long)((nowMs() - t0) * 1e3);
}

// The focus records of an ok row of a camera with a model on this thread: the definition
void focusRowHost(const Plan &pl, const uint8_t *cur, const uint8_t *mu, SurveyRow &row)
{
    const double t0 = nowMs();
    row.focus.resize((size_t)pl.focusNcx * pl.focusNcy * FocusRecordWords);
    focusCellsHost(cur, mu, pl.W, pl.H, pl.focusX0, pl.focusY0, pl.focusNcx, pl.focusNcy, row.focus.data());
    row.hasFocus = true;
    row.focusOnKernel = false;
    if (pl.focusHostUs)
        *pl.focusHostUs += (long long)((nowMs() - t0) * 1e3);
}

// The host route's per-frame function: row i on this thread, its state and its record.  It asks nothing of the other rows:
// the reference frame is decoded here as well, and is there iff its own row is ok
void surveyFrame(Parser &p, const Plan &pl, size_t i, SurveyRow &row)
{
    row.onKernel = false;
    row.hasShift = row.shiftOnKernel = false;
    row.hasField = row.fieldOnKernel = false;
    row.hasLight = row.lightOnKernel = false;
    row.hasFocus = row.focusOnKernel = false;
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
    if (pl.shiftR && mu)
        shiftRowHost(pl, cur.data, mu, row);
    if (pl.fieldR && mu)
        fieldRowHost(pl, cur.data, mu, row);
    if (pl.light && mu)
        lightRowHost(pl, cur.data, mu, row);
    if (pl.focus && mu)
        focusRowHost(pl, cur.data, mu, row);
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

// The device route: the rows in batches.  Per batch: the reference frames of its first rows that lie in front of it take
// the first slots (they are read again), then the rows; the pool reads the files into a pinned buffer; upload; the decoders
// into the slab, slot s at s * align16(W * H); one abub_frame_stats_dev launch over the rows that are in place, and the
// records back in one copy.  A row that is not in place goes to surveyFrame.  With pl.planes the rows in place are also
// added to the per-pixel planes on the device, [camera][6][stride] u32 cleared once: behind the batch's statistics launch one
// abub_pixel_activity_dev call per camera that has rows in place, its jobs behind the records in the same meta buffer; they
// come back in one copy at the end, into devPlanes.  A row in place whose file no GPU decoder reads was decoded by a reading
// thread; its pixels are on the host, and it is added to the host planes there, not by the kernel.
// With pl.shiftR the rows in place that have a model are also searched for their displacement, behind the statistics launch
// and on the same stream: one abub_frame_shift_dev call per batch over [jobs][status words][surfaces] in a buffer of its own
// (mu is resident already), the surfaces back in one copy; shiftBest on the host says what each means.  Every row in place
// is in the slab, whichever decoder or thread put it there, so all of them are the kernel's.
// With pl.fieldR the same rows are then searched per cell, behind the shift launch on the same stream, over
// [jobs][status words][surfaces] in a buffer of its own: abub_frame_shift_cells_dev in calls of as many jobs as keep the
// surfaces below 64 MiB (ABUB_FIELD_CHUNK=n, a test knob: of n jobs), each call's status words and surfaces back in one copy.
// A job's surface depends on nothing but the job, so the split cannot show in the result.
// With pl.light the same rows then get their light records, behind the launches above on the same stream: one
// abub_frame_light_cells_dev call per batch over [jobs][status words][records] in a buffer of its own, the status words and
// the records (24 bytes per cell) back in one copy.
// With pl.focus the same rows then get their focus records in the same way, behind the light's launch on the same stream: one
// abub_frame_focus_cells_dev call per batch over [jobs][status words][records] in a buffer of its own, the status words and
// the records (20 bytes per cell) back in one copy.
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
    PinnedBuffer h_meta, h_shift, h_field, h_light, h_focus;
    DeviceBuffer d_meta, d_shift, d_field, d_light, d_focus, d_model; // d_model: [mu of every camera][sigma6 of every camera], camera c at c * stride
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
            if (pl.shiftR) {
                st.stats_s += (nowMs() - t0) * 1e-3;
                t0 = nowMs();
                std::vector<size_t> with; // the jobs that have a model
                for (size_t g = 0; g < nj; ++g)
                    if (jobs[g].model != UINT64_MAX)
                        with.push_back(g);
                const size_t ns = with.size(), N = (2 * (size_t)pl.shiftR + 1) * (2 * (size_t)pl.shiftR + 1);
                if (ns) {
                    const size_t jobBytes = ns * sizeof(abub_shift_job), statusBytes = (ns * sizeof(uint32_t) + 7) & ~(size_t)7;
                    const size_t bytes = jobBytes + statusBytes + ns * N * sizeof(uint64_t);
                    h_shift.grow(bytes);
                    d_shift.grow(bytes);
                    abub_shift_job *sj = (abub_shift_job *)h_shift.get();
                    for (size_t q = 0; q < ns; ++q)
                        sj[q] = abub_shift_job{jobs[with[q]].cur, jobs[with[q]].model};
                    HIPOK(hipMemcpyAsync(d_shift.get(), h_shift.get(), jobBytes, hipMemcpyHostToDevice, cs));
                    check(abub_frame_shift_dev(B.slab.get(), slots * stride, d_model.get(), C * stride, (const abub_shift_job *)d_shift.get(),
                                               (int)ns, W, H, pl.shiftR, (uint32_t *)(d_shift.get() + jobBytes),
                                               (uint64_t *)(d_shift.get() + jobBytes + statusBytes), cs),
                          "abub_frame_shift_dev");
                    HIPOK(hipMemcpyAsync(h_shift.get() + jobBytes, d_shift.get() + jobBytes, bytes - jobBytes, hipMemcpyDeviceToHost, cs));
                    HIPOK(hipStreamSynchronize(cs));
                    const uint32_t *status = (const uint32_t *)(h_shift.get() + jobBytes);
                    const uint64_t *sad = (const uint64_t *)(h_shift.get() + jobBytes + statusBytes);
                    for (size_t q = 0; q < ns; ++q) {
                        if (status[q] != 0)
                            throw std::runtime_error("survey: abub_frame_shift_dev refused a frame of its own slab");
                        SurveyRow &row = pl.rows[rowOf(slot[with[q]])];
                        row.shift = shiftBest(sad + q * N, pl.shiftR);
                        row.hasShift = row.shiftOnKernel = true;
                    }
                    ++st.shiftLaunches;
                }
                st.shift_s += (nowMs() - t0) * 1e-3;
                t0 = nowMs();
            }
            if (pl.fieldR) {
                st.stats_s += (nowMs() - t0) * 1e-3;
                t0 = nowMs();
                std::vector<size_t> with; // the jobs that have a model
                for (size_t g = 0; g < nj; ++g)
                    if (jobs[g].model != UINT64_MAX)
                        with.push_back(g);
                const size_t N = (2 * (size_t)pl.fieldR + 1) * (2 * (size_t)pl.fieldR + 1), words = pl.fieldCells * N;
                size_t chunk = std::max<size_t>(1, ((size_t)64 << 20) / (words * sizeof(uint32_t)));
                if (const char *e = getenv("ABUB_FIELD_CHUNK"))
                    if (atoi(e) > 0)
                        chunk = (size_t)atoi(e);
                for (size_t q0 = 0; q0 < with.size(); q0 += chunk) {
                    const size_t ns = std::min(chunk, with.size() - q0);
                    const size_t jobBytes = ns * sizeof(abub_shift_job), bytes = jobBytes + ns * (1 + words) * sizeof(uint32_t);
                    h_field.grow(bytes);
                    d_field.grow(bytes);
                    abub_shift_job *fj = (abub_shift_job *)h_field.get();
                    for (size_t q = 0; q < ns; ++q)
                        fj[q] = abub_shift_job{jobs[with[q0 + q]].cur, jobs[with[q0 + q]].model};
                    HIPOK(hipMemcpyAsync(d_field.get(), h_field.get(), jobBytes, hipMemcpyHostToDevice, cs));
                    uint32_t *d_status = (uint32_t *)(d_field.get() + jobBytes);
                    check(abub_frame_shift_cells_dev(B.slab.get(), slots * stride, d_model.get(), C * stride,
                                                     (const abub_shift_job *)d_field.get(), (int)ns, W, H, pl.fieldR, d_status, d_status + ns, cs),
                          "abub_frame_shift_cells_dev");
                    HIPOK(hipMemcpyAsync(h_field.get() + jobBytes, d_field.get() + jobBytes, bytes - jobBytes, hipMemcpyDeviceToHost, cs));
                    HIPOK(hipStreamSynchronize(cs));
                    const uint32_t *status = (const uint32_t *)(h_field.get() + jobBytes), *sad = status + ns;
                    for (size_t q = 0; q < ns; ++q) {
                        if (status[q] != 0)
                            throw std::runtime_error("survey: abub_frame_shift_cells_dev refused a frame of its own slab");
                        fieldRecords(pl, sad + q * words, pl.rows[rowOf(slot[with[q0 + q]])], true);
                    }
                    ++st.fieldLaunches;
                }
                st.field_s += (nowMs() - t0) * 1e-3;
                t0 = nowMs();
            }
            if (pl.light) {
                st.stats_s += (nowMs() - t0) * 1e-3;
                t0 = nowMs();
                std::vector<size_t> with; // the jobs that have a model
                for (size_t g = 0; g < nj; ++g)
                    if (jobs[g].model != UINT64_MAX)
                        with.push_back(g);
                const size_t ns = with.size(), words = (size_t)pl.lightNcx * pl.lightNcy * LightRecordWords;
                if (ns) {
                    const size_t jobBytes = ns * sizeof(abub_shift_job), bytes = jobBytes + ns * (1 + words) * sizeof(uint32_t);
                    h_light.grow(bytes);
                    d_light.grow(bytes);
                    abub_shift_job *lj = (abub_shift_job *)h_light.get();
                    for (size_t q = 0; q < ns; ++q)
                        lj[q] = abub_shift_job{jobs[with[q]].cur, jobs[with[q]].model};
                    HIPOK(hipMemcpyAsync(d_light.get(), h_light.get(), jobBytes, hipMemcpyHostToDevice, cs));
                    uint32_t *d_status = (uint32_t *)(d_light.get() + jobBytes);
                    check(abub_frame_light_cells_dev(B.slab.get(), slots * stride, d_model.get(), C * stride,
                                                     (const abub_shift_job *)d_light.get(), (int)ns, W, H, pl.lightX0, pl.lightY0, pl.lightNcx,
                                                     pl.lightNcy, d_status, d_status + ns, cs),
                          "abub_frame_light_cells_dev");
                    HIPOK(hipMemcpyAsync(h_light.get() + jobBytes, d_light.get() + jobBytes, bytes - jobBytes, hipMemcpyDeviceToHost, cs));
                    HIPOK(hipStreamSynchronize(cs));
                    const uint32_t *status = (const uint32_t *)(h_light.get() + jobBytes), *rec = status + ns;
                    for (size_t q = 0; q < ns; ++q) {
                        if (status[q] != 0)
                            throw std::runtime_error("survey: abub_frame_light_cells_dev refused a frame of its own slab");
                        SurveyRow &row = pl.rows[rowOf(slot[with[q]])];
                        row.light.assign(rec + q * words, rec + (q + 1) * words);
                        row.hasLight = row.lightOnKernel = true;
                    }
                    ++st.lightLaunches;
                }
                st.light_s += (nowMs() - t0) * 1e-3;
                t0 = nowMs();
            }
            if (pl.focus) {
                st.stats_s += (nowMs() - t0) * 1e-3;
                t0 = nowMs();
                std::vector<size_t> with; // the jobs that have a model
                for (size_t g = 0; g < nj; ++g)
                    if (jobs[g].model != UINT64_MAX)
                        with.push_back(g);
                const size_t ns = with.size(), words = (size_t)pl.focusNcx * pl.focusNcy * FocusRecordWords;
                if (ns) {
                    const size_t jobBytes = ns * sizeof(abub_shift_job), bytes = jobBytes + ns * (1 + words) * sizeof(uint32_t);
                    h_focus.grow(bytes);
                    d_focus.grow(bytes);
                    abub_shift_job *fj = (abub_shift_job *)h_focus.get();
                    for (size_t q = 0; q < ns; ++q)
                        fj[q] = abub_shift_job{jobs[with[q]].cur, jobs[with[q]].model};
                    HIPOK(hipMemcpyAsync(d_focus.get(), h_focus.get(), jobBytes, hipMemcpyHostToDevice, cs));
                    uint32_t *d_status = (uint32_t *)(d_focus.get() + jobBytes);
                    check(abub_frame_focus_cells_dev(B.slab.get(), slots * stride, d_model.get(), C * stride,
                                                     (const abub_shift_job *)d_focus.get(), (int)ns, W, H, pl.focusX0, pl.focusY0, pl.focusNcx,
                                                     pl.focusNcy, d_status, (int32_t *)(d_status + ns), cs),
                          "abub_frame_focus_cells_dev");
                    HIPOK(hipMemcpyAsync(h_focus.get() + jobBytes, d_focus.get() + jobBytes, bytes - jobBytes, hipMemcpyDeviceToHost, cs));
                    HIPOK(hipStreamSynchronize(cs));
                    const uint32_t *status = (const uint32_t *)(h_focus.get() + jobBytes);
                    const int32_t *rec = (const int32_t *)(status + ns);
                    for (size_t q = 0; q < ns; ++q) {
                        if (status[q] != 0)
                            throw std::runtime_error("survey: abub_frame_focus_cells_dev refused a frame of its own slab");
                        SurveyRow &row = pl.rows[rowOf(slot[with[q]])];
                        row.focus.assign(rec + q * words, rec + (q + 1) * words);
                        row.hasFocus = row.focusOnKernel = true;
                    }
                    ++st.focusLaunches;
                }
                st.focus_s += (nowMs() - t0) * 1e-3;
                t0 = nowMs();
            }
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

// The files of the per-cell shift field, one writer for both routes ("Surveying a run for local
// movement"): per camera with a model cam<c>_field.npy, the records of its rows that have a surface in survey order (the
// `index` column of field.txt), and field.txt
void writeField(const std::string &dir, int radius, const Plan &pl)
{
    std::string failed;
    if (!makeDirs(dir, &failed))
        throw std::runtime_error("survey: cannot make the directory " + failed);
    int ncx = 0, ncy = 0, x0 = 0, y0 = 0;
    if (pl.W > 0)
        abub_frame_cells_grid(pl.W, pl.H, radius, &ncx, &ncy, &x0, &y0);
    for (size_t c = 0; c < pl.models.size(); ++c) {
        if (!pl.models[c].trained)
            continue;
        std::string data;
        size_t n = 0;
        for (const SurveyRow &r : pl.rows)
            if ((size_t)r.cam == c && r.state == SurveyRow::Ok && r.hasField && r.field.size() == pl.fieldCells * FieldRecordWords) {
                data.append((const char *)r.field.data(), r.field.size() * sizeof(int32_t));
                ++n;
            }
        char shape[96];
        snprintf(shape, sizeof shape, "(%zu, %d, %d, %d)", n, ncy, ncx, (int)FieldRecordWords);
        const std::string file = npyHead("<i4", shape) + data, path = dir + "/cam" + std::to_string(c) + "_field.npy";
        if (!writeFile(path, (const unsigned char *)file.data(), file.size()))
            throw std::runtime_error("survey: cannot write " + path);
    }
    const std::string text = FieldReport(radius, pl.W, pl.H, pl.models, pl.rows);
    if (!writeFile(dir + "/field.txt", (const unsigned char *)text.data(), text.size()))
        throw std::runtime_error("survey: cannot write " + dir + "/field.txt");
}

// The files of the light records, one writer for both routes ("Surveying a run for lighting changes"): per
// camera with a model cam<c>_light.npy, the records of its rows that have one in survey order (the `index` column of
// light.txt), cam<c>_light_model.npy, and light.txt
void writeLight(const std::string &dir, int radius, const Plan &pl)
{
    std::string failed;
    if (!makeDirs(dir, &failed))
        throw std::runtime_error("survey: cannot make the directory " + failed);
    const size_t cells = (size_t)pl.lightNcx * pl.lightNcy;
    for (size_t c = 0; c < pl.models.size(); ++c) {
        if (!pl.models[c].trained)
            continue;
        std::string data;
        size_t n = 0;
        for (const SurveyRow &r : pl.rows)
            if ((size_t)r.cam == c && r.state == SurveyRow::Ok && r.hasLight && r.light.size() == cells * LightRecordWords) {
                data.append((const char *)r.light.data(), r.light.size() * sizeof(uint32_t));
                ++n;
            }
        char shape[96];
        snprintf(shape, sizeof shape, "(%zu, %d, %d, %d)", n, pl.lightNcy, pl.lightNcx, (int)LightRecordWords);
        const std::string stem = dir + "/cam" + std::to_string(c);
        std::string file = npyHead("<i4", shape) + data;
        if (!writeFile(stem + "_light.npy", (const unsigned char *)file.data(), file.size()))
            throw std::runtime_error("survey: cannot write " + stem + "_light.npy");
        snprintf(shape, sizeof shape, "(%d, %d, %d)", pl.lightNcy, pl.lightNcx, (int)LightModelWords);
        const std::vector<uint32_t> &m = pl.models[c].light;
        file = npyHead("<i4", shape) + std::string((const char *)m.data(), m.size() * sizeof(uint32_t));
        if (!writeFile(stem + "_light_model.npy", (const unsigned char *)file.data(), file.size()))
            throw std::runtime_error("survey: cannot write " + stem + "_light_model.npy");
    }
    const std::string text = LightReport(radius, pl.W, pl.H, pl.models, pl.rows);
    if (!writeFile(dir + "/light.txt", (const unsigned char *)text.data(), text.size()))
        throw std::runtime_error("survey: cannot write " + dir + "/light.txt");
}

// The files of the focus records, one writer for both routes ("Surveying a run for lost focus"): per
// camera with a model cam<c>_focus.npy, the records of its rows that have one in survey order (the `index` column of
// focus.txt), cam<c>_focus_model.npy, and focus.txt
void writeFocus(const std::string &dir, int radius, const Plan &pl)
{
    std::string failed;
    if (!makeDirs(dir, &failed))
        throw std::runtime_error("survey: cannot make the directory " + failed);
    const size_t cells = (size_t)pl.focusNcx * pl.focusNcy;
    for (size_t c = 0; c < pl.models.size(); ++c) {
        if (!pl.models[c].trained)
            continue;
        std::string data;
        size_t n = 0;
        for (const SurveyRow &r : pl.rows)
            if ((size_t)r.cam == c && r.state == SurveyRow::Ok && r.hasFocus && r.focus.size() == cells * FocusRecordWords) {
                data.append((const char *)r.focus.data(), r.focus.size() * sizeof(int32_t));
                ++n;
            }
        char shape[96];
        snprintf(shape, sizeof shape, "(%zu, %d, %d, %d)", n, pl.focusNcy, pl.focusNcx, (int)FocusRecordWords);
        const std::string stem = dir + "/cam" + std::to_string(c);
        std::string file = npyHead("<i4", shape) + data;
        if (!writeFile(stem + "_focus.npy", (const unsigned char *)file.data(), file.size()))
            throw std::runtime_error("survey: cannot write " + stem + "_focus.npy");
        snprintf(shape, sizeof shape, "(%d, %d, %d)", pl.focusNcy, pl.focusNcx, (int)FocusModelWords);
        const std::vector<int64_t> &m = pl.models[c].focus;
        file = npyHead("<i8", shape) + std::string((const char *)m.data(), m.size() * sizeof(int64_t));
        if (!writeFile(stem + "_focus_model.npy", (const unsigned char *)file.data(), file.size()))
            throw std::runtime_error("survey: cannot write " + stem + "_focus_model.npy");
    }
    const std::string text = FocusReport(radius, pl.W, pl.H, pl.models, pl.rows);
    if (!writeFile(dir + "/focus.txt", (const unsigned char *)text.data(), text.size()))
        throw std::runtime_error("survey: cannot write " + dir + "/focus.txt");
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

int surveyRun(Parser *parser, const std::vector<Trainer *> &trainers, int numCams, const std::string &format,
              const std::string &reportPath, int nthreads, int device, SurveyStats *stats, std::vector<SurveyRow> *rows,
              std::vector<SurveyModel> *models, const SurveyPlanes &planes, const SurveyShift &shift, const SurveyField &field,
              const SurveyLight &light, const SurveyFocus &focus)
{
    const double t0 = nowMs();
    SurveyStats st;
    if (device >= 0) // (before anything else)
        requireDevice(device, "survey", "; without --survey-gpu the run is surveyed on the host");
    const std::string planesDir = trimSlashes(planes.dir);
    // (the planes' files have names of their own, but a run directory is not the place for what was derived from it)
    if (!planesDir.empty() && sameDirectory(trimSlashes(planes.srcRunDir), planesDir))
        throw std::runtime_error("survey: " + planesDir + " is the run that is being read");
    const std::string fieldDir = trimSlashes(field.dir);
    if (!fieldDir.empty() && sameDirectory(trimSlashes(field.srcRunDir), fieldDir))
        throw std::runtime_error("survey: " + fieldDir + " is the run that is being read");
    const std::string lightDir = trimSlashes(light.dir);
    if (!lightDir.empty() && sameDirectory(trimSlashes(light.srcRunDir), lightDir))
        throw std::runtime_error("survey: " + lightDir + " is the run that is being read");
    const std::string focusDir = trimSlashes(focus.dir);
    if (!focusDir.empty() && sameDirectory(trimSlashes(focus.srcRunDir), focusDir))
        throw std::runtime_error("survey: " + focusDir + " is the run that is being read");
    if ((!fieldDir.empty() || !lightDir.empty() || !focusDir.empty()) && (field.radius < 1 || field.radius > 8))
        throw std::runtime_error("survey: the field radius must be in [1, 8], not " + std::to_string(field.radius));
    if (!shift.path.empty() && (shift.radius < 1 || shift.radius > 8))
        throw std::runtime_error("survey: the shift radius must be in [1, 8], not " + std::to_string(shift.radius));
    Plan pl = planRun(parser, trainers, numCams, format);
    std::atomic<long long> shiftHostUs{0};
    if (!shift.path.empty()) {
        const int need = 2 * shift.radius + 1;
        if (pl.W > 0 && (pl.W < need || pl.H < need))
            throw std::runtime_error("survey: a shift search at radius " + std::to_string(shift.radius) + " needs frames of at least " +
                                     std::to_string(need) + "x" + std::to_string(need) + ", the run's are " + std::to_string(pl.W) + "x" +
                                     std::to_string(pl.H));
        pl.shiftR = shift.radius;
        pl.shiftHostUs = &shiftHostUs;
    }
    std::atomic<long long> fieldHostUs{0};
    if (!fieldDir.empty()) {
        const int need = ABUB_FIELD_CELL + 2 * field.radius;
        int ncx = 0, ncy = 0, x0 = 0, y0 = 0;
        if (pl.W > 0) {
            abub_frame_cells_grid(pl.W, pl.H, field.radius, &ncx, &ncy, &x0, &y0);
            if (ncx == 0 || ncy == 0)
                throw std::runtime_error("survey: a shift field at radius " + std::to_string(field.radius) + " needs frames of at least " +
                                         std::to_string(need) + "x" + std::to_string(need) + ", the run's are " + std::to_string(pl.W) + "x" +
                                         std::to_string(pl.H));
        }
        pl.fieldR = field.radius;
        pl.fieldCells = (size_t)ncx * ncy;
        pl.fieldHostUs = &fieldHostUs;
    }
    std::atomic<long long> lightHostUs{0};
    if (!lightDir.empty()) {
        if (pl.W > 0) {
            abub_frame_cells_grid(pl.W, pl.H, field.radius, &pl.lightNcx, &pl.lightNcy, &pl.lightX0, &pl.lightY0);
            if (pl.lightNcx == 0 || pl.lightNcy == 0) {
                const int need = ABUB_FIELD_CELL + 2 * field.radius;
                throw std::runtime_error("survey: the light records at radius " + std::to_string(field.radius) + " need frames of at least " +
                                         std::to_string(need) + "x" + std::to_string(need) + ", the run's are " + std::to_string(pl.W) + "x" +
                                         std::to_string(pl.H));
            }
        }
        pl.light = true;
        pl.lightHostUs = &lightHostUs;
        for (size_t c = 0; c < pl.models.size(); ++c) // (the model's sums depend on the camera alone: once, here, for both routes)
            if (pl.models[c].trained) {
                pl.models[c].light.resize((size_t)pl.lightNcx * pl.lightNcy * LightModelWords);
                lightModelHost(pl.mu[c], pl.sigma6[c].data(), pl.W, pl.H, pl.lightX0, pl.lightY0, pl.lightNcx, pl.lightNcy,
                               pl.models[c].light.data());
            }
    }
    std::atomic<long long> focusHostUs{0};
    if (!focusDir.empty()) {
        if (pl.W > 0) {
            abub_frame_cells_grid(pl.W, pl.H, field.radius, &pl.focusNcx, &pl.focusNcy, &pl.focusX0, &pl.focusY0);
            if (pl.focusNcx == 0 || pl.focusNcy == 0) {
                const int need = ABUB_FIELD_CELL + 2 * field.radius;
                throw std::runtime_error("survey: the focus records at radius " + std::to_string(field.radius) + " need frames of at least " +
                                         std::to_string(need) + "x" + std::to_string(need) + ", the run's are " + std::to_string(pl.W) + "x" +
                                         std::to_string(pl.H));
            }
        }
        pl.focus = true;
        pl.focusHostUs = &focusHostUs;
        for (size_t c = 0; c < pl.models.size(); ++c) // (the model's sums depend on the camera alone: once, here, for both routes)
            if (pl.models[c].trained) {
                pl.models[c].focus.resize((size_t)pl.focusNcx * pl.focusNcy * FocusModelWords);
                focusModelHost(pl.mu[c], pl.sigma6[c].data(), pl.W, pl.H, pl.focusX0, pl.focusY0, pl.focusNcx, pl.focusNcy,
                               pl.models[c].focus.data());
            }
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
    // (abub_frame_shift_dev, abub_frame_shift_cells_dev, abub_frame_light_cells_dev and abub_frame_focus_cells_dev take sides
    // of up to 65535: a larger run with a shift file, a field, light or focus records is the host route's whole)
    if (device >= 0 && pl.W > 0 && decodersTakeWidth(pl.W) &&
        ((!pl.shiftR && !pl.fieldR && !pl.light && !pl.focus) || (pl.W <= 65535 && pl.H <= 65535))) {
        st.device = device;
        deviceFrames(parser, pl, nthreads, device, st, devPlanes);
    } else
        hostFrames(parser, pl, nthreads);
    for (const SurveyRow &r : pl.rows) {
        long long *const counter[] = {&st.ok, &st.undecodable, &st.missing, &st.otherSize};
        ++*counter[r.state];
        ++st.frames;
        ++(r.onKernel ? st.framesKernel : st.framesHostRoute);
        if (r.state == SurveyRow::Ok && r.hasShift)
            ++(r.shiftOnKernel ? st.shiftFramesKernel : st.shiftFramesHost);
        if (r.state == SurveyRow::Ok && r.hasField)
            ++(r.fieldOnKernel ? st.fieldFramesKernel : st.fieldFramesHost);
        if (r.state == SurveyRow::Ok && r.hasLight)
            ++(r.lightOnKernel ? st.lightFramesKernel : st.lightFramesHost);
        if (r.state == SurveyRow::Ok && r.hasFocus)
            ++(r.focusOnKernel ? st.focusFramesKernel : st.focusFramesHost);
    }
    st.shiftHost_s = (double)shiftHostUs * 1e-6;
    st.fieldHost_s = (double)fieldHostUs * 1e-6;
    st.lightHost_s = (double)lightHostUs * 1e-6;
    st.focusHost_s = (double)focusHostUs * 1e-6;
    if (!reportPath.empty()) {
        const std::string text = SurveyReport(pl.models, pl.rows);
        if (!writeFile(reportPath, (const unsigned char *)text.data(), text.size()))
            throw std::runtime_error("survey: cannot write " + reportPath);
    }
    if (!shift.path.empty()) {
        const std::string text = ShiftReport(shift.radius, pl.models, pl.rows);
        if (!writeFile(shift.path, (const unsigned char *)text.data(), text.size()))
            throw std::runtime_error("survey: cannot write " + shift.path);
    }
    if (!fieldDir.empty())
        writeField(fieldDir, field.radius, pl);
    if (!lightDir.empty())
        writeLight(lightDir, field.radius, pl);
    if (!focusDir.empty())
        writeFocus(focusDir, field.radius, pl);
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

} // namespace

int SurveyRun(Parser *parser, const std::vector<Trainer *> &trainers, int numCams, const std::string &imageFormat,
              const std::string &reportPath, int nthreads, SurveyStats *stats, std::vector<SurveyRow> *rows,
              std::vector<SurveyModel> *models, const SurveyPlanes &planes, const SurveyShift &shift, const SurveyField &field,
              const SurveyLight &light, const SurveyFocus &focus)
{
    return surveyRun(parser, trainers, numCams, imageFormat, reportPath, nthreads, -1, stats, rows, models, planes, shift, field, light,
                     focus);
}

int SurveyRunDevice(Parser *parser, const std::vector<Trainer *> &trainers, int numCams, const std::string &imageFormat,
                    const std::string &reportPath, int nthreads, int device, SurveyStats *stats, std::vector<SurveyRow> *rows,
                    std::vector<SurveyModel> *models, const SurveyPlanes &planes, const SurveyShift &shift, const SurveyField &field,
                    const SurveyLight &light, const SurveyFocus &focus)
{
    if (device < 0)
        throw std::runtime_error("survey: no such HIP device: " + std::to_string(device));
    return surveyRun(parser, trainers, numCams, imageFormat, reportPath, nthreads, device, stats, rows, models, planes, shift, field,
                     light, focus);
}

} // namespace abub
