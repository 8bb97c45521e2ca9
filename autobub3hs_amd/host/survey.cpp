// survey.cpp -- a run measured frame by frame ("Surveying a run"): abub3hs --survey.  No analysis.
// frameStatsHost is the definition of the per-frame record, plain byte loops.  SurveyRun is host only: per frame
// cv::imdecode of the frame and of its reference frame, then frameStatsHost.  SurveyRunDevice (--survey-gpu) reads the
// frames of the run's size through the FileBatch protocol into a resident slab and fills the same records with one
// abub_frame_stats_dev launch per batch; what is not in place in the slab gets its row from the host route's per-frame
// function, of which there is one copy.  Both routes fill one row per frame and share everything behind that: the list of
// the rows, the models, the counters, the report's text, the exit status.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>

#include "AlgorithmTraining/Trainer.hpp"
#include "driver.hpp"
#include "framefiles.hpp"
#include "runbatch.hpp"
#include "runframes.hpp"

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

// The part of a survey that is not its frames' pixels
struct Plan {
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

// The host route's per-frame function: row i on this thread, its state and its record.  It asks nothing of the other rows:
// the reference frame is decoded here as well, and is there iff its own row is ok
void surveyFrame(Parser &p, const Plan &pl, size_t i, SurveyRow &row)
{
    row.onKernel = false;
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
// records back in one copy.  A row that is not in place goes to surveyFrame.
void deviceFrames(Parser *parser, Plan &pl, int nthreads, int device, SurveyStats &st)
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
    PinnedBuffer h_meta;
    DeviceBuffer d_meta, d_model; // d_model: [mu of every camera][sigma6 of every camera], camera c at c * stride
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
            const size_t metaBytes = nj * (sizeof(abub_stat_job) + sizeof(abub_stat_result));
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
}

int surveyRun(Parser *parser, const std::vector<Trainer *> &trainers, int numCams, const std::string &format,
              const std::string &reportPath, int nthreads, int device, SurveyStats *stats, std::vector<SurveyRow> *rows,
              std::vector<SurveyModel> *models)
{
    const double t0 = nowMs();
    SurveyStats st;
    if (device >= 0) // (before anything else)
        requireDevice(device, "survey", "; without --survey-gpu the run is surveyed on the host");
    Plan pl = planRun(parser, trainers, numCams, format);
    st.events = (int)pl.events.size();
    st.W = pl.W;
    st.H = pl.H;
    for (const SurveyModel &m : pl.models)
        st.modelCams += m.trained;
    if (device >= 0 && pl.W > 0 && decodersTakeWidth(pl.W)) {
        st.device = device;
        deviceFrames(parser, pl, nthreads, device, st);
    } else
        hostFrames(parser, pl, nthreads);
    for (const SurveyRow &r : pl.rows) {
        long long *const counter[] = {&st.ok, &st.undecodable, &st.missing, &st.otherSize};
        ++*counter[r.state];
        ++st.frames;
        ++(r.onKernel ? st.framesKernel : st.framesHostRoute);
    }
    if (!reportPath.empty()) {
        const std::string text = SurveyReport(pl.models, pl.rows);
        if (!writeFile(reportPath, (const unsigned char *)text.data(), text.size()))
            throw std::runtime_error("survey: cannot write " + reportPath);
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
              std::vector<SurveyModel> *models)
{
    return surveyRun(parser, trainers, numCams, imageFormat, reportPath, nthreads, -1, stats, rows, models);
}

int SurveyRunDevice(Parser *parser, const std::vector<Trainer *> &trainers, int numCams, const std::string &imageFormat,
                    const std::string &reportPath, int nthreads, int device, SurveyStats *stats, std::vector<SurveyRow> *rows,
                    std::vector<SurveyModel> *models)
{
    if (device < 0)
        throw std::runtime_error("survey: no such HIP device: " + std::to_string(device));
    return surveyRun(parser, trainers, numCams, imageFormat, reportPath, nthreads, device, stats, rows, models);
}

} // namespace abub
