// verify.cpp -- a run compared with another copy of it, frame by frame ("Verifying a repacked run"):
// abub3hs --verify-repack.  No analysis.  Both runs are read through the Parser interface.  VerifyRun is host only and is
// the definition: both files through cv::imdecode, memcmp, and a byte loop for the numbers of a frame that differs.
// VerifyRunDevice (--verify-gpu) decodes the frames of the run's size on both sides with the GPU decoders and compares them
// with abub_frames_compare_dev; what the decoders do not take gets its verdict from the host route's per-frame function,
// of which there is one copy.  Both routes fill one verdict per task and share everything behind that: the counters, the
// findings in task order, the extras, the event file, the exit status.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <set>
#include <sstream>
#include <stdexcept>

#include "driver.hpp"
#include "framefiles.hpp"
#include "runbatch.hpp"
#include "runframes.hpp"

namespace abub {

const char *VerifyFinding::verdictName() const
{
    static const char *const names[] = {"same",    "same_not_packed", "copied",           "differ",            "missing",
                                        "undecodable", "extra",       "event_file_differs", "event_file_missing"};
    return names[verdict];
}

std::string VerifyFinding::text() const
{
    if (verdict == EventFileDiffers || verdict == EventFileMissing)
        return std::string("event file ") + name + (verdict == EventFileDiffers ? ": differs" : ": missing");
    std::string s = name.empty() ? event : event + "/" + name;
    char buf[160];
    switch (verdict) {
    case SameNotPacked:
        return s + ": same but not packed";
    case Differ:
        if (w != otherW || h != otherH)
            snprintf(buf, sizeof buf, ": differ: size %dx%d in the source, %dx%d in the other run", w, h, otherW, otherH);
        else
            snprintf(buf, sizeof buf, ": differ: %lld pixels, first at (x=%d, y=%d), max |a-b| = %d", ndiff, x, y, maxAbs);
        return s + buf;
    case Extra:
        return s + (name.empty() ? ": extra (an event the source does not list)" : ": extra (a frame the source does not list)");
    default:
        return s + ": " + verdictName();
    }
}

const char *VerifyStats::eventFileName() const
{
    static const char *const names[] = {"same", "differs", "missing", "not compared"};
    return names[eventFile];
}

namespace {

// what one frame got; the event and the name are the task's
struct Verdict {
    int verdict = VerifyFinding::Same;
    long long ndiff = 0;
    uint32_t first = 0;
    int maxAbs = 0, w = 0, h = 0, otherW = 0, otherH = 0;
    bool onKernel = false;
};

// `n` differing bytes of a W-wide frame, the first at index `first`
Verdict differing(long long n, uint32_t first, int maxAbs)
{
    Verdict v;
    v.verdict = VerifyFinding::Differ;
    v.ndiff = n;
    v.first = first;
    v.maxAbs = maxAbs;
    return v;
}

Verdict plain(int verdict)
{
    Verdict v;
    v.verdict = verdict;
    return v;
}

// identical pixels: a packed file says `same`
Verdict sameAs(const unsigned char *other, size_t on)
{
    int w = 0, h = 0;
    return plain(cv::abfProbe(other, on, &w, &h) ? VerifyFinding::Same : VerifyFinding::SameNotPacked);
}

// The definition: the source file's bytes against the other file's
Verdict verifyBytes(const unsigned char *s, size_t sn, const unsigned char *o, size_t on)
{
    const cv::Mat ms = sn ? cv::imdecode(s, sn, 0) : cv::Mat();
    if (ms.empty()) // (what repack does with such a file: it copies it)
        return plain(sn == on && (!sn || !std::memcmp(s, o, sn)) ? VerifyFinding::Copied : VerifyFinding::Undecodable);
    const cv::Mat mo = on ? cv::imdecode(o, on, 0) : cv::Mat();
    if (mo.empty())
        return plain(VerifyFinding::Undecodable);
    if (ms.cols != mo.cols || ms.rows != mo.rows) {
        Verdict v = plain(VerifyFinding::Differ);
        v.w = ms.cols;
        v.h = ms.rows;
        v.otherW = mo.cols;
        v.otherH = mo.rows;
        return v;
    }
    const size_t P = (size_t)ms.cols * ms.rows;
    if (!std::memcmp(ms.data, mo.data, P))
        return sameAs(o, on);
    long long n = 0;
    uint32_t first = 0;
    int maxAbs = 0;
    for (size_t i = 0; i < P; ++i)
        if (ms.data[i] != mo.data[i]) {
            if (!n++)
                first = (uint32_t)i;
            maxAbs = std::max(maxAbs, std::abs((int)ms.data[i] - (int)mo.data[i]));
        }
    Verdict v = differing(n, first, maxAbs);
    v.w = v.otherW = ms.cols; // (equal sizes; the width places `first`)
    v.h = v.otherH = ms.rows;
    return v;
}

// Each thread's clones of the two parsers
struct Clones {
    std::unique_ptr<Parser> src, other;
};

// The part of a verify that is not its frames' pixels
struct Plan {
    std::vector<std::string> events;
    std::vector<FrameTask> tasks;                // every frame of the source, in event, camera and frame order
    std::vector<std::set<std::string>> listed;   // listed[e]: the names the other run lists for events[e]
    std::vector<VerifyFinding> extras;
};

Plan planRun(Parser *src, Parser *other, int numCams)
{
    Plan pl;
    pl.events = sortedEvents(*src);
    pl.listed.resize(pl.events.size());
    std::vector<std::set<std::string>> mine(pl.events.size());
    for (size_t e = 0; e < pl.events.size(); ++e) {
        const size_t at = pl.tasks.size();
        appendEventFrames(*src, pl.events[e], e, numCams, pl.tasks);
        for (size_t i = at; i < pl.tasks.size(); ++i)
            mine[e].insert(pl.tasks[i].name);
    }
    for (const std::string &ev : sortedEvents(*other)) {
        const size_t e = std::find(pl.events.begin(), pl.events.end(), ev) - pl.events.begin();
        VerifyFinding f;
        f.verdict = VerifyFinding::Extra;
        f.event = ev;
        if (e == pl.events.size()) {
            pl.extras.push_back(f);
            continue;
        }
        std::vector<FrameTask> theirs;
        appendEventFrames(*other, ev, e, numCams, theirs);
        for (FrameTask &t : theirs) {
            if (!mine[e].count(t.name) && !pl.listed[e].count(t.name)) {
                f.name = t.name;
                pl.extras.push_back(f);
            }
            pl.listed[e].insert(std::move(t.name));
        }
    }
    return pl;
}

// The host route's per-frame function: task i on this thread, both files through its parsers
Verdict verifyFrame(Clones &c, const Plan &pl, size_t i)
{
    static thread_local std::vector<unsigned char> a, b;
    const FrameTask &t = pl.tasks[i];
    if (!pl.listed[t.ev].count(t.name))
        return plain(VerifyFinding::Missing);
    readWhole(*c.src, pl.events[t.ev], t.name, a);
    readWhole(*c.other, pl.events[t.ev], t.name, b);
    return verifyBytes(a.data(), a.size(), b.data(), b.size());
}

template <class Fn>
void forEachPair(Parser *src, Parser *other, int nthreads, size_t n, const Fn &fn)
{
    forEachTaskWith(
        nthreads, n, [&]() { return Clones{std::unique_ptr<Parser>(src->clone()), std::unique_ptr<Parser>(other->clone())}; }, fn);
}

void hostFrames(Parser *src, Parser *other, const Plan &pl, int nthreads, std::vector<Verdict> &verdicts)
{
    forEachPair(src, other, nthreads, pl.tasks.size(), [&](Clones &c, size_t i) { verdicts[i] = verifyFrame(c, pl, i); });
}

// The device route: the frames in batches.  Per batch and side: the pool reads the files into a pinned buffer (a frame
// that is no file for the decoders on either side gets its verdict on the spot, from verifyFrame); upload; both decoders
// into the side's slab, frame i at i * align16(W * H); then one abub_frames_compare_dev launch over the frames that are in
// place on both sides, and the records back in one copy.  What a decoder refused behind its header goes to verifyFrame too.
void deviceFrames(Parser *src, Parser *other, const Plan &pl, int nthreads, int device, int W, int H, VerifyStats &st,
                  std::vector<Verdict> &verdicts)
{
    HIPOK(hipSetDevice(device));
    size_t perBatch = framesPerBatch(device);
    if (const char *e = getenv("ABUB_VERIFY_BATCH"))
        if (atoi(e) > 0)
            perBatch = (size_t)atoi(e);
    const size_t P = (size_t)W * H, stride = (P + 15) & ~(size_t)15;
    FileBatch S, O; // the two sides of a batch: the files, the decoders' scratch, the slab of decoded frames
    S.sizer.reset(src->clone());
    O.sizer.reset(other->clone());
    PinnedBuffer h_meta;
    DeviceBuffer d_meta;
    Stream stream;
    hipStream_t cs = stream.get();
    long long srcUnzipped = 0, otherUnzipped = 0;

    for (size_t i0 = 0; i0 < pl.tasks.size(); i0 += perBatch) {
        const size_t n = std::min(perBatch, pl.tasks.size() - i0);
        // ---- read -------------------------------------------------------------------------------------------------------
        double t0 = nowMs();
        std::vector<uint8_t> done(n, 0); // the frame has its verdict
        for (FileBatch *side : {&S, &O}) {
            side->begin();
            side->reset(n, n * stride);
        }
        for (size_t i = 0; i < n; ++i) {
            const FrameTask &t = pl.tasks[i0 + i];
            S.plan((int)i, 0, pl.events[t.ev], t.name);
            if (!pl.listed[t.ev].count(t.name))
                O.plan((int)i, 0, pl.events[t.ev], t.name, false).state = FileTask::Bad;
            else
                O.plan((int)i, 0, pl.events[t.ev], t.name);
        }
        S.ready();
        O.ready();
        // A pair is read when both its files are there to be read, the source first, and once more (`second`) when a side of it
        // waited for the device's inflate of its archive entry (ABUB_GPU_UNZIP=1); it is final only when neither side waits
        const auto readPair = [&](Clones &c, size_t i, bool second) {
            const FrameTask &t = pl.tasks[i0 + i];
            FileTask &fs = S.ft[i], &fo = O.ft[i];
            if (second || (fs.state == FileTask::Planned && fo.state == FileTask::Planned)) {
                bool settled = S.read(*c.src, i, pl.events[t.ev], t.name, W, H);
                if (fs.state != FileTask::Bad)
                    settled = O.read(*c.other, i, pl.events[t.ev], t.name, W, H) && settled;
                if (!settled)
                    return;
            }
            const bool sOk = fs.onGpu() || fs.state == FileTask::HostDecoded, oOk = fo.onGpu() || fo.state == FileTask::HostDecoded;
            if (sOk && oOk)
                return;
            verdicts[i0 + i] = verifyFrame(c, pl, i0 + i);
            done[i] = 1;
            fs.pix = fo.pix = std::vector<uint8_t>();
            fs.state = fo.state = FileTask::Other;
        };
        forEachPair(src, other, nthreads, n, [&](Clones &c, size_t i) { readPair(c, i, false); });
        S.inflateOnDevice(cs);
        O.inflateOnDevice(cs);
        std::vector<size_t> waited; // the pairs a side of which waited
        std::set_union(S.pending().begin(), S.pending().end(), O.pending().begin(), O.pending().end(), std::back_inserter(waited));
        if (!waited.empty())
            forEachPair(src, other, nthreads, waited.size(), [&](Clones &c, size_t k) { readPair(c, waited[k], true); });
        srcUnzipped += S.unzip.unzipped;
        otherUnzipped += O.unzip.unzipped;
        st.srcGpuUnzipped = srcUnzipped;
        st.otherGpuUnzipped = otherUnzipped;
        st.read_s += (nowMs() - t0) * 1e-3;

        // ---- upload and decode ------------------------------------------------------------------------------------------
        t0 = nowMs();
        const auto dstOf = [&](int s, int) { return (uint64_t)s * stride; };
        S.upload(cs);
        O.upload(cs);
        S.launch(0, n, W, H, dstOf, cs);
        O.launch(0, n, W, H, dstOf, cs);
        HIPOK(hipStreamSynchronize(cs));
        S.finish(W, H, cs);
        O.finish(W, H, cs);
        st.srcGpuPngDecoded = S.decodedBy[GpuPng];
        st.srcGpuUnpacked = S.decodedBy[GpuPacked];
        st.srcGpuBmpDecoded = S.decodedBy[GpuBmp];
        st.srcHostDecoded = S.hostDecoded;
        st.otherGpuPngDecoded = O.decodedBy[GpuPng];
        st.otherGpuUnpacked = O.decodedBy[GpuPacked];
        st.otherGpuBmpDecoded = O.decodedBy[GpuBmp];
        st.otherHostDecoded = O.hostDecoded;
        HIPOK(hipStreamSynchronize(cs));
        st.decode_s += (nowMs() - t0) * 1e-3;

        // ---- compare: [pairs][results] in one buffer ------------------------------------------------------------------------
        t0 = nowMs();
        std::vector<size_t> slot;
        for (size_t i = 0; i < n; ++i)
            if (!done[i] && S.good[i] && O.good[i])
                slot.push_back(i);
        const size_t np = slot.size();
        if (np) {
            const size_t metaBytes = np * (sizeof(abub_cmp_pair) + sizeof(abub_cmp_result));
            h_meta.grow(metaBytes);
            d_meta.grow(metaBytes);
            abub_cmp_pair *pairs = (abub_cmp_pair *)h_meta.get();
            for (size_t g = 0; g < np; ++g)
                pairs[g].a = pairs[g].b = (uint64_t)slot[g] * stride;
            HIPOK(hipMemcpyAsync(d_meta.get(), h_meta.get(), np * sizeof(abub_cmp_pair), hipMemcpyHostToDevice, cs));
            abub_cmp_result *d_res = (abub_cmp_result *)(d_meta.get() + np * sizeof(abub_cmp_pair));
            const abub_cmp_result *res = (const abub_cmp_result *)(h_meta.get() + np * sizeof(abub_cmp_pair));
            check(abub_frames_compare_dev(S.slab.get(), n * stride, O.slab.get(), n * stride, (const abub_cmp_pair *)d_meta.get(), (int)np,
                                          P, d_res, cs),
                  "abub_frames_compare_dev");
            HIPOK(hipMemcpyAsync(h_meta.get() + np * sizeof(abub_cmp_pair), d_res, np * sizeof(abub_cmp_result), hipMemcpyDeviceToHost, cs));
            HIPOK(hipStreamSynchronize(cs));
            for (size_t g = 0; g < np; ++g) {
                const size_t i = slot[g];
                const abub_cmp_result &r = res[g];
                if (r.status != 0)
                    throw std::runtime_error("verify: abub_frames_compare_dev refused a frame of its own slab");
                Verdict v = r.ndiff ? differing(r.ndiff, r.first, (int)r.max_abs) : sameAs(O.h_files.get() + O.ft[i].off, (size_t)O.ft[i].size);
                v.w = v.otherW = W;
                v.h = v.otherH = H;
                v.onKernel = true;
                verdicts[i0 + i] = v;
                done[i] = 1;
            }
        }
        st.compare_s += (nowMs() - t0) * 1e-3;

        // ---- what the decoders left (a file that is damaged behind its header): the host route's answer -------------------
        t0 = nowMs();
        std::vector<size_t> left;
        for (size_t i = 0; i < n; ++i)
            if (!done[i])
                left.push_back(i);
        forEachPair(src, other, nthreads, left.size(),
                    [&](Clones &c, size_t k) { verdicts[i0 + left[k]] = verifyFrame(c, pl, i0 + left[k]); });
        st.read_s += (nowMs() - t0) * 1e-3;
        ++st.batches;
    }
}

// 0 .. 3 of VerifyStats::EventFile
int compareEventFiles(const std::string &srcRunFile, const std::string &otherRunFile)
{
    if (srcRunFile.empty() || otherRunFile.empty())
        return VerifyStats::FileNotCompared;
    std::ifstream a(srcRunFile, std::ios::binary), b(otherRunFile, std::ios::binary);
    if (!a)
        return VerifyStats::FileNotCompared; // (repack then wrote a file of its own making)
    if (!b)
        return VerifyStats::FileMissing;
    std::ostringstream sa, sb;
    sa << a.rdbuf();
    sb << b.rdbuf();
    return sa.str() == sb.str() ? VerifyStats::FileSame : VerifyStats::FileDiffers;
}

// The same where the copy is an archive: its side is the bytes of its <run>.txt entry, the source's side its file or, for a
// zipped source, its own entry
int compareEventFileBytes(Parser *src, Parser *other, const std::string &srcRunFile)
{
    std::string a, b;
    std::ifstream in(srcRunFile, std::ios::binary);
    if (!srcRunFile.empty() && in) {
        std::ostringstream sa;
        sa << in.rdbuf();
        a = sa.str();
    } else if (!src->GetRunFileBytes(a))
        return VerifyStats::FileNotCompared; // (repack then wrote a file of its own making)
    if (!other->GetRunFileBytes(b))
        return VerifyStats::FileMissing;
    return a == b ? VerifyStats::FileSame : VerifyStats::FileDiffers;
}

int verifyRun(Parser *src, Parser *other, const std::string &srcRunFile, const std::string &otherRunFile, int numCams, int nthreads,
              int device, VerifyStats *stats, std::vector<VerifyFinding> *findings, bool otherIsArchive)
{
    const double t0 = nowMs();
    VerifyStats st;
    if (device >= 0) // (before anything else)
        requireDevice(device, "verify", "; without --verify-gpu the run is verified on the host");
    const Plan pl = planRun(src, other, numCams);
    st.events = (int)pl.events.size();
    std::vector<Verdict> verdicts(pl.tasks.size());
    int W = 0, H = 0;
    if (device >= 0 && firstFrameSize(src, pl.events, pl.tasks, W, H) && decodersTakeWidth(W)) {
        st.device = device;
        st.W = W;
        st.H = H;
        deviceFrames(src, other, pl, nthreads, device, W, H, st, verdicts);
    } else
        hostFrames(src, other, pl, nthreads, verdicts);

    // ---- the verdicts into the counters and, in task order, into the findings -------------------------------------------------
    std::vector<VerifyFinding> found;
    for (size_t i = 0; i < verdicts.size(); ++i) {
        const Verdict &v = verdicts[i];
        long long *const counter[] = {&st.same, &st.sameNotPacked, &st.copied, &st.differ, &st.missing, &st.undecodable};
        ++*counter[v.verdict];
        ++st.frames;
        ++(v.onKernel ? st.framesKernel : st.framesHostRoute);
        if (v.verdict == VerifyFinding::Same || v.verdict == VerifyFinding::Copied)
            continue;
        VerifyFinding f;
        f.verdict = v.verdict;
        f.event = pl.events[pl.tasks[i].ev];
        f.name = pl.tasks[i].name;
        if (v.verdict == VerifyFinding::Differ) {
            if (v.w != v.otherW || v.h != v.otherH) {
                f.w = v.w;
                f.h = v.h;
                f.otherW = v.otherW;
                f.otherH = v.otherH;
            } else {
                f.ndiff = v.ndiff;
                f.x = (int)(v.first % (uint32_t)v.w);
                f.y = (int)(v.first / (uint32_t)v.w);
                f.maxAbs = v.maxAbs;
            }
        }
        found.push_back(std::move(f));
    }
    st.extra = (long long)pl.extras.size();
    found.insert(found.end(), pl.extras.begin(), pl.extras.end());
    st.eventFile = otherIsArchive ? compareEventFileBytes(src, other, srcRunFile) : compareEventFiles(srcRunFile, otherRunFile);
    if (st.eventFile == VerifyStats::FileDiffers || st.eventFile == VerifyStats::FileMissing) {
        VerifyFinding f;
        f.verdict = st.eventFile == VerifyStats::FileDiffers ? VerifyFinding::EventFileDiffers : VerifyFinding::EventFileMissing;
        const size_t slash = otherRunFile.find_last_of('/');
        f.name = slash == std::string::npos ? otherRunFile : otherRunFile.substr(slash + 1);
        found.push_back(std::move(f));
    }
    bool failed = false;
    for (const VerifyFinding &f : found)
        failed = failed || f.failure();
    st.total_s = (nowMs() - t0) * 1e-3;
    if (stats)
        *stats = st;
    if (findings)
        *findings = std::move(found);
    return failed ? 1 : 0;
}

} // namespace

int VerifyRun(Parser *src, Parser *other, const std::string &srcRunFile, const std::string &otherRunFile, int numCams, int nthreads,
              VerifyStats *stats, std::vector<VerifyFinding> *findings, bool otherIsArchive)
{
    return verifyRun(src, other, srcRunFile, otherRunFile, numCams, nthreads, -1, stats, findings, otherIsArchive);
}

int VerifyRunDevice(Parser *src, Parser *other, const std::string &srcRunFile, const std::string &otherRunFile, int numCams,
                    int nthreads, int device, VerifyStats *stats, std::vector<VerifyFinding> *findings, bool otherIsArchive)
{
    if (device < 0)
        throw std::runtime_error("verify: no such HIP device: " + std::to_string(device));
    return verifyRun(src, other, srcRunFile, otherRunFile, numCams, nthreads, device, stats, findings, otherIsArchive);
}

} // namespace abub
