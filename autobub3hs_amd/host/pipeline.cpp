// pipeline.cpp -- run-level batched driver: every (event, camera) stack of a run is resident in HBM
// as one slab [E][C][F][H][W]; the GPU work of ALL stacks is issued in a handful of launches per
// stage, the per-event state machines (the same AnalyzerUnit / L3Localizer code as the drop-in path)
// run on host threads in between.  This is what bench.py times as "end-to-end detect".
//
//   stage 1  K2 trigger-only over every frame of every stack        -> [S][F-1][256] histograms
//   stage 2  host: FindTriggerFrame per stack (AnyCamAnalysis loop, AutoBubStart3.cpp:87-110)
//   stage 3  K2 store for the genesis pairs, K3 for the post-trigger frames, Otsu thresholds on the
//            host from the histograms, K4 compaction of all foreground pixels into one list
//   stage 4  host: LocalizeOMatic per stack (contours, blobs, tracking)
//   stacks whose trigger produced no accepted bubble go round again from the next frame.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "AlgorithmTraining/Trainer.hpp"
#include "AnalyzerUnit.hpp"
#include "BubbleLocalizer/L3Localizer.hpp"
#include "ParseFolder/Parser.hpp"
#include "common/CommonParameters.h"
#include "PICOFormatWriter/PICOFormatWriterV4.hpp"
#include "devctx.hpp"
#include "driver.hpp"
#include "holders.hpp"
#include "hostlogic.hpp"
#include "pipeline.hpp"
#include "stackresult.hpp"

namespace abub {
extern bool g_quietAnalyzers;
// trigger knob, summed over every pipeline run of the process (a batched run owns its pipelines; abh_pipe_trigger_totals):
// stacks searched on the device, stacks on the host route
static std::atomic<long long> g_trigTotals[2];
// localize knob, likewise (abh_pipe_localize_totals): stacks localised on the device, stacks on the host route
static std::atomic<long long> g_locTotals[2];

namespace {

// FindTriggerFrame's frame offset: frame i is differenced against frame max(i - off, 0), off = 1 when the model was
// trained on fewer than 6 frames (AnalyzerUnit.cpp:185-188)
int refOffset(int tss) { return tss < 6 ? 1 : 2; }
// that offset when every camera shares it, else 0
int chainStrideOf(const int *tss, int C)
{
    for (int c = 1; c < C; ++c)
        if (refOffset(tss[c]) != refOffset(tss[0]))
            return 0;
    return refOffset(tss[0]);
}
// the bellows templates are Mats of the process-wide mask cache: the same template is the same buffer
bool sameTemplate(const cv::Mat &a, const cv::Mat &b) { return a.data == b.data && a.cols == b.cols && a.rows == b.rows; }

struct PlannedImage {
    int kind = 0; // 0 = D(i; ref) (genesis), 1 = post-trigger image of frame i, 2 = bellows residual of D(i; ref)
    int i = 0, ref = 0;
    int slot = -1; // index into the image / histogram slabs of this round
    int tozero = 0;
    int thr = 0;
    // an image that waits for its batch: no slot, no Otsu threshold yet
    static PlannedImage make(int kind, int i, int ref, int tozero, int minBox)
    {
        PlannedImage p;
        p.kind = kind, p.i = i, p.ref = ref, p.tozero = tozero, p.minBox = minBox;
        return p;
    }
    const uint32_t *fg = nullptr; // raster indices of the candidate pixels (value > tozero), grouped on the GPU
    const uint8_t *fgv = nullptr; // their values: the Otsu cut is applied on the host
    uint32_t nfg = 0;
    int minBox = -1; // the localizer drops contours with box area <= minBox (-1: keeps all): kTrackMinBoxArea when tracking
    // blobs knob: the pixels of the kept components (K4b, abub_blobs.hip) in raster order, labelled on the device with the
    // device's Otsu threshold (kept == nullptr: served from fg / fgv)
    const uint32_t *kept = nullptr;
    uint32_t nkept = 0;
    bool otsuMismatch = false; // the device's Otsu threshold differs from the host's (parity tripwire)
    // contours knob: the contours of the kept pixels traced on the device (K5, abub_contours.hip): contour k has cnp[k]
    // vertices, one after the other in cpts (x | y << 16).  traced == false: the slot takes the host route from `kept`
    bool traced = false;
    bool keptShipped = true; // false: the batch had no declined slot, so its kept pixels stayed on the device
    const uint32_t *cnp = nullptr, *cpts = nullptr;
    uint32_t ncont = 0;
    bool vertsShipped = true; // false (localize knob): every stack of the batch was localised on the device, the vertices stayed there
};

// thrown by the batched provider when the trigger search asks for a frame whose block has not been evaluated yet: the
// pipeline evaluates that block for the stack and runs the search again (see RunPipeline::runGroup)
struct NeedMoreFrames : public std::runtime_error {
    NeedMoreFrames() : std::runtime_error("trigger search needs the next block of frames") {}
};

// thrown by the batched provider when the bellows veto asks for a template match or a residual image that has not been
// computed yet: the request is recorded, the pipeline serves all of them in a veto round and runs localize again (see
// RunPipeline::vetoRound).  Both throws come before LocalizeOMatic pushes anything to bubbleRects or BubbleList.
struct NeedBellows : public std::runtime_error {
    NeedBellows() : std::runtime_error("bellows veto waits for the batched match / residual") {}
};

// EventData served from the pipeline's batched results
class BatchEventData : public EventData {
public:
    // The trigger search's histograms arrive in blocks of frames: block k covers frames [bstart[k], bstart[k + 1]).
    // ref[k] is this stack's part of block k, bound when launch `fetch` of the block is queued for it (Group::Search::Block::
    // bind): its first job in the block's buffers, frame i's histogram at hist + (i - bstart[k]) * 256, and inc (deferred
    // launches only): per frame, 1 while the histogram is not final -- its dense rows were handed over by the bound scan and
    // the row machine has not run on them yet (deferred pieces); cleared when they are completed.  histDev / incDev: the same in
    // device memory, what the device search reads from the launch on.  The host search reads hist / inc only once the block
    // has `arrived`: the launch has been waited for
    struct BlockRef {
        int fetch = -1;
        bool arrived = false;
        size_t job = 0;
        const uint32_t *hist = nullptr, *histDev = nullptr;
        uint8_t *inc = nullptr;
        const uint8_t *incDev = nullptr;
        bool launched() const { return fetch >= 0; }
        bool deferred() const { return inc != nullptr; }
    };
    static constexpr int MAXB = 32;
    int nblocks = 0;
    int bstart[MAXB + 1] = {0};
    BlockRef ref[MAXB];
    int blockOf(int frame) const
    {
        int k = 0;
        while (k + 1 < nblocks && frame >= bstart[k + 1])
            ++k;
        return k;
    }
    // What a search that stopped asks for (the host's diffHist, or the device's answer): block `block` for this stack, or
    // (pieces) that block is there, but frame `frame` and the later ones must be completed.  block < 0: nothing
    struct Need {
        int block = -1, frame = 0;
        bool pieces = false;
    } need;
    bool asked() const { return need.block >= 0; }
    void request(int block, int frame, bool pieces) { need = Need{block, frame, pieces}; }
    void clearNeed() { need = Need(); }
    int tss = 0, refOffset = 2; // the camera's training set size and FindTriggerFrame's frame offset for it
    const uint32_t *roundHists = nullptr; // [nslots][256] of the current round
    std::vector<PlannedImage> planned;
    const PlannedImage *cur = nullptr;
    // bellows veto memos of the current trigger (cleared when the search moves on): template matches keyed by frame and
    // template, residual images keyed by (trig, pre, rt, rp); entries with ready == false are requests
    bool bellowsDropIn = false; // ABUB_PIPE_BELLOWS=dropin: the veto goes through the one-at-a-time path
    struct MatchMemo {
        int frame;
        cv::Mat templ;
        bool ready;
        cv::Point2f xy;
    };
    struct ResidualMemo {
        int trig, pre;
        cv::Rect rt, rp, roi;
        cv::Mat templ;
        bool ready;
        uint32_t hist[256];
        PlannedImage img;
    };
    std::vector<MatchMemo> matches;
    std::vector<ResidualMemo> residuals; // (cur points into it only until the next request)
    void clearVeto()
    {
        matches.clear();
        residuals.clear();
    }
    const uint8_t *ok = nullptr; // per-frame "decoded" flags of a stack that came from disk (NULL: all good)

    bool frameOk(int i) const override { return i >= 0 && i < F && (!ok || ok[i]); }
    // the first frame that was not decoded (F: none)
    int firstBad() const
    {
        int i = 0;
        while (i < F && frameOk(i))
            ++i;
        return i;
    }
    cv::Mat hostFrame(int) const override { return cv::Mat(); }
    const uint32_t *diffHist(int i, int off) override
    {
        if (off != refOffset || i < 1 || i >= F)
            throw std::runtime_error("BatchEventData::diffHist: unplanned request");
        const int k = blockOf(i);
        const BlockRef &b = ref[k];
        if (!b.arrived || (b.inc && b.inc[i - bstart[k]])) {
            request(k, i, b.arrived);
            throw NeedMoreFrames();
        }
        return b.hist + (size_t)(i - bstart[k]) * 256;
    }
    const uint32_t *find(int kind, int i, int ref)
    {
        for (size_t k = 0; k < planned.size(); ++k)
            if (planned[k].kind == kind && planned[k].i == i && (kind == 1 || planned[k].ref == ref)) {
                cur = &planned[k];
                return roundHists + (size_t)planned[k].slot * 256;
            }
        throw std::runtime_error("BatchEventData: image was not planned for this round");
    }
    const uint32_t *diffFrame(int i, int ref, cv::Mat *) override { return find(0, i, ref); }
    const uint32_t *diffFrameROI(int, int, cv::Rect, cv::Mat *) override
    {
        throw std::runtime_error("BatchEventData: ROI diff is not available in the batched path");
    }
    const uint32_t *postTrig(int i, cv::Mat *) override { return find(1, i, 0); }
    void matchTerms(int, const cv::Mat &, std::vector<unsigned long long> &, std::vector<unsigned long long> &) override
    {
        throw NeedsDropInPath("bellows veto requested in the batched path");
    }
    const uint32_t *subtractFromCurrent(const cv::Mat &) override
    {
        throw NeedsDropInPath("bellows veto requested in the batched path");
    }
    static bool same(const cv::Rect &a, const cv::Rect &b)
    {
        return a.x == b.x && a.y == b.y && a.width == b.width && a.height == b.height;
    }
    MatchMemo *findMatch(int i, const cv::Mat &templ)
    {
        for (MatchMemo &m : matches)
            if (m.frame == i && sameTemplate(m.templ, templ))
                return &m;
        return nullptr;
    }
    void requestMatch(int i, const cv::Mat &templ)
    {
        if (!findMatch(i, templ))
            matches.push_back(MatchMemo{i, templ, false, cv::Point2f()});
    }
    cv::Point2f bestMatch(int i, const cv::Mat &templ) override
    {
        if (bellowsDropIn)
            throw NeedsDropInPath("bellows veto requested in the batched path");
        if (MatchMemo *m = findMatch(i, templ))
            if (m->ready)
                return m->xy;
        requestMatch(i, templ);
        // the veto always locates the template in the genesis pair's two frames: ask for both in one match round
        for (const PlannedImage &p : planned)
            if (p.kind == 0 && p.i == i)
                requestMatch(p.ref, templ);
        throw NeedBellows();
    }
    const uint32_t *bellowsResidual(int trig, int pre, const cv::Mat &templ, cv::Rect rt, cv::Rect rp, cv::Rect roi) override
    {
        if (bellowsDropIn)
            throw NeedsDropInPath("bellows veto requested in the batched path");
        for (ResidualMemo &r : residuals)
            if (r.trig == trig && r.pre == pre && same(r.rt, rt) && same(r.rp, rp) && same(r.roi, roi) && r.templ.data == templ.data) {
                if (!r.ready)
                    throw NeedBellows();
                cur = &r.img;
                return r.hist;
            }
        ResidualMemo r{};
        r.trig = trig;
        r.pre = pre;
        r.rt = rt;
        r.rp = rp;
        r.roi = roi;
        r.templ = templ;
        r.ready = false;
        residuals.push_back(r);
        throw NeedBellows();
    }
    void foreground(int thr, std::vector<uint32_t> &idx) override
    {
        if (!cur || cur->thr != thr)
            throw std::runtime_error("BatchEventData::foreground: threshold differs from the planned one");
        const PlannedImage &p = *cur;
        idx.clear();
        for (uint32_t k = 0; k < p.nfg; ++k)
            if ((int)p.fgv[k] > thr)
                idx.push_back(p.fg[k]);
    }
    void foregroundKept(int thr, int minBoxArea, std::vector<uint32_t> &idx) override
    {
        if (!cur || cur->thr != thr || cur->minBox != minBoxArea)
            throw std::runtime_error("BatchEventData::foregroundKept: threshold or min box area differs from the planned one");
        const PlannedImage &p = *cur;
        if (!p.kept) {
            foreground(thr, idx);
            return;
        }
        if (p.otsuMismatch)
            throw std::runtime_error("BatchEventData::foregroundKept: device Otsu threshold differs from the host's");
        if (!p.keptShipped)
            throw std::runtime_error("BatchEventData::foregroundKept: the kept pixels of a traced image stayed on the device");
        idx.assign(p.kept, p.kept + p.nkept);
    }
    bool contoursKept(int thr, int minBoxArea, std::vector<std::vector<cv::Point>> &out) override
    {
        if (!cur || cur->thr != thr || cur->minBox != minBoxArea)
            throw std::runtime_error("BatchEventData::contoursKept: threshold or min box area differs from the planned one");
        const PlannedImage &p = *cur;
        if (!p.traced)
            return false;
        if (p.otsuMismatch)
            throw std::runtime_error("BatchEventData::contoursKept: device Otsu threshold differs from the host's");
        if (!p.vertsShipped)
            throw std::runtime_error("BatchEventData::contoursKept: the vertices of a localised batch stayed on the device");
        out.resize(p.ncont);
        const uint32_t *q = p.cpts;
        for (uint32_t k = 0; k < p.ncont; ++k) {
            std::vector<cv::Point> &c = out[k];
            c.resize(p.cnp[k]);
            for (uint32_t v = 0; v < p.cnp[k]; ++v, ++q)
                c[v] = cv::Point((int)(*q & 0xffffu), (int)(*q >> 16));
        }
        return true;
    }
    // localize knob: the finished localisation of the planned trigger (K7, abub_localize.hip) in the round's lists; valid
    // from batchImages() until the search plans the next trigger
    bool locReady = false;
    int locTrig = -1;
    abub_loc_result locRes{};
    const int32_t *locRects = nullptr;
    const uint32_t *locTracks = nullptr;
    const abub_contour_desc *locDesc = nullptr;
    bool localized(int trig, std::vector<cv::Rect> &rects, std::vector<std::vector<BubbleImageFrame>> &tracks) override
    {
        if (!locReady || trig != locTrig)
            return false;
        const int32_t *r = locRects + 4 * (size_t)locRes.rect_off;
        for (uint32_t k = 0; k < locRes.nrects; ++k, r += 4)
            rects.push_back(cv::Rect(r[0], r[1], r[2], r[3]));
        const uint32_t *t = locTracks + locRes.track_off;
        tracks.resize(locRes.nbubbles);
        for (uint32_t b = 0; b < locRes.nbubbles; ++b) {
            const uint32_t n = *t++;
            for (uint32_t j = 0; j < n; ++j) {
                const abub_contour_desc &d = locDesc[*t++];
                BubbleImageFrame f;
                f.ContArea = d.area;
                f.newPosition = cv::Rect(d.x, d.y, d.w, d.h);
                f.moments = cv::Moments();
                f.moments.m00 = d.m00;
                f.moments.m10 = d.m10;
                f.moments.m01 = d.m01;
                f.ContRadius = d.radius;
                f.MassCentres = j == 0 ? cv::Point2f(d.gx, d.gy) : cv::Point2f(d.cx, d.cy); // genesis / tracking form
                tracks[b].push_back(f);
            }
        }
        return true;
    }
};

// the stack's result (a stack that ends before its first trigger reports the analyzer's initial loc_thres and
// okToProceed) and its state while the run is on
struct StackState : StackResult {
    StackState()
    {
        loc_thres = 3;
        ok = 1;
    }
    std::unique_ptr<L3Localizer> analyzer;
    BatchEventData data;
    bool done = false;
    bool localize = false;
    bool dropIn = false; // must be re-run through the one-at-a-time path (bellows veto)
    // (the trigger search stopped at frames that are not evaluated yet: data.asked())
    bool needBellows = false; // localize stopped at a bellows-veto request (data.matches / data.residuals)
    // trigger knob: the device search's answer for the analyzer's current state (trigReady: not consumed yet)
    bool trigReady = false;
    abub_trig_result trigRes{};
    bool vetoed = false;      // a bellows residual was computed for this stack in the batch
    size_t rectsBegin = 0;    // the analyzer's bubbleRects before its last LocalizeOMatic round
};

// Persistent worker pool shared by all stack groups: a group that is waiting for the GPU lends its
// threads to the groups that are in their host stages (no per-call thread creation either).
class WorkerPool {
public:
    explicit WorkerPool(int nthreads)
    {
        for (int t = 0; t < nthreads; ++t)
            workers.emplace_back([this]() { workerLoop(); });
    }
    ~WorkerPool()
    {
        {
            std::lock_guard<std::mutex> lock(mu);
            stop = true;
        }
        cv.notify_all();
        for (auto &t : workers)
            t.join();
    }
    // runs fn(0..n-1); the caller takes part, returns when every index is done
    void parallelFor(int n, const std::function<void(int)> &fn)
    {
        if (n <= 0)
            return;
        if (n == 1 || workers.empty()) {
            for (int i = 0; i < n; ++i)
                fn(i);
            return;
        }
        auto batch = std::make_shared<Batch>();
        batch->n = n;
        batch->fn = &fn;
        batch->remaining = n;
        {
            std::lock_guard<std::mutex> lock(mu);
            batches.push_back(batch);
        }
        cv.notify_all();
        runBatch(*batch); // help
        std::unique_lock<std::mutex> lock(mu);
        batch->done.wait(lock, [&] { return batch->remaining == 0; });
        for (auto it = batches.begin(); it != batches.end(); ++it)
            if (it->get() == batch.get()) {
                batches.erase(it);
                break;
            }
    }

private:
    struct Batch {
        int n = 0;
        const std::function<void(int)> *fn = nullptr;
        std::atomic<int> next{0};
        int remaining = 0; // guarded by mu
        std::condition_variable done;
    };
    void runBatch(Batch &b)
    {
        int finished = 0;
        for (;;) {
            const int i = b.next.fetch_add(1);
            if (i >= b.n)
                break;
            (*b.fn)(i);
            ++finished;
        }
        if (finished) {
            std::lock_guard<std::mutex> lock(mu);
            b.remaining -= finished;
            if (b.remaining == 0)
                b.done.notify_all();
        }
    }
    void workerLoop()
    {
        std::unique_lock<std::mutex> lock(mu);
        for (;;) {
            std::shared_ptr<Batch> pick;
            for (auto &b : batches)
                if (b->next.load() < b->n) {
                    pick = b;
                    break;
                }
            if (pick) {
                lock.unlock();
                runBatch(*pick);
                lock.lock();
                continue;
            }
            if (stop)
                return;
            cv.wait(lock);
        }
    }
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::shared_ptr<Batch>> batches;
    std::vector<std::thread> workers;
    bool stop = false;
};

} // namespace

// The candidate pixels of a batch of images (stage 3, or the veto's residuals): (raster index, value) pairs as the
// compaction kernels write them, grouped by image on the device, and the host mirrors the localizer reads
struct CandidateList {
    // gidx carries the capacity in pairs, cap(): it is the list that is seeded, grows (slack 1024, at most 2^30 pairs) and
    // is checked for overflow; the other arrays follow it at the start of the next batch (start())
    GrowList<uint32_t> gidx{1024, 1, 1u << 30};
    Mirror<uint8_t> gval;
    DeviceArray<uint32_t> pairs;    // [2 cap]
    size_t followed = 0;            // the capacity pairs and gval were made for
    DeviceArray<uint32_t> gscratch; // [2 nimg]
    Mirror<uint32_t> count, goff;   // pairs found (the kernels count past cap); image k's pairs are [goff[k], goff[k + 1])
    // blobs knob (stage 3): the kept pixels are a subset of the candidates, so the kept list and K4b's scratch follow cap too
    int keptImages = 0, keptW = 0, keptH = 0; // images of W x H the kept list has room for from the next start() on (0: none)
    Mirror<uint32_t> kidx;
    DeviceArray<uint8_t> keptScratch;
    size_t keptScratchBytes = 0, keptFollowed = 0;

    uint32_t cap() const { return (uint32_t)gidx.cap(); }
    // room for the per-image arrays of `nimg` images
    void allocate(size_t nimg)
    {
        count.allocate(1);
        gscratch.allocate(2 * nimg);
        goff.allocate(nimg + 1);
    }
    // before the launches of a batch: the arrays that follow the capacity are made for it (the streams that used the old
    // ones have been synchronised: gidx has grown, or the kept list is new), the count is zeroed
    void start(hipStream_t s)
    {
        if (followed != gidx.cap()) {
            pairs.allocate(2 * gidx.cap());
            gval.allocate(gidx.cap());
            followed = gidx.cap();
        }
        if (keptImages && keptFollowed != gidx.cap()) {
            keptScratchBytes = abub_label_blobs_scratch_bytes(keptImages, keptW, keptH, cap(), 0);
            if (keptScratchBytes == 0)
                throw std::runtime_error("RunPipeline: frame size not supported by the blob labelling");
            keptScratch.allocate(keptScratchBytes);
            kidx.allocate(gidx.cap());
            keptFollowed = gidx.cap();
        }
        HIPOK(hipMemsetAsync(count.d, 0, sizeof(uint32_t), s));
    }
    // the pairs grouped by image (per-image counts from the histograms and TOZERO cuts of the same launches)
    void group(int nimg, const uint32_t *d_hist, const int32_t *d_thr, hipStream_t s, const char *what)
    {
        check(abub_pairs_group_hist_dev(pairs, count.d, cap(), nimg, gscratch, goff.d, gidx.d, gval.d, d_hist, d_thr, s), what);
    }
    void offsetsToHost(int nimg, hipStream_t s)
    {
        count.toHost(1, s);
        goff.toHost((size_t)nimg + 1, s);
    }
    void pairsToHost(hipStream_t s)
    {
        if (const uint32_t n = *count.h) {
            gidx.toHost(n, s);
            gval.toHost(n, s);
        }
    }
    // image k's candidates (pointers into the host mirrors: valid until the next grow)
    void bind(PlannedImage &p, int k) const
    {
        p.fg = gidx.h + goff.h[k];
        p.fgv = gval.h + goff.h[k];
        p.nfg = goff.h[k + 1] - goff.h[k];
    }
};

// One overflow check of a batch: the kernels counted `needed` entries for `list`.  Rows of the same step grow together;
// locRegrow: counts as a regrow of the localize knob's lists (PipeStats)
struct Fit {
    Growable *list;
    size_t needed;
    const char *message;
    int step;
    bool locRegrow;
};
// The checks of a batch in the order of `rows`, once its counts are on the host and its kernels are done: the lists of the
// first step that does not fit grow (Growable::fit; attempt 0 starts the batch) and the caller redoes the batch -> the
// first row that grew, nullptr when everything fitted
static const Fit *fitLists(const Fit *rows, size_t n, int attempt)
{
    for (size_t k = 0; attempt == 0 && k < n; ++k)
        rows[k].list->newBatch();
    const Fit *grew = nullptr;
    for (size_t k = 0; k < n && (!grew || rows[k].step == grew->step); ++k)
        if (!rows[k].list->fit(rows[k].needed, rows[k].message) && !grew)
            grew = &rows[k];
    return grew;
}

// The counters a getter (abh_pipe_*_stats, abh_pipe_bellows, abh_pipe_timing) hands out are one struct of doubles in the
// getter's slot order -- a count stays exact in a double far beyond any run's -- so each counter is declared, and named,
// once: the struct is copied out as it stands, and two of them add slot by slot
template <class T>
void copySlots(const T &s, double *out)
{
    static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % sizeof(double) == 0, "a struct of doubles");
    std::memcpy(out, &s, sizeof s);
}
template <class T>
void addSlots(T &a, const T &b)
{
    double x[sizeof(T) / sizeof(double)], y[sizeof(T) / sizeof(double)];
    copySlots(a, x);
    copySlots(b, y);
    for (size_t k = 0; k < sizeof(T) / sizeof(double); ++k)
        x[k] += y[k];
    std::memcpy(&a, x, sizeof a);
}

// Counters of one run: every stack group keeps its own, the pipeline merges them.  The groups run side by side, so the
// times and rounds of the stage timers take the maximum; counts, and the kernel ms of the knobs, add up over groups and rounds
struct PipeStats {
    // abh_pipe_timing: host wall time (ms) waiting for stage 1, of stages 2 .. 4 summed over the rounds, of the whole run;
    // of stage 3: launches + kernels + histogram / count D2H, list D2H + thresholds, an unused slot (the key s3_bucket_ms
    // stays in the reports); candidate pairs of the last stage-3 batch; trigger-search jobs (F - 1 per stack when nothing is
    // lazy); stacks on the one-at-a-time path (bellows veto); jobs whose dense rows were evaluated on demand
    struct Timing {
        double stage1Ms = 0, stage2Ms = 0, stage3Ms = 0, stage4Ms = 0, totalMs = 0, s3GpuMs = 0, s3ListMs = 0, s3BucketMs = 0;
        double pairs = 0, jobsLaunched = 0, dropIns = 0, jobsCompleted = 0;
        // (totalMs and the last three are kept by the pipeline across its groups, under launchMu or after the groups ended)
        void add(const Timing &g)
        {
            for (double Timing::*t : {&Timing::stage1Ms, &Timing::stage2Ms, &Timing::stage3Ms, &Timing::stage4Ms,
                                      &Timing::s3GpuMs, &Timing::s3ListMs})
                this->*t = std::max(this->*t, g.*t);
            pairs += g.pairs;
        }
    } timing;
    int rounds = 0; // what abh_pipe_timing returns
    // abh_pipe_bellows, the veto inside the batch: stacks, template-match jobs and launches, residual images, ms of its rounds
    struct Bellows {
        double vetoed = 0, matchJobs = 0, matchLaunches = 0, residualImages = 0, vetoMs = 0;
    } bellows;
    // abh_pipe_blob_stats: candidate pairs, foreground pixels after the Otsu cut, kept pixels (shipped to the host),
    // components, kept components, slots labelled on the global-memory path, ms of the Otsu and of the K4b launches
    struct Blobs {
        double candidates = 0, foreground = 0, kept = 0, components = 0, keptComponents = 0, largeSlots = 0, otsuMs = 0, k4bMs = 0;
    } blobs;
    // abh_pipe_contour_stats: slots traced on the device, slots left to the host route, contours, vertices, ms of K5
    struct Contours {
        double traced = 0, host = 0, contours = 0, vertices = 0, k5Ms = 0;
    } contours;
    // abh_pipe_trigger_stats: stacks searched on the device, stacks on the host route, search launches (kept by the
    // pipeline, like jobsLaunched: a group's are 0), NEED_FRAMES and NEED_FINAL answers, ms of the K6 launches
    struct Trigger {
        double devStacks = 0, hostStacks = 0, launches = 0, needFrames = 0, needFinal = 0, k6Ms = 0;
    } trigger;
    // abh_pipe_localize_stats, summed over the rounds: stacks localised on the device, stacks on the host route by reason
    // (over a limit; a declined slot or an undecodable frame; every genesis contour in the bellows mask; an Otsu mismatch),
    // bubbles and descriptors of the device's tracks, ms of the K7 launches; bytes of the kept-pixel, contour, vertex, record,
    // box and track lists copied to the host (with the contours knob alone, too); batches redone to grow the knob's lists
    struct Localize {
        double device = 0, hostLimit = 0, hostSlot = 0, hostBellows = 0, hostOther = 0, bubbles = 0, descs = 0, k7Ms = 0;
        double listBytes = 0, regrows = 0;
        double hostRoute() const { return hostLimit + hostSlot + hostBellows + hostOther; }
    } loc;

    void reset() { *this = PipeStats(); }
    // a group's counters into the run's
    void merge(const PipeStats &g)
    {
        timing.add(g.timing);
        rounds = std::max(rounds, g.rounds);
        addSlots(bellows, g.bellows);
        addSlots(blobs, g.blobs);
        addSlots(contours, g.contours);
        addSlots(trigger, g.trigger);
        addSlots(loc, g.loc);
    }
};

// One slice of the run with its own stream and scratch: groups run concurrently on host threads, so the
// GPU work of one group overlaps the host state machines of another (no group waits on another).
struct Group {
    int s0 = 0, s1 = 0; // stacks [s0, s1)
    size_t ns = 0, n3 = 0; // their number, and the image slots of a stage-3 batch: NumFramesBubbleTrack + 1 per stack
    Event stage1Done, kernelsDone, blockDone;
    // The trigger search (stages 1 and 2) of the group's stacks: the frame blocks' buffers, their launches (K2), the deferred
    // pieces and the device search (K6).  The launching functions take `run`, the pipeline's own counters (jobsLaunched,
    // jobsCompleted, trigger.launches are kept across the groups): the caller holds the pipeline's launchMu, or no group
    // thread runs yet.  Everything else here belongs to the group's thread.
    struct Search {
        using BlockRef = BatchEventData::BlockRef;
        // what the pipeline's constructor fixes: geometry, the frame offset every camera shares (else 0), whether dense
        // frames' rows are evaluated on demand, and the frame blocks: block k = frames [starts[k], starts[k + 1])
        struct Setup {
            int W = 0, H = 0, F = 0, C = 0, chainStride = 0;
            bool deferPieces = false;
            std::vector<int> starts;
            int nblocks() const { return (int)starts.size() - 1; }
        };
        struct Fetch {
            int first = 0, n = 0;   // stacks [first, first + n) of the block's buffers
            size_t pieceOff = 0;    // its range of the block's piece list
            bool deferred = false;
        };
        // per frame block: job lists and histograms (capacity: every stack of the group once), and the deferred pieces:
        // handed-over row ranges of every launch of the block, per-launch counters, per-job "incomplete" / "wanted" flags
        struct Block {
            int first = 0, len = 0; // frames [first, first + len)
            Mirror<abub_job> jobs;
            Mirror<uint32_t> hist;
            DeviceArray<uint64_t> pieces;
            DeviceArray<uint32_t> pcount; // [64]: one per launch
            Mirror<uint8_t> inc, want;
            size_t pieceCap = 0, pieceUsed = 0;
            int used = 0; // stacks already served in this run (each stack fetches a block at most once: `ns` at the most)
            std::vector<Fetch> fetches;
            // where the stack at position q of launch f lies in the block's buffers (the only place that works it out)
            BlockRef bind(int f, int q) const
            {
                const Fetch &fe = fetches[f];
                BlockRef r;
                r.fetch = f;
                r.job = (size_t)(fe.first + q) * len;
                r.hist = hist.h + r.job * 256;
                r.histDev = hist.d + r.job * 256;
                if (fe.deferred)
                    r.inc = inc.h + r.job, r.incDev = inc.d + r.job;
                return r;
            }
        };
        Setup cfg;
        size_t ns = 0; // stacks of the group: every per-job buffer of a block holds each of them once
        std::vector<Block> blocks;
        // trigger knob: K6 (abub_trigger.hip) on the blocks' device histograms: descriptors of one launch (pinned, copied by
        // the launcher), its results, the stacks it serves in launch order.  One launch at a time: every launch is waited for
        // (stage1Done / blockDone) and collected before the next one is filled in.
        struct Trigger {
            bool inflight = false;
            PinnedArray<abub_trig_stack> st;
            PinnedArray<abub_trig_seg> sg;
            DeviceArray<uint8_t> desc;
            size_t descBytes = 0;
            Mirror<abub_trig_result> res;
            std::vector<int> list;
            Event ev[2]; // before and after the launch
            void firstUse(size_t ns)
            {
                if (ev[1].get())
                    return;
                const size_t nsg = ns * BatchEventData::MAXB;
                st.allocate(ns);
                sg.allocate(nsg);
                descBytes = abub_trigger_search_desc_bytes((int)ns, (int)nsg);
                desc.allocate(descBytes);
                res.allocate(ns);
                ev[0].create(true);
                ev[1].create(true);
            }
        } trig;

        void allocate(const Setup &setup, size_t nstacks)
        {
            cfg = setup;
            ns = nstacks;
            blocks.resize((size_t)cfg.nblocks());
            for (int k = 0; k < cfg.nblocks(); ++k) {
                Block &B = blocks[k];
                B.first = cfg.starts[k];
                B.len = cfg.starts[k + 1] - cfg.starts[k];
                const size_t nj = ns * (size_t)std::max(B.len, 1);
                B.jobs.allocate(nj);
                B.hist.allocate(nj * 256);
                // deferred pieces: at most H / 16 + 8 row ranges per job (chunks are at least 16 rows), 64 launches per block
                B.pieceCap = cfg.deferPieces ? nj * (size_t)(cfg.H / 16 + 8) : 1;
                B.pieces.allocate(B.pieceCap);
                B.pcount.allocate(64);
                B.inc.allocate(nj);
                B.want.allocate(nj);
            }
        }
        // a new run: no block has served a stack, no search is under way
        void beginRun()
        {
            for (Block &B : blocks) {
                B.used = 0;
                B.pieceUsed = 0;
                B.fetches.clear();
            }
            trig.inflight = false;
        }
        // trigger-search job of frame i of stack s (FindTriggerFrame's pairing, see refOffset).  Frames a shorter stack does
        // not have are replaced by its last one on both sides (D = 0: a quiet job that keeps the chain structure the scan
        // relies on).
        abub_job triggerJob(int s, const BatchEventData &d, int i, uint32_t out) const
        {
            const int last = std::max(d.F - 1, 0);
            abub_job j;
            j.cur = (uint32_t)(s * cfg.F + std::min(i, last));
            j.ref = (uint32_t)(s * cfg.F + std::min(std::max(i - d.refOffset, 0), last));
            j.model = (uint32_t)(s % cfg.C);
            j.out = out;
            return j;
        }
        // K2 over block k for the listed stacks, which are bound to the launch: jobs -> device, launch, histograms -> host
        void launchBlock(int k, const std::vector<int> &list, std::vector<StackState> &stacks, const uint8_t *d_frames,
                         const uint8_t *d_sigma6, hipStream_t stream, PipeStats &run)
        {
            Block &B = blocks[k];
            const int W = cfg.W, H = cfg.H, blen = B.len, first = B.used, n = (int)list.size();
            if (blen <= 0 || n == 0)
                return;
            if (first + n > (int)ns)
                throw std::runtime_error("RunPipeline: a frame block was requested twice for one stack");
            const size_t j0 = (size_t)first * blen;
            for (int q = 0; q < n; ++q)
                for (int i = 0; i < blen; ++i)
                    B.jobs.h[j0 + (size_t)q * blen + i] =
                        triggerJob(list[q], stacks[list[q]].data, B.first + i, (uint32_t)((size_t)q * blen + i));
            abub_job *dj = B.jobs.d + j0;
            uint32_t *dh = B.hist.d + j0 * 256;
            const int nj = n * blen;
            B.jobs.toDevice(nj, stream, j0);
            Fetch fe;
            fe.first = first;
            fe.n = n;
            // deferral is decided per launch: the K2 options (abub_k2_set_option "bound") may change after construction
            const bool defer = cfg.deferPieces && abub_k2_deferred_ok(W, H);
            const size_t pcap = defer ? abub_k2_pieces_cap(nj, W, H) : 0;
            if (defer && B.fetches.size() < 64 && B.pieceUsed + pcap <= B.pieceCap) {
                // the scan alone: dense frames' rows go to this launch's range of the block's piece list, their jobs are flagged
                fe.deferred = true;
                fe.pieceOff = B.pieceUsed;
                B.pieceUsed += pcap;
                check(abub_diff_hist_chained_deferred_dev(d_frames, d_sigma6, dj, nj, W, H, dh, blen, cfg.chainStride,
                                                          B.pieces + fe.pieceOff, (uint32_t)pcap, B.pcount + B.fetches.size(),
                                                          B.inc.d + j0, stream),
                      "trigger search K2 (deferred pieces)");
                B.inc.toHost(nj, stream, j0);
            } else {
                // all cameras on the same frame offset: per stack the jobs are a chain (job i refs the cur frame of job i - off)
                // and the scan loads every frame row once for both of its jobs
                check(cfg.chainStride > 0
                          ? abub_diff_hist_chained_dev(d_frames, d_sigma6, dj, nj, W, H, dh, blen, cfg.chainStride, stream)
                          : abub_diff_hist_dev(d_frames, d_sigma6, dj, nj, W, H, dh, nullptr, 0, stream),
                      "trigger search K2");
            }
            B.hist.toHost((size_t)nj * 256, stream, j0 * 256);
            B.fetches.push_back(fe);
            B.used = first + n;
            for (int q = 0; q < n; ++q)
                stacks[list[q]].data.ref[k] = B.bind((int)B.fetches.size() - 1, q);
            run.timing.jobsLaunched += nj;
        }
        // The row machine on launch f of block k: for every asking stack (all served by that launch), the flagged frames from
        // the one it stopped at to the end of the block.  clearOnDevice (trigger knob): they are final on the device too, where
        // K6 reads the flags (the host mirror of the flags is cleared by served())
        void completePieces(int k, int f, const std::vector<int> &askers, const std::vector<StackState> &stacks,
                            const uint8_t *d_frames, const uint8_t *d_sigma6, bool clearOnDevice, hipStream_t stream, PipeStats &run)
        {
            Block &B = blocks[k];
            const Fetch &fe = B.fetches[f];
            const size_t blen = (size_t)B.len, nj = (size_t)fe.n * blen, base = (size_t)fe.first * blen;
            std::memset(B.want.h + base, 0, nj);
            for (int sI : askers) {
                const BatchEventData &d = stacks[sI].data;
                for (size_t j = (size_t)(d.need.frame - B.first); j < blen; ++j)
                    if (d.ref[k].inc[j]) {
                        B.want.h[d.ref[k].job + j] = 1;
                        ++run.timing.jobsCompleted;
                    }
            }
            B.want.toDevice(nj, stream, base);
            check(abub_diff_hist_pieces_dev(d_frames, d_sigma6, B.jobs.d + base, (int)nj, cfg.W, cfg.H, B.hist.d + base * 256,
                                            B.pieces + fe.pieceOff, B.pcount + f, B.want.d + base, stream),
                  "trigger search K2 (pieces)");
            for (int sI : askers) {
                const BatchEventData &d = stacks[sI].data;
                const size_t j0 = (size_t)(d.need.frame - B.first);
                B.hist.toHost((blen - j0) * 256, stream, (d.ref[k].job + j0) * 256);
            }
            if (clearOnDevice) // one launch per fetch
                check(abub_trigger_clear_pending_dev(B.inc.d + base, B.want.d + base, nj, stream), "trigger search flags");
        }
        // after the launches that serve the stack's request have been waited for: its block has arrived, or its frames are final
        void served(BatchEventData &d) const
        {
            BlockRef &r = d.ref[d.need.block];
            const Block &B = blocks[d.need.block];
            if (d.need.pieces)
                std::fill(r.inc + (d.need.frame - B.first), r.inc + B.len, (uint8_t)0);
            r.arrived = true;
            d.clearNeed();
        }
        // One K6 launch for the listed stacks, each from its analyzer's current state (retry: behind the last trigger), on
        // every block launched for it so far; the results come back with the next event the group waits for (collectSearch).
        void launchSearch(const std::vector<int> &list, const std::vector<StackState> &stacks, hipStream_t stream, PipeStats &run)
        {
            Trigger &T = trig;
            if (list.empty())
                return;
            if (T.inflight)
                throw std::runtime_error("RunPipeline: a trigger search was launched before the previous one was collected");
            T.firstUse(ns);
            uint32_t nseg = 0;
            for (size_t q = 0; q < list.size(); ++q) {
                const StackState &st_ = stacks[list[q]];
                abub_trig_stack &d = T.st[q];
                d.seg0 = nseg;
                d.F = st_.data.F;
                d.start = (st_.analyzer ? st_.analyzer->MatTrigFrame : 0) + 1;
                d.tss = st_.data.tss;
                d.first_bad = st_.data.firstBad();
                for (int k = 0; k < cfg.nblocks(); ++k)
                    if (st_.data.ref[k].launched()) {
                        abub_trig_seg &g = T.sg[nseg++];
                        g.hist = st_.data.ref[k].histDev;
                        g.pending = st_.data.ref[k].incDev;
                        g.first = blocks[k].first;
                        g.count = blocks[k].len;
                    }
                d.nseg = nseg - d.seg0;
            }
            HIPOK(hipEventRecord(T.ev[0].get(), stream));
            check(abub_trigger_search_dev(T.st, T.sg, (int)list.size(), (int)nseg, cfg.W, cfg.H, T.desc, T.descBytes, T.res.d,
                                          nullptr, 0, stream),
                  "trigger search K6");
            HIPOK(hipEventRecord(T.ev[1].get(), stream));
            T.res.toHost(list.size(), stream);
            T.list = list;
            T.inflight = true;
            ++run.trigger.launches;
        }
        // after the event behind the launch has been waited for: every served stack gets its answer
        void collectSearch(std::vector<StackState> &stacks, PipeStats &groupStats)
        {
            Trigger &T = trig;
            if (!T.inflight)
                return;
            for (size_t q = 0; q < T.list.size(); ++q) {
                StackState &st_ = stacks[T.list[q]];
                st_.trigRes = T.res.h[q];
                st_.trigReady = true;
            }
            groupStats.trigger.k6Ms += T.ev[1].msSince(T.ev[0]);
            T.inflight = false;
        }
    } search;
    Mirror<abub_job> jobs3;
    Mirror<uint32_t> hist3;
    DeviceArray<uint8_t> img;
    Mirror<int32_t> thr;
    CandidateList list;
    // The opt-in knobs of stage 3: each stage allocates nothing before its first use (which makes its last event last: that
    // event says the stage is there), and has one function per phase of batchImages, which calls them in this order:
    // launch, countsToHost, addTimings, (the overflow checks,) listsToHost, bind
    // blobs knob: the device also computes the Otsu thresholds and labels each image's foreground (K4b, abub_blobs.hip)
    // behind the grouping, and only the pixels of the components the localizer can use come back (the kept list is in `list`)
    struct Blobs {
        bool shipKept = true; // of the batch: its kept pixels travel (listsToHost)
        Mirror<int32_t> otsu, minbox;
        Mirror<uint32_t> koff, kstats; // kstats: K4b's counters
        DeviceArray<uint32_t> ncomp, nkc, coff;
        Event ev[3]; // before Otsu, between, after K4b
        void firstUse(size_t n3, CandidateList &L, int W, int H)
        {
            if (ev[2].get())
                return;
            otsu.allocate(n3);
            minbox.allocate(n3);
            koff.allocate(n3 + 1);
            ncomp.allocate(n3);
            nkc.allocate(n3);
            coff.allocate(n3 + 1);
            kstats.allocate(4);
            L.keptImages = (int)n3;
            L.keptW = W;
            L.keptH = H;
            for (Event &e : ev)
                e.create(true);
        }
        void launch(const CandidateList &L, const std::vector<PlannedImage *> &bySlot, const uint32_t *d_hist, const int32_t *d_thr,
                    int W, int H, hipStream_t stream)
        {
            const int nimg = (int)bySlot.size();
            for (int k = 0; k < nimg; ++k)
                minbox.h[k] = bySlot[k]->minBox;
            minbox.toDevice(nimg, stream);
            HIPOK(hipEventRecord(ev[0].get(), stream));
            check(abub_binarize_thr_dev(d_hist, d_thr, nimg, W, H, otsu.d, stream), "stage3 Otsu");
            HIPOK(hipEventRecord(ev[1].get(), stream));
            check(abub_label_blobs_dev(L.goff.d, L.gidx.d, L.gval.d, L.cap(), nimg, W, H, otsu.d, minbox.d, koff.d, L.kidx.d,
                                       L.cap(), ncomp, nkc, coff, nullptr, 0, kstats.d, L.keptScratch, L.keptScratchBytes, stream),
                  "stage3 K4b");
            HIPOK(hipEventRecord(ev[2].get(), stream));
        }
        void countsToHost(int nimg, hipStream_t back)
        {
            otsu.toHost(nimg, back);
            koff.toHost((size_t)nimg + 1, back);
            kstats.toHost(4, back);
        }
        void addTimings(PipeStats &stats)
        {
            stats.blobs.otsuMs += ev[1].msSince(ev[0]);
            stats.blobs.k4bMs += ev[2].msSince(ev[1]);
        }
        // `traced`: K5's counters (nullptr: contours knob off): then the kept pixels travel only when a slot was declined
        void listsToHost(hipStream_t back, const CandidateList &L, int nimg, const uint32_t *traced, PipeStats &stats)
        {
            const uint32_t nkept = koff.h[nimg];
            if (nkept > L.cap())
                throw std::runtime_error("RunPipeline: kept list larger than the candidate list");
            shipKept = !traced || traced[1] != 0;
            if (nkept && shipKept) {
                L.kidx.toHost(nkept, back);
                stats.loc.listBytes += traced ? 4.0 * nkept : 0;
            }
            stats.blobs.candidates += *L.count.h;
            stats.blobs.foreground += kstats.h[1];
            stats.blobs.kept += nkept;
            stats.blobs.components += kstats.h[2];
            stats.blobs.keptComponents += kstats.h[3];
            stats.blobs.largeSlots += kstats.h[0];
        }
        // image k's kept pixels, after the host's threshold p.thr (pointers into the host mirrors, like CandidateList::bind)
        void bind(PlannedImage &p, int k, const CandidateList &L) const
        {
            p.kept = L.kidx.h + koff.h[k];
            p.nkept = koff.h[k + 1] - koff.h[k];
            p.otsuMismatch = otsu.h[k] != p.thr;
            p.keptShipped = shipKept;
        }
    } blobs;
    // contours knob: K5 (abub_contours.hip) then traces each image's contours from K4b's kept list and the vertices come
    // back.  The scratch follows the candidate list's capacity, the contour and vertex lists have capacities of their own
    struct Contours {
        bool shipVerts = true; // of the batch: its vertices travel (listsToHost)
        size_t inCap = 0;      // the candidate capacity the scratch was made for
        Mirror<uint32_t> status, ncont, coff, poff, cstats;
        GrowList<uint32_t> cnpts{64}, pts{64}; // vertices per contour; vertices
        DeviceArray<uint8_t> scratch;
        size_t scratchBytes = 0;
        Event ev[2]; // before and after K5
        // the per-image arrays once, the scratch for the candidate list's capacity, which may just have grown (`back` has waited
        // for the kernels that used the old one), the two lists at a quarter of it to start with (few pixels are vertices)
        void fit(size_t n3, const CandidateList &L, int W, int H)
        {
            if (!ev[1].get()) {
                status.allocate(n3);
                ncont.allocate(n3);
                coff.allocate(n3 + 1);
                poff.allocate(n3 + 1);
                cstats.allocate(4);
                for (Event &e : ev)
                    e.create(true);
            }
            if (inCap != L.cap()) {
                scratchBytes = abub_trace_contours_scratch_bytes((int)n3, L.cap());
                if (scratchBytes == 0 || W > 65535 || H > 65535)
                    throw std::runtime_error("RunPipeline: frame size not supported by the contour tracing");
                scratch.allocate(scratchBytes);
                inCap = L.cap();
            }
            if (cnpts.cap() == 0) {
                cnpts.reserve(L.cap() / 4 + 64);
                pts.reserve(L.cap() / 4 + 64);
            }
        }
        void launch(size_t n3, const CandidateList &L, const uint32_t *d_koff, int nimg, int W, int H, hipStream_t stream)
        {
            fit(n3, L, W, H);
            HIPOK(hipEventRecord(ev[0].get(), stream));
            check(abub_trace_contours_dev(d_koff, L.kidx.d, L.cap(), nimg, W, H, status.d, ncont.d, coff.d, cnpts.d,
                                          (uint32_t)cnpts.cap(), poff.d, pts.d, (uint32_t)pts.cap(), cstats.d, scratch,
                                          scratchBytes, stream),
                  "stage3 K5");
            HIPOK(hipEventRecord(ev[1].get(), stream));
        }
        void countsToHost(int nimg, hipStream_t back)
        {
            status.toHost(nimg, back);
            coff.toHost((size_t)nimg + 1, back);
            poff.toHost((size_t)nimg + 1, back);
            cstats.toHost(4, back);
        }
        void addTimings(PipeStats &stats) { stats.contours.k5Ms += ev[1].msSince(ev[0]); }
        // `ship`: with the localize knob the vertices travel only when some stack was declined and takes the host route
        void listsToHost(hipStream_t back, int nimg, bool ship, PipeStats &stats)
        {
            shipVerts = ship;
            if (shipVerts) {
                if (const uint32_t nc = coff.h[nimg])
                    cnpts.toHost(nc, back);
                if (const uint32_t nv = poff.h[nimg])
                    pts.toHost(nv, back);
                stats.loc.listBytes += 4.0 * coff.h[nimg] + 4.0 * poff.h[nimg];
            }
            stats.contours.traced += cstats.h[0];
            stats.contours.host += cstats.h[1];
            stats.contours.contours += cstats.h[2];
            stats.contours.vertices += cstats.h[3];
        }
        // image k's contours, unless the kernel declined the slot
        void bind(PlannedImage &p, int k) const
        {
            p.traced = status.h[k] == 0;
            p.vertsShipped = shipVerts;
            if (p.traced) {
                p.cnp = cnpts.h + coff.h[k];
                p.cpts = pts.h + poff.h[k];
                p.ncont = coff.h[k + 1] - coff.h[k];
            }
        }
    } contours;
    // localize knob: K7 (abub_localize.hip) then describes every contour (the records) and runs the localizer's decisions per
    // stack (descriptors: pinned, copied by the launcher); the per-stack results, boxes and tracks come back
    struct Localize {
        GrowList<abub_contour_desc> desc{64};
        GrowList<int32_t> rects{64, 4}; // x, y, w, h
        GrowList<uint32_t> tracks{64};
        PinnedArray<abub_loc_stack> st;
        DeviceArray<uint8_t> scratch;
        size_t scratchBytes = 0;
        Mirror<abub_loc_result> res;
        Mirror<uint32_t> totals; // boxes and track entries of the batch
        Event ev[2]; // before K7a and after K7b
        // the per-stack arrays; the three lists at a modest size to start with, or exactly `locCap` entries each (to overflow)
        void firstUse(size_t ns, int C, int locCap)
        {
            if (ev[1].get())
                return;
            st.allocate(ns);
            scratchBytes = abub_localize_scratch_bytes((int)ns, C);
            scratch.allocate(scratchBytes);
            res.allocate(ns);
            totals.allocate(2);
            locCap > 0 ? desc.seed((size_t)locCap) : desc.reserve(64 * ns);
            locCap > 0 ? rects.seed((size_t)locCap) : rects.reserve(8 * ns);
            locCap > 0 ? tracks.seed((size_t)locCap) : tracks.reserve(16 * ns);
            for (Event &e : ev)
                e.create(true);
        }
        // the descriptors of the stacks of `loc` from their planned images, then K7a over the contours K5 traced and K7b
        void launch(size_t ns, int C, int locCap, const abub_loc_mask *masks, const Contours &K,
                    const std::vector<StackState> &stacks, const std::vector<int> &loc, int nimg, hipStream_t stream)
        {
            firstUse(ns, C, locCap);
            const int nloc = (int)loc.size();
            for (int k = 0; k < nloc; ++k) {
                const StackState &ss = stacks[loc[k]];
                abub_loc_stack &d = st[k];
                d = abub_loc_stack{};
                d.cam = loc[k] % C;
                d.bad = !ss.data.frameOk(0);
                int nt = 0;
                for (const PlannedImage &p : ss.data.planned) {
                    if (!ss.data.frameOk(p.i) || (p.kind == 0 && !ss.data.frameOk(p.ref)))
                        d.bad = 1;
                    if (p.kind == 0)
                        d.genesis = p.slot;
                    else if (nt < ABUB_LOC_MAXTRACK)
                        d.track[nt++] = p.slot; // (planned in frame order)
                    else
                        throw std::runtime_error("RunPipeline: more tracking frames planned than ABUB_LOC_MAXTRACK");
                }
                d.ntrack = nt;
            }
            HIPOK(hipEventRecord(ev[0].get(), stream));
            check(abub_describe_contours_dev(K.status.d, K.coff.d, K.cnpts.d, (uint32_t)K.cnpts.cap(), K.poff.d, K.pts.d,
                                             (uint32_t)K.pts.cap(), nimg, desc.d, (uint32_t)desc.cap(), stream),
                  "stage3 K7a");
            check(abub_localize_stacks_dev(st, nloc, masks, C, K.status.d, K.coff.d, nimg, desc.d,
                                           (uint32_t)std::min(desc.cap(), K.cnpts.cap()), scratch, scratchBytes, res.d, rects.d,
                                           (uint32_t)rects.cap(), tracks.d, (uint32_t)tracks.cap(), totals.d, stream),
                  "stage3 K7b");
            HIPOK(hipEventRecord(ev[1].get(), stream));
        }
        void countsToHost(int nloc, hipStream_t back)
        {
            res.toHost((size_t)nloc, back);
            totals.toHost(2, back);
        }
        void addTimings(PipeStats &stats) { stats.loc.k7Ms += ev[1].msSince(ev[0]); }
        // some stack of the batch was declined and takes the host route
        bool declined(int nloc) const
        {
            return std::any_of(res.h + 0, res.h + nloc, [](const abub_loc_result &r) { return r.status != ABUB_LOC_DONE; });
        }
        // the records of the batch's `nc` contours, its boxes and its tracks
        void listsToHost(hipStream_t back, uint32_t nc, int nloc, PipeStats &stats)
        {
            if (nc)
                desc.toHost(nc, back);
            if (totals.h[0])
                rects.toHost(4 * (size_t)totals.h[0], back);
            if (totals.h[1])
                tracks.toHost(totals.h[1], back);
            stats.loc.listBytes += (double)sizeof(abub_contour_desc) * nc + 16.0 * totals.h[0] + 4.0 * totals.h[1] +
                                   (double)sizeof(abub_loc_result) * nloc;
        }
        // stack k: one the kernels finished, and whose thresholds the host confirms, skips stage 4's arithmetic; the others
        // are counted by the reason they take the host route for
        void bind(BatchEventData &d, int k, PipeStats &stats) const
        {
            const abub_loc_result &r = res.h[k];
            d.locReady = r.status == ABUB_LOC_DONE &&
                         std::none_of(d.planned.begin(), d.planned.end(), [](const PlannedImage &p) { return p.otsuMismatch; });
            if (d.locReady) {
                d.locTrig = d.planned[0].i;
                d.locRes = r;
                d.locRects = rects.h;
                d.locTracks = tracks.h;
                d.locDesc = desc.h;
                ++stats.loc.device;
                stats.loc.bubbles += r.nbubbles;
                stats.loc.descs += r.ntrack - r.nbubbles;
            } else if (r.status == ABUB_LOC_LIMIT)
                ++stats.loc.hostLimit;
            else if (r.status == ABUB_LOC_SLOT || r.status == ABUB_LOC_BAD_FRAME)
                ++stats.loc.hostSlot;
            else if (r.status == ABUB_LOC_BELLOWS)
                ++stats.loc.hostBellows;
            else
                ++stats.loc.hostOther;
        }
    } loc;
    // bellows veto round (vetoRound): its own buffers, allocated on first use, grown on demand
    struct Veto {
        int capJobs = 0;           // match jobs the buffers hold
        size_t scratchBytes = 0;   // abub_match_best_batch_dev scratch
        Mirror<uint32_t> fidx;
        Mirror<float> xy;
        DeviceArray<uint8_t> scratch;
        int capImg = 0;            // residual images
        Mirror<uint8_t> rend;      // [2n][P]: trigger copy, pre-trigger copy
        DeviceArray<uint8_t> syn, img; // [n][P]: ROI ProcessFrame of the renderings, the residual
        DeviceArray<uint32_t> rhist;   // [n][256] (ROI ProcessFrame histograms, unused)
        Mirror<uint32_t> hist;
        Mirror<abub_job> jobs;
        Mirror<int32_t> thr;
        CandidateList list;
        std::vector<std::pair<cv::Mat, DeviceArray<uint8_t>>> templates; // device copies of the bellows templates (deviceTemplate)
    } veto;
    int nthreads = 1;
    PipeStats stats; // of the group's part of the last run
    std::string error;
    // declared last, so destroyed first: the holder finishes the stream's work before the buffers above are freed
    Stream stream;
};

// an integer from the environment (atoi of the variable's text), `unset` when the variable is not there
static int envInt(const char *name, int unset)
{
    const char *e = getenv(name);
    return e ? atoi(e) : unset;
}

// An opt-in knob of a pipeline object (0 or 1): abh_pipe_set_option's name for it, the environment variable a new pipeline
// takes it from (unset: 0), the member that holds it
class RunPipeline;
struct Knob {
    const char *name, *env;
    int RunPipeline::*value;
};

class RunPipeline {
public:
    static const Knob knobs[4];
    int device, W, H, F, E, C, S, nthreads, ngroups;
    size_t P;
    std::vector<int> tss;
    std::string maskDir;
    // Declaration order: the streams (stage1Stream, copyStream, each group's last member) come after the buffers their
    // work uses, so they are destroyed first, and a Stream finishes its work before it goes (see ~RunPipeline)
    DeviceArray<uint8_t> ownFrames;     // frame slab owned by the pipeline (streamed mode only)
    std::vector<Group> groups;
    std::unique_ptr<WorkerPool> pool;
    Group::Search::Setup search;        // the trigger search's constants (see the constructor): every group has a copy
    bool bellowsDropIn = false;         // ABUB_PIPE_BELLOWS=dropin: every bellows veto takes the one-at-a-time path (A/B)
    PipeStats stats;                    // the last run's, merged over the groups
    Stream stage1Stream;                // all trigger-search launches, in group order (see run())
    bool ordered = true;                // a group's later kernels queue on stage1Stream too (see kernelStream())
    int pairCap = 0;                    // ABUB_PIPE_PAIRCAP (0: unset)
    int locCap = 0;                     // ABUB_PIPE_LOCCAP (0: unset)
    int blobs = 0, contours = 0, trigger = 0, localizeDev = 0; // the knobs (see `knobs` and abh_pipe_set_option)
    std::mutex maskMu;                  // the cameras' masks on the device, uploaded once per pipeline (deviceMasks)
    bool masksReady = false;
    std::vector<DeviceArray<uint8_t>> maskBuf;
    std::vector<abub_loc_mask> locMasks;
    bool trigOn = false;                // `trigger` as read at the start of the current run
    int trigMaxF = 0;                   // abub_trigger_search_limits: a longer stack keeps the host search
    std::mutex launchMu;
    std::vector<StackState> stacks;
    std::vector<std::unique_ptr<Trainer>> trainers;
    MemParser parser;
    // optional (runs ingested from a Parser): real ids / names / decode flags per stack; a stack may be shorter than F
    std::vector<StackMeta> meta;
    MemParser metaParser;
    const uint8_t *d_sigmaRaw = nullptr; // optional: sigma (not 6*sigma) for stacks that need the drop-in path
    // streamed mode (runFromHost): the uploads, one event per group, and whether run() waits for them
    Stream copyStream;
    std::vector<Event> copied;
    bool waitCopies = false;

    void setStackMeta(std::vector<StackMeta> &&m)
    {
        if ((int)m.size() != S)
            throw std::runtime_error("RunPipeline::setStackMeta: one entry per stack expected");
        meta = std::move(m);
        metaParser = MemParser();
        for (int s = 0; s < S; ++s) {
            if ((int)meta[s].names.size() > F || meta[s].ok.size() != meta[s].names.size())
                throw std::runtime_error("RunPipeline::setStackMeta: stack longer than the pipeline's frame count");
            metaParser.AddNamedFrames(meta[s].eventID, s % C, meta[s].names);
        }
    }
    // event k's cameras of the last run staged into `out` and written: the analyzers are gone, so the track records are
    // rebuilt from the results (and freed once the block is written)
    void writeEvent(int k, int eventNumber, OutputWriter &out)
    {
        StagedBubbles staged;
        for (int c = 0; c < C; ++c) {
            const StackState &ss = stacks[(size_t)k * C + c];
            if (!ss.error.empty())
                std::cout << ss.error << '\n'; // (AnyCamAnalysis prints the exception text, then stages -6)
            staged.stage(out, ss, c, eventNumber);
        }
        out.writeCameraOutput();
    }
    int stackFrames(int s) const { return meta.empty() ? F : (int)meta[s].names.size(); }
    // trigger knob: is stack s searched on the device in this run (decided before the first search, from the kernel's static
    // limits; the host search stays for the others), and the stacks of a list that are
    bool devRoute(int s) const { return trigOn && stackFrames(s) <= trigMaxF && P <= (size_t)ABUB_TRIG_MAX_PIXELS; }
    std::vector<int> devRoute(std::vector<int> list) const
    {
        list.erase(std::remove_if(list.begin(), list.end(), [this](int s) { return !devRoute(s); }), list.end());
        return list;
    }
    // Where a group's kernels behind stage 1 go (their results come back on the group's own stream).  Ordered mode (default):
    // every group's kernels queue on the one trigger-search stream, so the GPU sees K2(g0) K2(g1) .. S3(g0) S3(g1) .. strictly
    // one kernel at a time -- chip-filling kernels launched on different streams only slow each other down -- while the host
    // stages of group g run under the kernels of group g+1.
    hipStream_t kernelStream(Group &G) { return ordered ? stage1Stream.get() : G.stream.get(); }

    RunPipeline(int device_, int W_, int H_, int F_, int E_, int C_, const int *tss_, int nthreads_, const char *maskdir)
        : device(device_), W(W_), H(H_), F(F_), E(E_), C(C_), S(E_ * C_), nthreads(nthreads_), P((size_t)W_ * H_),
          tss(tss_, tss_ + C_), maskDir(maskdir ? maskdir : "")
    {
        if (W <= 0 || H <= 0 || F <= 0 || E <= 0 || C <= 0)
            throw std::runtime_error("RunPipeline: bad geometry");
        HIPOK(hipSetDevice(device));
        ngroups = envInt("ABUB_PIPE_GROUPS", 1); // >1 overlaps host stages of one group with the GPU work of the next
        const char *ebw = getenv("ABUB_PIPE_BELLOWS");
        bellowsDropIn = ebw && std::string(ebw) == "dropin";
        ordered = envInt("ABUB_PIPE_ORDERED", 1) != 0;
        for (const Knob &k : knobs)
            this->*k.value = envInt(k.env, 0) != 0;
        int trigMaxSegs = 0;
        check(abub_trigger_search_limits(&trigMaxF, &trigMaxSegs), "abub_trigger_search_limits");
        if (trigMaxSegs < BatchEventData::MAXB)
            trigMaxF = 0; // (cannot happen: the kernel's segment limit is MAXB) -- every stack keeps the host search
        int prLow = 0, prHigh = 0; // (numerically lower = higher priority)
        HIPOK(hipDeviceGetStreamPriorityRange(&prLow, &prHigh));
        stage1Stream.create(prLow);
        if (ngroups < 1)
            ngroups = 1;
        if (ngroups > S)
            ngroups = S;
        const int K = NumFramesBubbleTrack + 1;
        search.W = W, search.H = H, search.F = F, search.C = C;
        search.chainStride = chainStrideOf(tss.data(), C);
        groups.resize(ngroups);
        pool.reset(new WorkerPool(std::max(0, nthreads - ngroups))); // the group driver threads take part too
        // Frame blocks of the trigger search.  The reference walks the frames in order and stops at the trigger
        // (AnalyzerUnit.cpp:191, break at :307); it never differences the frames behind it unless the localizer finds no
        // bubble and the search goes on (AutoBubStart3.cpp:87-110).  So the histograms are produced block by block: block 0
        // for every stack up front, later blocks only for the stacks whose search reaches them.  ABUB_PIPE_LAZY=0: one
        // block (every frame of every stack up front, what round 2 did).
        {
            const bool lazy = envInt("ABUB_PIPE_LAZY", 1) != 0;
            // first block: up to the frame the cameras' own trigger puts the bubble at (the middle of the stack) plus the
            // two look-ahead frames and a margin; then blocks of about a fifth of the stack (a value > 0 overrides either)
            const int e0 = envInt("ABUB_PIPE_BLOCK0", 0), e1 = envInt("ABUB_PIPE_BLOCK", 0);
            int first = e0 > 0 ? e0 : F / 2 + 4, step = e1 > 0 ? e1 : std::max(4, F / 5);
            std::vector<int> &blocks = search.starts;
            blocks.push_back(1);
            if (lazy && F > 8)
                for (int b = std::min(first + 1, F); b < F && (int)blocks.size() < BatchEventData::MAXB; b += step)
                    blocks.push_back(b);
            blocks.push_back(std::max(F, 1)); // block k = frames [blocks[k], blocks[k + 1])
            // Deferred pieces: inside a block the bound scan still covers every frame, but the row machine runs only on the
            // dense frames a search actually reaches (ABUB_PIPE_DEFER=0: at once, for every frame of the block).
            search.deferPieces = envInt("ABUB_PIPE_DEFER", 1) != 0 && search.chainStride > 0 && abub_fast_path(W) != 0;
        }
        // initial capacity of the candidate lists (they grow on demand): ABUB_PIPE_PAIRCAP sets the veto's too
        pairCap = envInt("ABUB_PIPE_PAIRCAP", 0);
        // ... and of the record, box and track lists of the localize knob: ABUB_PIPE_LOCCAP entries each
        locCap = envInt("ABUB_PIPE_LOCCAP", 0);
        for (int g = 0; g < ngroups; ++g) {
            Group &G = groups[g];
            G.s0 = (int)((long long)S * g / ngroups);
            G.s1 = (int)((long long)S * (g + 1) / ngroups);
            const size_t ns = G.ns = (size_t)(G.s1 - G.s0), n3 = G.n3 = ns * K;
            G.nthreads = std::max(1, nthreads / ngroups);
            // the short localisation launches of a finished group must not queue behind the next group's
            // chip-filling trigger search
            G.stream.create(prHigh);
            G.stage1Done.create(false);
            G.kernelsDone.create(false);
            G.blockDone.create(false);
            G.search.allocate(search, ns);
            G.jobs3.allocate(n3);
            G.hist3.allocate(n3 * 256);
            G.img.allocate(abub_fast_path(W) ? 256 : n3 * P); // only the unfused fallback stores images
            G.thr.allocate(n3);
            G.list.allocate(n3);
            G.list.gidx.seed(pairCap > 0 ? (uint32_t)pairCap : (8u << 20) / ngroups);
        }
        // frame names only: the images live in HBM
        for (int c = 0; c < C; ++c) {
            trainers.emplace_back(new Trainer(c, {}, "", "cam%d_image%u.png", "", parser.clone(), false));
            trainers.back()->TrainingSetSize = tss[c];
            trainers.back()->ModelId = 0;
        }
        std::vector<cv::Mat> none((size_t)F);
        for (int e = 0; e < E; ++e)
            for (int c = 0; c < C; ++c)
                parser.AddFrames(std::to_string(e), c, none, 10000); // 5-digit numbers: lexicographic == numeric
    }

    // hipSetDevice first, then each stream that owns library scratch gives it back; the members go after the body, the
    // streams before the buffers their work uses (declaration order)
    ~RunPipeline()
    {
        (void)hipSetDevice(device);
        for (Group &G : groups)
            (void)abub_scratch_release(G.stream.get());
        (void)abub_scratch_release(stage1Stream.get()); // the trigger search's work list lives in library scratch
    }

    // Streamed mode (BASELINE configs[4]): the run sits in HOST memory (ideally pinned).  Stack groups are
    // uploaded in order on a copy stream; the trigger search of group g waits only for its own upload, so it
    // overlaps the transfer of group g+1 (double buffering in time; the slab itself stays resident for the
    // localisation stages).
    void runFromHost(const uint8_t *h_frames, const uint8_t *d_mu, const uint8_t *d_sigma6)
    {
        HIPOK(hipSetDevice(device));
        if (!ownFrames) {
            ownFrames.allocate((size_t)S * F * P);
            copied.resize(ngroups);
            for (Event &e : copied)
                e.create(false);
        }
        for (int g = 0; g < ngroups; ++g) {
            const Group &G = groups[g];
            const size_t off = (size_t)G.s0 * F * P, n = (size_t)(G.s1 - G.s0) * F * P;
            HIPOK(hipMemcpyAsync(ownFrames + off, h_frames + off, n, hipMemcpyHostToDevice, copyStream.get()));
            HIPOK(hipEventRecord(copied[g].get(), copyStream.get()));
        }
        waitCopies = true;
        run(ownFrames, d_mu, d_sigma6, nullptr);
        waitCopies = false;
    }

    // `callerStream`: work already queued there (e.g. the upload of the frames) is waited for first
    void run(const uint8_t *d_frames, const uint8_t *d_mu, const uint8_t *d_sigma6, hipStream_t callerStream)
    {
        HIPOK(hipSetDevice(device));
        if (!waitCopies)
            HIPOK(hipStreamSynchronize(callerStream));
        g_quietAnalyzers = true;
        double t0 = nowMs();
        stacks.clear();
        stacks.resize(S);
        trigOn = trigger != 0; // read once per run
        // what the providers of the fresh stacks serve from (the analyzers are built by the groups, while stage 1 runs)
        for (int s = 0; s < S; ++s) {
            BatchEventData &d = stacks[s].data;
            d.W = W;
            d.H = H;
            d.F = stackFrames(s);
            d.ok = meta.empty() ? nullptr : meta[s].ok.data();
            d.tss = tss[s % C];
            d.refOffset = refOffset(d.tss);
            d.bellowsDropIn = bellowsDropIn;
            d.nblocks = search.nblocks();
            std::copy(search.starts.begin(), search.starts.end(), d.bstart);
        }
        // Stage 1 of every group goes to ONE stream in group order: the trigger search of group g+1 runs
        // on the GPU while the host threads of group g are in their state machines (two kernels launched on
        // different streams would simply share the chip and finish together, leaving nothing to overlap).
        stats.reset();
        for (size_t gi = 0; gi < groups.size(); ++gi) {
            Group &G = groups[gi];
            if (waitCopies)
                HIPOK(hipStreamWaitEvent(stage1Stream.get(), copied[gi].get(), 0));
            G.search.beginRun();
            std::vector<int> all;
            for (int sI = G.s0; sI < G.s1; ++sI)
                all.push_back(sI);
            // block 0: every stack, in group order (nothing to launch for one-frame stacks); trigger knob: the first search
            // of every stack right behind the K2 that produces its input: the decisions arrive with stage1Done
            G.search.launchBlock(0, all, stacks, d_frames, d_sigma6, stage1Stream.get(), stats);
            G.search.launchSearch(devRoute(all), stacks, stage1Stream.get(), stats);
            HIPOK(hipEventRecord(G.stage1Done.get(), stage1Stream.get()));
        }
        std::vector<std::thread> th;
        for (int g = 1; g < ngroups; ++g)
            th.emplace_back([&, g]() { runGroupNoThrow(groups[g], d_frames, d_mu, d_sigma6); });
        runGroupNoThrow(groups[0], d_frames, d_mu, d_sigma6);
        for (auto &t : th)
            t.join();
        // stacks the batched providers could not serve (bellows veto): one at a time through the drop-in path
        for (int s = 0; s < S; ++s)
            if (stacks[s].dropIn) {
                ++stats.timing.dropIns;
                runDropIn(s, d_frames, d_mu);
            }
        for (Group &G : groups) {
            if (!G.error.empty())
                throw std::runtime_error(G.error);
            stats.merge(G.stats);
        }
        g_trigTotals[0] += (long long)stats.trigger.devStacks;
        g_trigTotals[1] += (long long)stats.trigger.hostStacks;
        g_locTotals[0] += (long long)stats.loc.device;
        g_locTotals[1] += (long long)stats.loc.hostRoute();
        stats.timing.totalMs = nowMs() - t0;
    }

private:
    // AnyCamAnalysis of one stack with host copies of its frames and model (the rare bellows-veto case)
    void runDropIn(int s, const uint8_t *d_frames, const uint8_t *d_mu)
    {
        StackState &st_ = stacks[s];
        st_.bubbles.clear();
        if (!d_sigmaRaw) {
            st_.staged = -6;
            st_.error = "bellows veto needs the drop-in path, but no sigma image was given to the pipeline";
            return;
        }
        const int e = s / C, c = s % C;
        try {
            const int Fs = stackFrames(s);
            std::vector<cv::Mat> frames((size_t)Fs);
            for (int i = 0; i < Fs; ++i) {
                if (!meta.empty() && !meta[s].ok[i])
                    continue; // undecodable on disk: stays an empty Mat (GetImage == -1)
                frames[i].create(H, W, CV_8U);
                HIPOK(hipMemcpy(frames[i].data, d_frames + ((size_t)s * F + i) * P, P, hipMemcpyDeviceToHost));
            }
            MemParser mp;
            const std::string evName = meta.empty() ? std::to_string(e) : meta[s].eventID;
            if (meta.empty())
                mp.AddFrames(evName, c, frames, 10000);
            else
                mp.AddNamedFrames(evName, c, meta[s].names, &frames);
            Trainer t(c, {}, "", "cam%d_image%u.png", "", mp.clone(), false);
            t.TrainedAvgImage.create(H, W, CV_8U);
            t.TrainedSigmaImage.create(H, W, CV_8U);
            HIPOK(hipMemcpy(t.TrainedAvgImage.data, d_mu + (size_t)c * P, P, hipMemcpyDeviceToHost));
            HIPOK(hipMemcpy(t.TrainedSigmaImage.data, d_sigmaRaw + (size_t)c * P, P, hipMemcpyDeviceToHost));
            t.TrainingSetSize = tss[c];
            t.ModelId = 0; // always (re)uploaded
            Trainer *tp = &t;
            L3Localizer A(evName, "", c, true, &tp, maskDir, mp.clone());
            size_t rectsBegin = 0;
            st_.staged = analyzeUntilBubble(&A, true, "", st_.error, &rectsBegin);
            if (st_.staged != -6) // (after an exception the stack keeps the state its batched attempt ended with)
                st_.capture(A, rectsBegin);
        } catch (std::exception &ex) {
            st_.error = ex.what();
            st_.staged = -6;
        }
        DeviceContext::releaseThread();
    }

    void runGroupNoThrow(Group &G, const uint8_t *d_frames, const uint8_t *d_mu, const uint8_t *d_sigma6)
    {
        G.error.clear();
        try {
            (void)hipSetDevice(device);
            runGroup(G, d_frames, d_mu, d_sigma6);
        } catch (std::exception &e) {
            G.error = e.what();
        }
    }

    void runGroup(Group &G, const uint8_t *d_frames, const uint8_t *d_mu, const uint8_t *d_sigma6)
    {
        G.stats.reset();
        const int ns = G.s1 - G.s0;
        double t0 = nowMs();
        // ---- stage 1 (already queued by run()) -----------------------------------------------------
        // analyzers are (re)built while the GPU works
        pool->parallelFor(ns, [&](int k) {
            const int s = G.s0 + k;
            StackState &st_ = stacks[s];
            const int e = s / C, c = s % C;
            Trainer *t = trainers[c].get();
            st_.analyzer.reset(new L3Localizer(meta.empty() ? std::to_string(e) : meta[s].eventID, "", c, true, &t, maskDir,
                                               (meta.empty() ? parser : metaParser).clone()));
            st_.analyzer->AttachEventData(&st_.data);
            st_.rectsBegin = 0;
        });
        HIPOK(hipEventSynchronize(G.stage1Done.get()));
        G.stats.timing.stage1Ms = nowMs() - t0;

        // block 0, and with the trigger knob the first answers, came with stage1Done
        std::vector<int> pending(ns);
        for (int k = 0; k < ns; ++k) {
            pending[k] = G.s0 + k;
            BatchEventData::BlockRef &r = stacks[pending[k]].data.ref[0];
            r.arrived = r.launched();
        }
        G.search.collectSearch(stacks, G.stats);
        G.stats.trigger.devStacks = (double)devRoute(pending).size();
        G.stats.trigger.hostStacks = trigOn ? ns - G.stats.trigger.devStacks : 0;
        while (!pending.empty()) {
            ++G.stats.rounds;
            // ---- stage 2: trigger search + plan ------------------------------------------------
            // A search that runs into a frame block which has not been evaluated for its stack stops there
            // (NeedMoreFrames); those blocks are evaluated -- one launch per block index -- and the searches run again.
            double t2 = nowMs();
            std::vector<int> todo(pending);
            while (!todo.empty()) {
                // trigger knob: the stacks without an answer from the event last waited for (retry rounds: the search goes
                // on behind a trigger that gave no bubble) get a launch of their own
                std::vector<int> ask;
                for (int sI : devRoute(todo))
                    if (!stacks[sI].trigReady)
                        ask.push_back(sI);
                if (!ask.empty())
                    fetchBlocks(G, {}, ask, d_frames, d_sigma6);
                pool->parallelFor((int)todo.size(), [&](int k) { triggerAndPlan(stacks[todo[k]]); });
                std::vector<int> need;
                for (int sI : todo) {
                    const BatchEventData &d = stacks[sI].data;
                    if (!d.asked())
                        continue;
                    need.push_back(sI);
                    if (devRoute(sI))
                        ++(d.need.pieces ? G.stats.trigger.needFinal : G.stats.trigger.needFrames);
                }
                if (need.empty())
                    break;
                fetchBlocks(G, need, devRoute(need), d_frames, d_sigma6);
                todo.swap(need);
            }
            G.stats.timing.stage2Ms += nowMs() - t2;
            // ---- stage 3: batched images, thresholds, foreground ---------------------------------
            double t3 = nowMs();
            std::vector<int> loc;
            for (int s : pending)
                if (stacks[s].localize)
                    loc.push_back(s);
            if (!loc.empty())
                batchImages(G, loc, d_frames, d_mu, d_sigma6);
            G.stats.timing.stage3Ms += nowMs() - t3;
            // ---- stage 4: localize + track -------------------------------------------------------
            double t4 = nowMs();
            pool->parallelFor((int)loc.size(), [&](int k) { localize(stacks[loc[k]]); });
            vetoRound(G, loc, d_frames, d_sigma6);
            G.stats.timing.stage4Ms += nowMs() - t4;
            std::vector<int> next;
            for (int s : pending)
                if (!stacks[s].done)
                    next.push_back(s);
            pending.swap(next);
        }
        // results out, analyzers released
        pool->parallelFor(ns, [&](int k) {
            StackState &st_ = stacks[G.s0 + k];
            st_.capture(*st_.analyzer, st_.rectsBegin);
            st_.analyzer.reset();
        });
    }

    // What the stopped searches asked for: the next frame block of a stack (one launch per block index), or the dense rows
    // of frames of a block that is already there (one row-machine launch per launch of the block that holds them); then one
    // device search for the stacks of `ask`.  Returns when all of it is on the host: blocks arrived, answers collected.
    void fetchBlocks(Group &G, const std::vector<int> &need, const std::vector<int> &ask, const uint8_t *d_frames,
                     const uint8_t *d_sigma6)
    {
        hipStream_t stream = kernelStream(G);
        // (block, its launch that holds the pieces; -1: the block itself) -> the stacks that ask for it, block by block
        std::map<std::pair<int, int>, std::vector<int>> asked;
        for (int sI : need) {
            const BatchEventData &d = stacks[sI].data;
            asked[{d.need.block, d.need.pieces ? d.ref[d.need.block].fetch : -1}].push_back(sI);
        }
        {
            std::lock_guard<std::mutex> lock(launchMu); // (the counters, and one launch sequence at a time per pipeline)
            for (const auto &a : asked)
                if (a.first.second < 0)
                    G.search.launchBlock(a.first.first, a.second, stacks, d_frames, d_sigma6, stream, stats);
                else
                    G.search.completePieces(a.first.first, a.first.second, a.second, stacks, d_frames, d_sigma6, trigOn, stream, stats);
            // the searches that asked go on right behind the launches that produce what they asked for
            G.search.launchSearch(ask, stacks, stream, stats);
            HIPOK(hipEventRecord(G.blockDone.get(), stream));
        }
        HIPOK(hipEventSynchronize(G.blockDone.get()));
        for (int sI : need)
            G.search.served(stacks[sI].data);
        G.search.collectSearch(stacks, G.stats);
    }

    // trigger knob: what FindTriggerFrame(true, MatTrigFrame + 1) would have left in the analyzer, from the device search's
    // answer (K6, abub_trigger.hip).  false: the search needs frames (the request is recorded as diffHist would have recorded
    // it; nothing to roll back).  A look-ahead frame that cannot be decoded throws what the host search throws.
    bool applySearch(StackState &st_)
    {
        AnalyzerUnit *A = st_.analyzer.get();
        BatchEventData &d = st_.data;
        const abub_trig_result r = st_.trigRes;
        st_.trigReady = false;
        if (r.state == ABUB_TRIG_NEED_FRAMES || r.state == ABUB_TRIG_NEED_FINAL) {
            const int k = d.blockOf(r.need_frame);
            const bool pieces = r.state == ABUB_TRIG_NEED_FINAL;
            if (pieces ? !d.ref[k].deferred() : d.ref[k].launched())
                throw std::runtime_error("RunPipeline: the device trigger search asked for a frame that is there");
            d.request(k, r.need_frame, pieces);
            return false;
        }
        if (r.state == ABUB_TRIG_BAD_LOOKAHEAD)
            throw std::runtime_error("AnalyzerUnit::FindTriggerFrame: undecodable look-ahead frame");
        if (r.state != ABUB_TRIG_DONE)
            throw std::runtime_error("RunPipeline: unknown answer of the device trigger search");
        const int s = (int)(&st_ - stacks.data());
        if (r.status == -9 && d.F >= 5 && !meta.empty()) { // the line FindTriggerFrame prints for the frame it stopped at
            const int i = A->MatTrigFrame + 1 + r.evaluated;
            if (i >= 0 && i < (int)meta[s].names.size())
                std::cout << "Image " << meta[s].names[i] << " is corrupted/empty of camera " << s % C << " for the event "
                          << meta[s].eventID << "." << std::endl;
        }
        A->TriggerFrameIdentificationStatus = r.status;
        if (r.loc_thres >= 0)
            A->loc_thres = r.loc_thres;
        if (r.status == 0)
            A->MatTrigFrame = r.trig;
        else
            A->okToProceed = false;
        return true;
    }

    // What the host search may change in the analyzer before it runs out of evaluated frames (it only ever appends to
    // pix_counts), taken before the search; restore() puts it back
    struct AnalyzerSnapshot {
        size_t pixSize[256];
        bool havePix, ok;
        int trig, loc, status;
        explicit AnalyzerSnapshot(const AnalyzerUnit &A)
            : havePix(A.pix_counts.size() == 256), ok(A.okToProceed), trig(A.MatTrigFrame), loc(A.loc_thres),
              status(A.TriggerFrameIdentificationStatus)
        {
            for (int b = 0; havePix && b < 256; ++b)
                pixSize[b] = A.pix_counts[b].size();
        }
        void restore(AnalyzerUnit &A) const
        {
            for (int b = 0; havePix && b < 256 && A.pix_counts.size() == 256; ++b)
                A.pix_counts[b].resize(pixSize[b]);
            A.MatTrigFrame = trig;
            A.loc_thres = loc;
            A.TriggerFrameIdentificationStatus = status;
            A.okToProceed = ok;
        }
    };

    // AnyCamAnalysis body up to LocalizeOMatic (AutoBubStart3.cpp:87-107): the search on its route, then the plan.  A search
    // that stopped at frames that are not there leaves its request in st_.data (asked()) and the analyzer as it was
    void triggerAndPlan(StackState &st_)
    {
        st_.localize = false;
        st_.data.clearNeed();
        AnalyzerUnit *A = st_.analyzer.get();
        try {
            if (devRoute((int)(&st_ - stacks.data()))) {
                if (!st_.trigReady)
                    throw std::runtime_error("RunPipeline: no answer of the device trigger search for this stack");
                if (!applySearch(st_))
                    return;
            } else {
                const AnalyzerSnapshot before(*A);
                try {
                    A->FindTriggerFrame(true, A->MatTrigFrame + 1);
                } catch (NeedMoreFrames &) {
                    before.restore(*A);
                    return;
                }
            }
            if (!A->okToProceed) {
                st_.staged = A->TriggerFrameIdentificationStatus;
                st_.done = true;
            } else if (st_.data.F <= 5) { // LocalizeOMatic refuses (L3Localizer.cpp:889) -> -8
                A->LocalizeOMatic("");
                st_.staged = -8;
                st_.done = true;
            } else
                planImages(st_);
        } catch (std::exception &e) {
            st_.error = e.what();
            st_.staged = -6;
            st_.done = true;
        }
    }

    // the images stage 3 makes for the trigger the search found: the genesis pair and the tracking frames behind it
    void planImages(StackState &st_)
    {
        const AnalyzerUnit *A = st_.analyzer.get();
        BatchEventData &d = st_.data;
        const int t = A->MatTrigFrame;
        d.planned.clear();
        d.cur = nullptr;
        d.locReady = false;
        d.clearVeto(); // a new trigger: new veto keys
        // genesis: largestBoxArea / allInBellowsMask need the small contours too
        d.planned.push_back(
            PlannedImage::make(0, t, std::max(t - refOffset(A->TrainedData->TrainingSetSize), 0), A->loc_thres, -1));
        const int last = (t < 29) ? NumFramesBubbleTrack : (39 - t);
        for (int k = 1; k <= last && t + k < d.F; ++k) // (this stack's frame count: <= the pipeline's)
            d.planned.push_back(PlannedImage::make(1, t + k, 0, 3, kTrackMinBoxArea));
        st_.localize = true;
    }

    void batchImages(Group &G, const std::vector<int> &loc, const uint8_t *d_frames, const uint8_t *d_mu,
                     const uint8_t *d_sigma6)
    {
        // Kernels go to `stream`, results come back on the group's own stream
        hipStream_t stream = kernelStream(G);
        hipStream_t back = G.stream.get();
        // slots: all genesis images first (K2), then all post-trigger images (K3), camera-major: consecutive K3 jobs
        // then share their model, which is what lets one scanning wave serve several tracking frames (k3_zero_scan)
        int nd = 0, np = 0;
        for (int s : loc)
            for (PlannedImage &p : stacks[s].data.planned)
                (p.kind == 0 ? nd : np)++;
        std::vector<int> order(loc);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return a % C < b % C; });
        int di = 0, pi = nd;
        for (int s : order) {
            const int c = s % C;
            for (PlannedImage &p : stacks[s].data.planned) {
                p.slot = p.kind == 0 ? di++ : pi++;
                abub_job &j = G.jobs3.h[p.slot];
                j.cur = (uint32_t)(s * F + p.i);
                j.ref = (uint32_t)(s * F + p.ref);
                j.model = (uint32_t)c;
                j.out = (uint32_t)(p.kind == 0 ? p.slot : p.slot - nd);
            }
        }
        const int nimg = nd + np, nloc = (int)loc.size();
        double ta = nowMs();
        // the knobs, read once per batch (Group has their stages): localize implies contours, which implies blobs
        const bool useLocalize = localizeDev != 0, useContours = contours != 0 || useLocalize, useBlobs = blobs != 0 || useContours;
        Group::Blobs &B = G.blobs;
        Group::Contours &K = G.contours;
        Group::Localize &Z = G.loc;
        CandidateList &L = G.list;
        std::vector<PlannedImage *> bySlot((size_t)nimg);
        for (int s : loc) {
            stacks[s].data.roundHists = G.hist3.h;
            for (PlannedImage &p : stacks[s].data.planned) {
                bySlot[p.slot] = &p;
                G.thr.h[p.slot] = p.tozero; // candidate cut = TOZERO threshold, known before the launch
            }
        }
        if (useBlobs)
            B.firstUse(G.n3, L, W, H); // (before the candidate list starts its batch: it makes room for the kept pixels)
        for (int attempt = 0;; ++attempt) {
            G.jobs3.toDevice(nimg, stream);
            G.thr.toDevice(nimg, stream);
            L.start(stream);
            if (abub_fast_path(W)) {
                // images are never materialised: histogram + candidate list come out of the same pass
                check(abub_diff_hist_compact_dev(d_frames, d_sigma6, G.jobs3.d, nd, W, H, G.hist3.d, nullptr, G.thr.d, L.pairs,
                                                 L.cap(), L.count.d, 0, stream),
                      "stage3 K2 compact");
                if (np > 0)
                    check(abub_posttrig_compact_dev(d_frames, d_mu, d_sigma6, G.jobs3.d + nd, np, W, H,
                                                    G.hist3.d + (size_t)nd * 256, nullptr, G.thr.d + nd, L.pairs, L.cap(),
                                                    L.count.d, (uint32_t)nd, stream),
                          "stage3 K3 compact");
            } else {
                check(abub_diff_hist_dev(d_frames, d_sigma6, G.jobs3.d, nd, W, H, G.hist3.d, G.img, 0, stream),
                      "stage3 K2 store");
                if (np > 0)
                    check(abub_posttrig_dev(d_frames, d_mu, d_sigma6, G.jobs3.d + nd, np, W, H, G.hist3.d + (size_t)nd * 256,
                                            G.img + (size_t)nd * P, stream),
                          "stage3 K3");
                check(abub_fg_compact_pairs_dev(G.img, nimg, W, H, G.thr.d, L.pairs, L.cap(), L.count.d, stream), "stage3 K4");
            }
            // group the list by image on the device; the host gets contiguous runs and never re-buckets
            // (per-slot counts come from the histograms the same launches produced: no counting pass)
            L.group(nimg, G.hist3.d, G.thr.d, stream, "stage3 group");
            if (useBlobs)
                B.launch(L, bySlot, G.hist3.d, G.thr.d, W, H, stream);
            if (useContours)
                K.launch(G.n3, L, B.koff.d, nimg, W, H, stream);
            if (useLocalize)
                Z.launch(G.ns, C, locCap, deviceMasks(), K, stacks, loc, nimg, stream);
            HIPOK(hipEventRecord(G.kernelsDone.get(), stream));
            HIPOK(hipStreamWaitEvent(back, G.kernelsDone.get(), 0));
            G.hist3.toHost((size_t)nimg * 256, back);
            L.offsetsToHost(nimg, back);
            if (useBlobs)
                B.countsToHost(nimg, back);
            if (useContours)
                K.countsToHost(nimg, back);
            if (useLocalize)
                Z.countsToHost(nloc, back);
            HIPOK(hipStreamSynchronize(back));
            if (useBlobs)
                B.addTimings(G.stats);
            if (useContours)
                K.addTimings(G.stats);
            if (useLocalize)
                Z.addTimings(G.stats);
            G.stats.timing.s3GpuMs += nowMs() - ta; // launches + kernels + hist/count D2H
            ta = nowMs();
            G.stats.timing.pairs = *L.count.h;
            // Needed vs. capacity: the kernels keep counting past a list's capacity, so the needed size is known (0: the
            // list's knob is off).  The lists of the first step that does not fit grow, once (the kernels that used them are
            // done: `back` waited for them), and the batch is redone: 1, dense foreground (e.g. a flash frame); 2, contours
            // and vertices; 3, the records, from K5's true count -- before step 4, because K7b declines (INCOMPLETE) every
            // stack with records beyond the record list and a declined stack reserves no boxes or tracks, so while the records
            // do not fit the two totals are lower bounds; 4, the boxes and tracks, from totals that are true counts now
            const uint32_t nc = useContours ? K.coff.h[nimg] : 0, nv = nc ? K.poff.h[nimg] : 0;
            const uint32_t *total = useLocalize ? (const uint32_t *)Z.totals.h : nullptr;
            const Fit rows[] = {
                {&L.gidx, *L.count.h, "RunPipeline: foreground list overflow (dense foreground in too many images)", 1, false},
                {&K.cnpts, nc, "RunPipeline: contour list overflow after it was grown", 2, false},
                {&K.pts, nv, "RunPipeline: contour list overflow after it was grown", 2, false},
                {&Z.desc, total ? nc : 0, "RunPipeline: localizer record list overflow after it was grown", 3, true},
                {&Z.rects, total ? total[0] : 0, "RunPipeline: localizer box / track list overflow after it was grown", 4, true},
                {&Z.tracks, total ? total[1] : 0, "RunPipeline: localizer box / track list overflow after it was grown", 4, true}};
            const Fit *grew = fitLists(rows, sizeof rows / sizeof *rows, attempt);
            if (!grew)
                break;
            G.stats.loc.regrows += grew->locRegrow;
        }
        // The lists travel; with the blobs knob the kept pixels in place of the candidates
        if (useBlobs)
            B.listsToHost(back, L, nimg, useContours ? (const uint32_t *)K.cstats.h : nullptr, G.stats);
        else
            L.pairsToHost(back);
        if (useContours)
            K.listsToHost(back, nimg, !useLocalize || Z.declined(nloc), G.stats);
        if (useLocalize)
            Z.listsToHost(back, K.coff.h[nimg], nloc, G.stats);
        // thresholds (TOZERO + Otsu) on the host from the histograms, while the lists travel (pointers into the lists: taken
        // after the grow loop, used until the next batch replans every image; what a knob that is off would bind is default)
        pool->parallelFor(nimg, [&](int k) {
            PlannedImage &p = *bySlot[k];
            p.thr = binarizeThresholdFromHist(G.hist3.h + (size_t)k * 256, P, p.tozero);
            if (useBlobs)
                B.bind(p, k, L);
            else
                L.bind(p, k);
            if (useContours)
                K.bind(p, k);
        });
        HIPOK(hipStreamSynchronize(back));
        for (int k = 0; useLocalize && k < nloc; ++k)
            Z.bind(stacks[loc[k]].data, k, G.stats);
        G.stats.timing.s3ListMs += nowMs() - ta; // list D2H (+ thresholds)
    }

    // ---- bellows veto round ----------------------------------------------------------------------------------------
    // The stacks of `loc` whose localize stopped at a veto request (NeedBellows) are served together on the group's own
    // stream, one host synchronisation per sub-round: first the template matches (trigger and pre-trigger frames, one
    // launch per template), then the residual images; after each, localize runs again on those stacks.  The round's
    // planned images (hist3, list) stay untouched: the veto has buffers of its own.
    void vetoRound(Group &G, const std::vector<int> &loc, const uint8_t *d_frames, const uint8_t *d_sigma6)
    {
        const double t0 = nowMs();
        bool any = false;
        for (int sub = 0;; ++sub) {
            std::vector<int> ask;
            for (int s : loc)
                if (stacks[s].needBellows)
                    ask.push_back(s);
            if (ask.empty())
                break;
            any = true;
            bool served = false, fallback = false;
            if (sub < 3) {
                try {
                    served = vetoMatches(G, ask, d_frames) || vetoResiduals(G, ask, d_frames, d_sigma6);
                } catch (VetoFallback &) {
                    fallback = true;
                } catch (AllocError &) {
                    fallback = true;
                }
                if (fallback) {
                    // no room for the veto buffers, or a shape the batched matcher refuses: the one-at-a-time path takes
                    // these stacks, as it took every veto before
                    for (int s : ask) {
                        stacks[s].needBellows = false;
                        stacks[s].dropIn = true;
                        stacks[s].done = true;
                    }
                    break;
                }
            }
            if (!served) {
                for (int s : ask) {
                    stacks[s].needBellows = false;
                    stacks[s].error = "bellows veto: request left unserved by the veto round";
                    stacks[s].staged = -6;
                    stacks[s].done = true;
                }
                break;
            }
            pool->parallelFor((int)ask.size(), [&](int k) { localize(stacks[ask[k]]); });
        }
        if (any)
            G.stats.bellows.vetoMs += nowMs() - t0;
    }

    struct VetoFallback {};

    // the group's device copy of a bellows template, uploaded once on the group's stream (the only stream that uses it;
    // the host Mat is the process-wide mask cache's, immutable and kept alive by the entry)
    const uint8_t *deviceTemplate(Group &G, const cv::Mat &t)
    {
        for (auto &e : G.veto.templates)
            if (sameTemplate(e.first, t))
                return e.second;
        DeviceArray<uint8_t> d;
        d.allocate(t.total());
        HIPOK(hipMemcpyAsync(d, t.data, t.total(), hipMemcpyHostToDevice, G.stream.get()));
        G.veto.templates.emplace_back(t, std::move(d));
        return G.veto.templates.back().second;
    }

    // every outstanding match request of the asking stacks; false if there is none
    bool vetoMatches(Group &G, const std::vector<int> &ask, const uint8_t *d_frames)
    {
        std::vector<cv::Mat> tpl;
        std::vector<std::vector<std::pair<int, BatchEventData::MatchMemo *>>> byT;
        for (int s : ask)
            for (BatchEventData::MatchMemo &m : stacks[s].data.matches) {
                if (m.ready)
                    continue;
                size_t t = 0;
                while (t < tpl.size() && !sameTemplate(tpl[t], m.templ))
                    ++t;
                if (t == tpl.size()) {
                    tpl.push_back(m.templ);
                    byT.emplace_back();
                }
                byT[t].emplace_back(s, &m);
            }
        if (tpl.empty())
            return false;
        Group::Veto &V = G.veto;
        int total = 0;
        size_t scratch = 0;
        for (size_t t = 0; t < tpl.size(); ++t) {
            total += (int)byT[t].size();
            const size_t need = abub_match_best_scratch_bytes(W, H, tpl[t].cols, tpl[t].rows, (int)byT[t].size());
            if (need == 0)
                throw VetoFallback();
            scratch = std::max(scratch, need);
        }
        // (the veto's earlier work on the group's stream has been waited for: growing frees the old buffers)
        if (V.capJobs < total) {
            const int cap = std::max(total, 2 * V.capJobs);
            V.capJobs = 0;
            V.fidx.allocate(cap);
            V.xy.allocate(2 * (size_t)cap);
            V.capJobs = cap;
        }
        if (V.scratchBytes < scratch) {
            V.scratchBytes = 0;
            V.scratch.allocate(scratch);
            V.scratchBytes = scratch;
        }
        hipStream_t st = G.stream.get();
        int off = 0;
        for (size_t t = 0; t < tpl.size(); ++t) {
            const int n = (int)byT[t].size();
            const uint8_t *dt = deviceTemplate(G, tpl[t]);
            for (int q = 0; q < n; ++q)
                V.fidx.h[off + q] = (uint32_t)(byT[t][q].first * F + byT[t][q].second->frame);
            V.fidx.toDevice(n, st, off);
            const int rc = abub_match_best_batch_dev(d_frames, W, H, V.fidx.d + off, n, dt, tpl[t].cols, tpl[t].rows,
                                                     V.xy.d + 2 * off, V.scratch, V.scratchBytes, st);
            if (rc == ABUB_E_INVALID) // refused before anything was queued (e.g. a frame wider than the matcher takes)
                throw VetoFallback();
            check(rc, "bellows veto match");
            off += n;
            ++G.stats.bellows.matchLaunches;
        }
        V.xy.toHost(2 * (size_t)total, st);
        HIPOK(hipStreamSynchronize(st));
        off = 0;
        for (size_t t = 0; t < tpl.size(); ++t)
            for (auto &r : byT[t]) {
                r.second->xy = cv::Point2f(V.xy.h[2 * off], V.xy.h[2 * off + 1]);
                r.second->ready = true;
                ++off;
            }
        G.stats.bellows.matchJobs += total;
        return true;
    }

    // every outstanding residual request of the asking stacks; false if there is none
    bool vetoResiduals(Group &G, const std::vector<int> &ask, const uint8_t *d_frames, const uint8_t *d_sigma6)
    {
        std::vector<std::pair<int, BatchEventData::ResidualMemo *>> req;
        for (int s : ask)
            for (BatchEventData::ResidualMemo &r : stacks[s].data.residuals)
                if (!r.ready)
                    req.emplace_back(s, &r);
        if (req.empty())
            return false;
        Group::Veto &V = G.veto;
        CandidateList &L = V.list;
        const int n = (int)req.size();
        if (V.capImg < n) {
            const int cap = std::max(n, 2 * V.capImg);
            V.capImg = 0;
            V.rend.allocate(2 * (size_t)cap * P);
            V.syn.allocate((size_t)cap * P);
            V.img.allocate((size_t)cap * P);
            V.rhist.allocate((size_t)cap * 256);
            V.hist.allocate((size_t)cap * 256);
            V.jobs.allocate(cap);
            V.thr.allocate(cap);
            L.allocate(cap);
            V.capImg = cap;
        }
        if (L.cap() == 0)
            L.gidx.seed(pairCap > 0 ? (uint32_t)pairCap : 1u << 20);
        hipStream_t st = G.stream.get();
        // the two renderings of the template (L3Localizer.cpp:326-334), then everything on the device with no sync between
        pool->parallelFor(n, [&](int k) {
            const BatchEventData::ResidualMemo &r = *req[k].second;
            uint8_t *t = V.rend.h + 2 * (size_t)k * P, *p = t + P;
            std::memset(t, 0, 2 * P);
            for (int y = 0; y < r.templ.rows; ++y) {
                std::memcpy(t + (size_t)(r.rt.y + y) * W + r.rt.x, r.templ.ptr<uchar>(y), (size_t)r.templ.cols);
                std::memcpy(p + (size_t)(r.rp.y + y) * W + r.rp.x, r.templ.ptr<uchar>(y), (size_t)r.templ.cols);
            }
        });
        V.rend.toDevice(2 * (size_t)n * P, st);
        for (int k = 0; k < n; ++k) {
            const int s = req[k].first, c = s % C;
            const BatchEventData::ResidualMemo &r = *req[k].second;
            // ROI ProcessFrame(trig copy, pre copy) (:355); the pre copy lies after the trigger copy, as the kernel wants
            check(abub_diff_roi_dev(V.rend.d + 2 * (size_t)k * P, V.rend.d + (2 * (size_t)k + 1) * P, d_sigma6 + (size_t)c * P, W, H,
                                    r.roi.x, r.roi.y, r.roi.width, r.roi.height, V.syn + (size_t)k * P, V.rhist + (size_t)k * 256,
                                    st),
                  "bellows veto ROI ProcessFrame");
            abub_job &j = V.jobs.h[k];
            j.cur = (uint32_t)(s * F + r.trig);
            j.ref = (uint32_t)(s * F + r.pre);
            j.model = (uint32_t)c;
            j.out = (uint32_t)k;
            V.thr.h[k] = stacks[s].analyzer->loc_thres; // TOZERO cut of contoursOfCurrentImage
        }
        V.jobs.toDevice(n, st);
        V.thr.toDevice(n, st);
        // D(trig; pre) stored, minus the synthetic diff (overTheSigma -= diff_frame, :362)
        check(abub_diff_hist_dev(d_frames, d_sigma6, V.jobs.d, n, W, H, V.hist.d, V.img, 0, st), "bellows veto K2 store");
        for (int k = 0; k < n; ++k)
            check(abub_subsat_hist_dev(V.img + (size_t)k * P, V.syn + (size_t)k * P, W, H, V.hist.d + (size_t)k * 256, st),
                  "bellows veto subtract");
        for (int attempt = 0;; ++attempt) {
            L.start(st);
            check(abub_fg_compact_pairs_dev(V.img, n, W, H, V.thr.d, L.pairs, L.cap(), L.count.d, st), "bellows veto K4");
            L.group(n, V.hist.d, V.thr.d, st, "bellows veto group");
            V.hist.toHost((size_t)n * 256, st);
            L.offsetsToHost(n, st);
            HIPOK(hipStreamSynchronize(st));
            const Fit row = {&L.gidx, *L.count.h, "RunPipeline: bellows veto foreground list overflow", 1, false};
            if (!fitLists(&row, 1, attempt)) // (grows after the sync above: only K4 is redone)
                break;
        }
        L.pairsToHost(st);
        HIPOK(hipStreamSynchronize(st));
        for (int k = 0; k < n; ++k) {
            const int s = req[k].first;
            BatchEventData::ResidualMemo &r = *req[k].second;
            std::memcpy(r.hist, V.hist.h + (size_t)k * 256, sizeof(r.hist));
            PlannedImage &p = r.img = PlannedImage::make(2, r.trig, r.pre, V.thr.h[k], -1);
            p.slot = k;
            p.thr = binarizeThresholdFromHist(r.hist, P, p.tozero);
            // valid until the veto's next sub-round: a ready memo is read only by the localize that directly follows
            L.bind(p, k);
            r.ready = true;
            if (!stacks[s].vetoed) {
                stacks[s].vetoed = true;
                ++G.stats.bellows.vetoed;
            }
        }
        G.stats.bellows.residualImages += n;
        return true;
    }

    // cam<N>_mask.bmp and cam<N>_bellows_mask.bmp of every camera as L3Localizer::isInMask reads them, decoded through the
    // process-wide mask cache and uploaded once per pipeline (one entry per camera comes back); no mask dir, or a file that
    // is not loadable: no mask
    const abub_loc_mask *deviceMasks()
    {
        std::lock_guard<std::mutex> lock(maskMu);
        if (masksReady)
            return locMasks.data();
        locMasks.assign((size_t)C, abub_loc_mask{});
        maskBuf.clear();
        maskBuf.resize(2 * (size_t)C);
        for (int c = 0; c < C && !maskDir.empty(); ++c)
            for (int b = 0; b < 2; ++b) {
                const cv::Mat m = cachedMaskImage(maskDir + "/cam" + std::to_string(c) + (b ? "_bellows_mask.bmp" : "_mask.bmp"));
                if (m.empty())
                    continue;
                DeviceArray<uint8_t> &buf = maskBuf[2 * (size_t)c + b];
                buf.allocate((size_t)m.cols * m.rows);
                HIPOK(hipMemcpy((uint8_t *)buf, m.data, (size_t)m.cols * m.rows, hipMemcpyHostToDevice)); // (a Mat is continuous)
                abub_loc_mask &k = locMasks[(size_t)c];
                (b ? k.bel : k.fid) = buf;
                (b ? k.bw : k.fw) = m.cols;
                (b ? k.bh : k.fh) = m.rows;
            }
        masksReady = true;
        return locMasks.data();
    }

    // AnyCamAnalysis body from LocalizeOMatic on (AutoBubStart3.cpp:94-110)
    void localize(StackState &st_)
    {
        st_.needBellows = false;
        AnalyzerUnit *A = st_.analyzer.get();
        try {
            st_.rectsBegin = A->bubbleRects.size(); // (a round the veto serves throws before it pushes any)
            A->LocalizeOMatic("");
            if (!A->okToProceed) {
                st_.staged = -8;
                st_.done = true;
                return;
            }
            st_.staged = A->BubbleList.empty() ? -1 : 0;
            st_.done = !A->BubbleList.empty(); // no accepted bubble: search on from the next frame
        } catch (NeedBellows &) {
            st_.needBellows = true; // not done: served by the veto round, then localized again
        } catch (NeedsDropInPath &) {
            st_.dropIn = true;
            st_.done = true;
        } catch (std::exception &e) {
            st_.error = e.what();
            st_.staged = -6;
            st_.done = true;
        }
    }
};

const Knob RunPipeline::knobs[4] = {{"blobs", "ABUB_PIPE_BLOBS", &RunPipeline::blobs},
                                    {"contours", "ABUB_PIPE_CONTOURS", &RunPipeline::contours},
                                    {"trigger", "ABUB_PIPE_TRIGGER", &RunPipeline::trigger},
                                    {"localize", "ABUB_PIPE_LOCALIZE", &RunPipeline::localizeDev}};

void RunPipelineDelete::operator()(RunPipeline *p) const { delete p; }

RunPipelinePtr newRunPipeline(int device, int W, int H, int F, int E, int C, const int *tss, int nthreads, const char *maskDir)
{
    return RunPipelinePtr(new RunPipeline(device, W, H, F, E, C, tss, nthreads, maskDir));
}
void setSigmaRaw(RunPipeline &p, const uint8_t *d_sigma) { p.d_sigmaRaw = d_sigma; }
bool setTrainingSetSizes(RunPipeline &p, const int *tss)
{
    if (chainStrideOf(tss, p.C) != p.search.chainStride)
        return false;
    for (int c = 0; c < p.C; ++c) {
        p.tss[c] = tss[c];
        p.trainers[c]->TrainingSetSize = tss[c];
    }
    return true;
}
void setStackMeta(RunPipeline &p, std::vector<StackMeta> &&meta) { p.setStackMeta(std::move(meta)); }
void run(RunPipeline &p, const uint8_t *d_frames, const uint8_t *d_mu, const uint8_t *d_sigma6, hipStream_t stream)
{
    p.run(d_frames, d_mu, d_sigma6, stream);
}
void writeEvent(RunPipeline &p, int k, int eventNumber, OutputWriter &out) { p.writeEvent(k, eventNumber, out); }
int bellowsVetoed(const RunPipeline &p) { return (int)p.stats.bellows.vetoed; }
const StackResult &stackResult(const RunPipeline &p, int s) { return p.stacks[s]; }
const std::string &stackEventID(const RunPipeline &p, int s) { return p.meta[s].eventID; }

} // namespace abub

// ---- C surface (bench.py / tests) ---------------------------------------------------------------
extern "C" {

void *abh_pipe_new(int device, int W, int H, int F, int E, int C, const int *tss, int nthreads, const char *maskdir)
{
    try {
        return new abub::RunPipeline(device, W, H, F, E, C, tss, nthreads, maskdir);
    } catch (std::exception &e) {
        fprintf(stderr, "abh_pipe_new: %s\n", e.what());
        return nullptr;
    }
}

void abh_pipe_free(void *p) { delete (abub::RunPipeline *)p; }

static thread_local std::string g_pipeErr;
const char *abh_pipe_error() { return g_pipeErr.c_str(); }

void abh_pipe_set_sigma(void *p, const void *sigma_dev) { ((abub::RunPipeline *)p)->d_sigmaRaw = (const uint8_t *)sigma_dev; }

int abh_pipe_run(void *p, const void *frames_dev, const void *mu_dev, const void *sigma6_dev, void *stream)
{
    try {
        ((abub::RunPipeline *)p)->run((const uint8_t *)frames_dev, (const uint8_t *)mu_dev, (const uint8_t *)sigma6_dev,
                                      (hipStream_t)stream);
        return 0;
    } catch (std::exception &e) {
        g_pipeErr = e.what();
        return -1;
    }
}

int abh_pipe_run_host(void *p, const void *frames_host, const void *mu_dev, const void *sigma6_dev)
{
    try {
        ((abub::RunPipeline *)p)->runFromHost((const uint8_t *)frames_host, (const uint8_t *)mu_dev, (const uint8_t *)sigma6_dev);
        return 0;
    } catch (std::exception &e) {
        g_pipeErr = e.what();
        return -1;
    }
}

// stack s of the last run as a StackResult for the abh_result_* readers (capi.cpp)
const void *abh_pipe_stack(void *p, int s)
{
    const abub::StackResult &res = ((abub::RunPipeline *)p)->stacks[s];
    return &res;
}

// The counters of the last run, one getter per struct of PipeStats: the struct has the getter's slots in their order and
// says what each counts (summed over stack groups and rounds; a knob's are zeros when the knob was off).  out[0..4],
// [0..5], [0..9], [0..4], [0..7], and [0..11] with the number of rounds as the return value
static const abub::PipeStats &statsOf(void *p) { return ((abub::RunPipeline *)p)->stats; }
void abh_pipe_bellows(void *p, double *out) { abub::copySlots(statsOf(p).bellows, out); }
void abh_pipe_trigger_stats(void *p, double *out) { abub::copySlots(statsOf(p).trigger, out); }
void abh_pipe_localize_stats(void *p, double *out) { abub::copySlots(statsOf(p).loc, out); }
void abh_pipe_contour_stats(void *p, double *out) { abub::copySlots(statsOf(p).contours, out); }
void abh_pipe_blob_stats(void *p, double *out) { abub::copySlots(statsOf(p).blobs, out); }
int abh_pipe_timing(void *p, double *out)
{
    abub::copySlots(statsOf(p).timing, out);
    return statsOf(p).rounds;
}

// out[0..1]: the first two numbers of abh_pipe_trigger_stats summed over every pipeline run of this process so far (the
// pipelines of a batched run are its own: a caller takes the difference around it)
void abh_pipe_trigger_totals(double *out)
{
    out[0] = (double)abub::g_trigTotals[0].load();
    out[1] = (double)abub::g_trigTotals[1].load();
}

// ... and the same for abh_pipe_localize_stats: stacks localised on the device, stacks on the host route
void abh_pipe_localize_totals(double *out)
{
    out[0] = (double)abub::g_locTotals[0].load();
    out[1] = (double)abub::g_locTotals[1].load();
}

// Run-time knobs of one pipeline object, each 0 or 1 (RunPipeline::knobs has the names, and the environment variables
// that give a new pipeline its values, else 0).  Results never depend on them.
//  - "blobs": 0 = the host applies the Otsu cut to every candidate pixel; 1 = the device labels the foreground and ships
//    only the pixels of the components the localizer can use.
//  - "contours": 1 = the device also traces the contours of those components (K5) and ships their vertices, whatever
//    "blobs" says; a slot the kernel declines keeps the host route.
//  - "trigger": 1 = stage 2's trigger search runs on the device (K6) for every stack inside abub_trigger_search_limits;
//    the host search stays for the others.  Read at the start of a run.
//  - "localize": 1 = stage 3 also describes the contours and runs the localizer's decisions per stack on the device (K7),
//    whatever "contours" and "blobs" say; a stack the kernels decline keeps the host route.
// Checked in this order, -1 for each: an unknown name, a value other than 0 or 1, no handle.
int abh_pipe_set_option(void *p, const char *name, int value)
{
    const std::string opt = name ? name : "";
    const abub::Knob *knob = nullptr;
    for (const abub::Knob &k : abub::RunPipeline::knobs)
        if (opt == k.name)
            knob = &k;
    if (!knob) {
        g_pipeErr = std::string("abh_pipe_set_option: unknown option ") + (name ? name : "(null)");
        return -1;
    }
    if (value != 0 && value != 1) {
        g_pipeErr = "abh_pipe_set_option: " + opt + " takes 0 or 1";
        return -1;
    }
    if (!p) {
        g_pipeErr = "abh_pipe_set_option: no pipeline";
        return -1;
    }
    ((abub::RunPipeline *)p)->*knob->value = value;
    return 0;
}
}
