// devctx.hpp -- glue between the analysis classes and the C-ABI (include/abub_hip.h layer B):
// a per-host-thread GPU context and the HBM-resident image of one (event, camera).
#ifndef ABUB3HS_DEVCTX_HPP
#define ABUB3HS_DEVCTX_HPP

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "abub_hip.h"
#include "bubble/bubble.hpp"
#include "cvlite.hpp"

class Parser;
class Trainer;

namespace abub {

// contours whose bounding box has at most this area are dropped in a tracking frame (L3Localizer.cpp:800-805)
constexpr int kTrackMinBoxArea = 10;

// Throws std::runtime_error carrying abub_last_error(): AnyCamAnalysis maps exceptions to status -6
// (reference AutoBubStart3.cpp:114-117).
void check(int rc, const char *what);

// One context per host thread, recreated when the frame geometry changes or more frames are needed.
class DeviceContext {
public:
    static DeviceContext &forThread(int W, int H, int minFrames);
    static void releaseThread();
    abub_ctx *ctx = nullptr;
    int W = 0, H = 0, maxF = 0;
    unsigned long long residentModel = 0; // Trainer::ModelId currently in HBM
    unsigned long long residentEvent = 0; // serial of the EventOnDevice currently in the frame slab (0: none)
    void ensureModel(const Trainer &t);
    ~DeviceContext();
};

// What the analysis classes need from the GPU for one (event, camera).  Two providers exist:
// EventOnDevice (below: decodes through the Parser, uploads into the per-thread context, one call at
// a time -- the drop-in path) and the batched provider of RunPipeline (pipeline.cpp: every stack of a
// run is already resident in HBM and all launches are shared across events).
class EventData {
public:
    virtual ~EventData() {}
    int F = 0, W = 0, H = 0;
    virtual bool frameOk(int i) const = 0;
    // host copy of frame i, or an empty Mat when the frames only exist in HBM
    virtual cv::Mat hostFrame(int i) const = 0;
    // histogram of D(frame[i]; frame[max(i-refOffset,0)])
    virtual const uint32_t *diffHist(int i, int refOffset) = 0;
    // D(frame[i]; frame[ref]) becomes the current image; returns its histogram
    virtual const uint32_t *diffFrame(int i, int ref, cv::Mat *out = nullptr) = 0;
    virtual const uint32_t *diffFrameROI(int i, int ref, cv::Rect roi, cv::Mat *out = nullptr) = 0;
    // post-trigger image of frame i becomes the current image; returns its histogram
    virtual const uint32_t *postTrig(int i, cv::Mat *out = nullptr) = 0;
    // foreground (v > thr) raster indices of the current image
    virtual void foreground(int thr, std::vector<uint32_t> &idx) = 0;
    // foreground raster indices of the current image, of which a provider may leave out the pixels of 8-connected
    // components whose bounding box has area <= minBoxArea (-1: none left out): the contours such components yield are
    // dropped by the caller anyway, and they enclose no other component (abub_blobs.hip).  Default: foreground().
    virtual void foregroundKept(int thr, int minBoxArea, std::vector<uint32_t> &idx) { foreground(thr, idx); }
    // the external contours of the current image's foreground as ContourFinder::find returns them for foregroundKept()'s
    // pixels, when the provider already has them (traced on the device, abub_contours.hip): true and `out` filled.
    // false: the caller traces the pixels of foregroundKept() itself.  Default: false.
    virtual bool contoursKept(int thr, int minBoxArea, std::vector<std::vector<cv::Point>> &out)
    {
        (void)thr;
        (void)minBoxArea;
        (void)out;
        return false;
    }
    // a finished localisation of trigger frame `trig`, when the provider has one (decided on the device, abub_localize.hip):
    // true, the boxes of L3Localizer::bubbleRects appended to `rects` and per bubble its descriptors in sighting order (the
    // genesis first) in `tracks`.  false: LocalizeOMatic runs as it always has.  Default: false.
    virtual bool localized(int trig, std::vector<cv::Rect> &rects, std::vector<std::vector<BubbleImageFrame>> &tracks)
    {
        (void)trig;
        (void)rects;
        (void)tracks;
        return false;
    }
    // bellows veto: exact correlation terms of frame i against a template ((H-th+1) x (W-tw+1) placements)
    virtual void matchTerms(int i, const cv::Mat &templ, std::vector<unsigned long long> &num,
                            std::vector<unsigned long long> &wsum2) = 0;
    // current image = saturate(current image - sub); returns the new histogram
    virtual const uint32_t *subtractFromCurrent(const cv::Mat &sub) = 0;

    // bellows veto, TrackAFeature (L3Localizer.cpp:473-510): best template position in frame i.
    // Default: matchTerms, normalised on the host (bestMatchFromTerms).
    virtual cv::Point2f bestMatch(int i, const cv::Mat &templ);
    // bellows veto, L3Localizer.cpp:326-362: the template rendered at rt (trigger copy) and at rp (pre-trigger copy), the
    // ROI ProcessFrame of the two renderings subtracted from D(trig; pre), which becomes the current image; returns its
    // histogram.  Default: host renders, processFrameROI, diffFrame, subtractFromCurrent.
    virtual const uint32_t *bellowsResidual(int trig, int pre, const cv::Mat &templ, cv::Rect rt, cv::Rect rp,
                                            cv::Rect diffROI);
    // AnalyzerUnit::ProcessFrame(cur, ref, out, 5, roi) with this event's model (used by the default bellowsResidual)
    virtual void processFrameROI(cv::Mat &cur, cv::Mat &ref, cv::Rect roi, cv::Mat &out);
};

// the mask image L3Localizer::isInMask reads from `path` (cam<N>_mask.bmp, cam<N>_bellows_mask.bmp), decoded once per
// process; empty when the file is missing or not loadable
cv::Mat cachedMaskImage(const std::string &path);

// AnalyzerUnit::ProcessFrame (AnalyzerUnit.cpp:79-97) on two host images with `model`: the pair is staged as a two-frame
// stack in the thread's context; out = D(cur; ref) on `roi` (the whole frame: the full-frame kernel)
void processFrameOnDevice(const Trainer &model, cv::Mat &cur, cv::Mat &ref, cv::Rect roi, cv::Mat &out);

// thrown by a provider that cannot serve a request (the batched pipeline re-runs such a stack one at a time)
struct NeedsDropInPath : public std::runtime_error {
    explicit NeedsDropInPath(const char *what) : std::runtime_error(what) {}
};

// Decoded frames of one (event, camera), pushed through the per-thread context on demand.
class EventOnDevice : public EventData {
public:
    EventOnDevice(Parser *parser, const std::string &eventID, const std::vector<std::string> &frameNames,
                  const Trainer *model);
    ~EventOnDevice() override;
    std::vector<cv::Mat> frames; // empty Mat == Parser::GetImage returned -1
    bool frameOk(int i) const override { return i >= 0 && i < F && !frames[i].empty(); }
    cv::Mat hostFrame(int i) const override { return frames[i]; }

    // all frames are evaluated in one batched launch the first time any histogram is asked for
    const uint32_t *diffHist(int i, int refOffset) override;
    const uint32_t *diffFrame(int i, int ref, cv::Mat *out = nullptr) override;
    const uint32_t *diffFrameROI(int i, int ref, cv::Rect roi, cv::Mat *out = nullptr) override;
    const uint32_t *postTrig(int i, cv::Mat *out = nullptr) override;
    void foreground(int thr, std::vector<uint32_t> &idx) override;
    void matchTerms(int i, const cv::Mat &templ, std::vector<unsigned long long> &num,
                    std::vector<unsigned long long> &wsum2) override;
    const uint32_t *subtractFromCurrent(const cv::Mat &sub) override;
    void processFrameROI(cv::Mat &cur, cv::Mat &ref, cv::Rect roi, cv::Mat &out) override;

private:
    DeviceContext &resident();
    const Trainer *model_;
    unsigned long long serial_; // process-wide, never reused (what DeviceContext::residentEvent remembers)
    std::vector<uint32_t> hists_[3]; // per refOffset (1,2): [F][256], empty until computed
    uint32_t lastHist_[256];
};

} // namespace abub
#endif
