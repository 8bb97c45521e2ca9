// peek.hpp -- the reference's six DebugPeek images (L3Localizer.cpp:222-257, 397, 448) written for the accepted stacks of a
// batch whose frames are resident in HBM: RunBatched's post-pass behind abub3hs --peek ("The peek
// planes").  Internal to the host library.
#ifndef ABUB3HS_PEEK_HPP
#define ABUB3HS_PEEK_HPP

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "cvlite.hpp"

namespace abub {

// One accepted stack: its final trigger and what the analyzer recorded for it
struct PeekStack {
    std::string eventID;
    int cam = 0;
    uint32_t trigFrame = 0, preFrame = 0; // frame numbers in the batch's slab: frame i lies at i * W * H
    int loc_thres = 0;                    // the TOZERO cut of the final trigger (AnalyzerUnit::loc_thres)
    std::vector<cv::Rect> rects;          // L3Localizer::bubbleRects of the final round
};

struct PeekStats {
    long long stacks = 0, files = 0, bytes = 0;
    int subBatches = 0;
};

// pre = max(trig - (tss < 6 ? 1 : 2), 0): the pre-trigger frame of L3Localizer.cpp:222, 885
inline int peekPreFrame(int trig, int tss)
{
    const int pre = trig - (tss < 6 ? 1 : 2);
    return pre < 0 ? 0 : pre;
}

// The two planes on a host thread, the definition of abub_peek_planes_dev: thr[i] = D[i] > cut ? 255 : 0, and pres = the
// trigger frame with cv::rectangle of every box
void peekPlanesHost(const uint8_t *D, const uint8_t *trig, int W, int H, int cut, const std::vector<cv::Rect> &rects, uint8_t *thr,
                    uint8_t *pres);

// Six canonical Huffman-only PNGs per stack under `dir` (which ends with '/'; created if missing):
// ev<EventID>_cam<c>_{000_AvgImage, 00_PreTrigFrame, 0_TrigFrame, 02_OvrThe6Sigma, 3_OtsuThresholded, 4_BubbleDetected}.png.
// One store-mode abub_diff_hist_dev launch per sub-batch gives D(trig, pre) and its histogram, the cut is
// binarizeThresholdFromHist(hist, W * H, loc_thres).  gpu: abub_peek_planes_dev forms the planes and abub_png_encode_dev
// the files, which come back finished; else the frames and D come back and `nthreads` host threads form the planes
// (peekPlanesHost) and encode (cv::pngHuffEncode): the same bytes.  The work is cut into sub-batches whose device buffers
// stay within budgetBytes (at least one stack each; maxStacks > 0: of at most that many stacks).  Work queued on `stream`
// is waited for; throws std::runtime_error on a HIP or IO failure.
void writePeekImages(int W, int H, int C, const uint8_t *d_frames, size_t framesBytes, const uint8_t *d_mu, const uint8_t *d_sigma6,
                     const std::vector<PeekStack> &stacks, const std::string &dir, bool gpu, size_t budgetBytes, int maxStacks,
                     int nthreads, hipStream_t stream, PeekStats &stats);

} // namespace abub
#endif
