// stackresult.hpp -- what is kept of the analysis of one (event, camera) stack once its analyzer is gone: the record that
// the test C-API (capi.cpp, the Run's last analysis) and the run pipeline (pipeline.cpp, one per stack) fill, read out and
// hand to the recon writer.  Internal to the host library.
#ifndef ABUB3HS_STACKRESULT_HPP
#define ABUB3HS_STACKRESULT_HPP

#include <algorithm>
#include <cstddef>
#include <memory>
#include <string>
#include <vector>

#include "AnalyzerUnit.hpp"
#include "PICOFormatWriter/PICOFormatWriterV4.hpp"

namespace abub {

struct BubbleOut {
    std::vector<BubbleImageFrame> desc;
    std::vector<float> dz;
    float dzdt, drdt;
};

// a descriptor as a row of doubles (the C surface, the writer probe; host.DESC_KEYS names the columns)
constexpr int kDescRow = 11; // x y w h area radius m00 m10 m01 cx cy
inline void descToRow(const BubbleImageFrame &f, double *out)
{
    out[0] = f.newPosition.x;
    out[1] = f.newPosition.y;
    out[2] = f.newPosition.width;
    out[3] = f.newPosition.height;
    out[4] = f.ContArea;
    out[5] = f.ContRadius;
    out[6] = f.moments.m00;
    out[7] = f.moments.m10;
    out[8] = f.moments.m01;
    out[9] = f.MassCentres.x;
    out[10] = f.MassCentres.y;
}
inline BubbleImageFrame descFromRow(const double *r)
{
    BubbleImageFrame f;
    f.newPosition = cv::Rect((int)r[0], (int)r[1], (int)r[2], (int)r[3]);
    f.ContArea = r[4];
    f.ContRadius = r[5];
    f.moments.m00 = r[6];
    f.moments.m10 = r[7];
    f.moments.m01 = r[8];
    f.MassCentres = cv::Point2f((float)r[9], (float)r[10]);
    return f;
}

struct StackResult {
    int staged = 0; // the status AnyCamAnalysis stages for the camera (0, -3, -9, -8, -6)
    int trig = 0, status = 0, loc_thres = 0, ok = 0; // the analyzer's MatTrigFrame, TriggerFrameIdentificationStatus, ...
    std::vector<BubbleOut> bubbles;
    std::string error; // the exception text behind a -6
    std::vector<cv::Rect> rects; // the analyzer's bubbleRects of its last LocalizeOMatic round (the boxes of _4_BubbleDetected)

    // the analyzer's state and the track record of every bubble (`staged` and `error` belong to whoever drove it)
    // rectsBegin: how many bubbleRects the analyzer held before that round (the list is never cleared between retries)
    void capture(AnalyzerUnit &A, size_t rectsBegin = 0)
    {
        rects.assign(A.bubbleRects.begin() + (std::ptrdiff_t)std::min(rectsBegin, A.bubbleRects.size()), A.bubbleRects.end());
        trig = A.MatTrigFrame;
        status = A.TriggerFrameIdentificationStatus;
        loc_thres = A.loc_thres;
        ok = A.okToProceed;
        bubbles.clear();
        for (bubble *b : A.BubbleList)
            bubbles.push_back(BubbleOut{b->KnownDescriptors, b->dz, b->dZdT(), b->dRdT()});
    }
};

// Stages results into an OutputWriter.  The writer borrows `bubble` objects, so they are rebuilt from the stored
// descriptors and owned here: the holder must outlive the writer's writeCameraOutput().
class StagedBubbles {
    std::vector<std::unique_ptr<bubble>> owned;

public:
    void stage(OutputWriter &out, const StackResult &r, int camera, int event)
    {
        if (r.staged != 0) {
            out.stageCameraOutputError(camera, r.staged, event);
            return;
        }
        std::vector<bubble *> list;
        for (const BubbleOut &bo : r.bubbles) {
            bubble *b = new bubble(bo.desc[0]);
            owned.emplace_back(b);
            for (size_t d = 1; d < bo.desc.size(); ++d) {
                b->lockThisIteration = false;
                *b << bo.desc[d];
            }
            list.push_back(b);
        }
        out.stageCameraOutput(list, camera, r.trig, event);
    }
};

} // namespace abub
#endif
