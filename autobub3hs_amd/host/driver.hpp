// driver.hpp -- pieces of the reference's main program (AutoBubStart3.cpp) shared by the CLI (abub3hs_main.cpp,
// runbatch.cpp), the test C-API (capi.cpp) and the run pipeline's one-at-a-time path (pipeline.cpp): the numeric
// order of the events (:284) and the per-camera retry loop (AnyCamAnalysis, :67-125).
#ifndef ABUB3HS_DRIVER_HPP
#define ABUB3HS_DRIVER_HPP

#include <algorithm>
#include <exception>
#include <iostream>
#include <mutex>
#include <string>
#include <vector>

#include "AnalyzerUnit.hpp"
#include "PICOFormatWriter/PICOFormatWriterV4.hpp"
#include "ParseFolder/Parser.hpp"

namespace abub {

inline void sortEvents(std::vector<std::string> &events)
{
    std::sort(events.begin(), events.end(), [](const std::string &a, const std::string &b) { return std::stoi(a) < std::stoi(b); });
}
// every event of the parser's run, in numeric order
inline std::vector<std::string> sortedEvents(Parser &parser)
{
    std::vector<std::string> events;
    parser.GetEventDirLists(events);
    sortEvents(events);
    return events;
}

// Runs FindTriggerFrame / LocalizeOMatic until a bubble is found or the search fails (:87-117).  Returns the status to
// stage for the camera: 0 (A->BubbleList holds the bubbles), the trigger status (-3, -9) when FindTriggerFrame refuses,
// -8 when LocalizeOMatic does, -6 on an exception, whose text goes to `error`.  rectsBegin (may be NULL): how many
// bubbleRects A held before its last LocalizeOMatic round.
inline int analyzeUntilBubble(AnalyzerUnit *A, bool nonStopPref, const std::string &out_dir, std::string &error,
                              size_t *rectsBegin = nullptr)
{
    try {
        do {
            A->FindTriggerFrame(nonStopPref, A->MatTrigFrame + 1);
            if (!A->okToProceed)
                return A->TriggerFrameIdentificationStatus;
            if (rectsBegin)
                *rectsBegin = A->bubbleRects.size();
            A->LocalizeOMatic(out_dir);
            if (!A->okToProceed)
                return -8;
        } while (A->BubbleList.size() == 0); // an empty list would be staged as -1 (PICOFormatWriterV4.cpp:99-110): go on
        return 0;
    } catch (std::exception &e) {
        error = e.what();
        return -6;
    }
}

// The loop above with its outcome staged in `writer`.  Upstream stages in every iteration; only the last one counts
// (both staging calls overwrite the camera's record), so it is staged once.  Returns the staged status.
inline int AnyCamAnalysis(AnalyzerUnit *A, int camera, bool nonStopPref, OutputWriter *writer, const std::string &out_dir,
                          int actualEventNumber)
{
    static std::mutex stageMutex; // `#pragma omp critical` around the staging upstream (:96-97)
    std::string error;
    const int staged = analyzeUntilBubble(A, nonStopPref, out_dir, error);
    if (staged == -6)
        std::cout << error << '\n';
    if (staged == 0) {
        std::lock_guard<std::mutex> lock(stageMutex);
        writer->stageCameraOutput(A->BubbleList, camera, A->MatTrigFrame, actualEventNumber);
    } else
        writer->stageCameraOutputError(camera, staged, actualEventNumber);
    return staged;
}

} // namespace abub
#endif
