// runframes.hpp -- a run as the list of its frames, for the tools that visit every frame without analysing any: repack
// (repack.cpp) and verify (verify.cpp).  The list, the size the GPU decoders are set up for and the device check are one
// copy here (the decoders' width gate and the batch size: framefiles.hpp).  Internal to the host library.
#ifndef ABUB3HS_RUNFRAMES_HPP
#define ABUB3HS_RUNFRAMES_HPP

#include <algorithm>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "ParseFolder/Parser.hpp"

namespace abub {

inline std::string trimSlashes(std::string s)
{
    while (s.size() > 1 && s.back() == '/')
        s.pop_back();
    return s;
}

// One frame of a run: the index of its event in the run's sorted event list, and its file name
struct FrameTask {
    size_t ev;
    std::string name;
};

// Appends the frames of event `ev` (index e) that the parser lists for cameras 0 .. numCams-1, in camera and frame order
inline void appendEventFrames(Parser &parser, const std::string &ev, size_t e, int numCams, std::vector<FrameTask> &tasks)
{
    for (int c = 0; c < numCams; ++c) {
        std::vector<std::string> names;
        parser.ParseAndSortFramesInFolder(ev, c, names);
        for (std::string &n : names)
            tasks.push_back(FrameTask{e, std::move(n)});
    }
}

// The size of the first frame that decodes; false if none does
inline bool firstFrameSize(Parser *parser, const std::vector<std::string> &events, const std::vector<FrameTask> &tasks, int &W, int &H)
{
    std::unique_ptr<Parser> p(parser->clone());
    for (const FrameTask &t : tasks) {
        cv::Mat m;
        try {
            if (p->GetImage(events[t.ev], t.name, m) != -1 && !m.empty()) {
                W = m.cols;
                H = m.rows;
                return true;
            }
        } catch (...) {
        }
    }
    return false;
}

// Throws "<who>: no such HIP device: ..." when there is no device `device`; `hint` says what the caller does without one
inline void requireDevice(int device, const std::string &who, const std::string &hint)
{
    int count = 0;
    if (device < 0 || hipGetDeviceCount(&count) != hipSuccess || device >= count)
        throw std::runtime_error(who + ": no such HIP device: " + std::to_string(device) + " (" + std::to_string(std::max(count, 0)) +
                                 " found)" + hint);
}

} // namespace abub
#endif
