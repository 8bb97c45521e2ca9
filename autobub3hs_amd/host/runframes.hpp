// runframes.hpp -- a run as the list of its frames, for the tools that visit every frame without analysing any: repack
// (repack.cpp), verify (verify.cpp) and survey (survey.cpp).  The list, the size the GPU decoders are set up for, the read
// of a whole file and the device check are one copy here (the decoders' width gate and the batch size: framefiles.hpp),
// and so are the two helpers with which repack and the peek images (peek.cpp) put files on disk.  Internal to the host
// library.
#ifndef ABUB3HS_RUNFRAMES_HPP
#define ABUB3HS_RUNFRAMES_HPP

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <sys/stat.h>

#include <hip/hip_runtime_api.h>

#include "ParseFolder/Parser.hpp"

namespace abub {

inline std::string trimSlashes(std::string s)
{
    while (s.size() > 1 && s.back() == '/')
        s.pop_back();
    return s;
}

// The directory `path` and those above it, made where they are missing.  false: *failed cannot be made or is no directory
// (errno says why)
inline bool makeDirs(const std::string &path, std::string *failed = nullptr)
{
    std::string part;
    for (size_t at = 1; at <= path.size(); ++at)
        if (at == path.size() || path[at] == '/') {
            part = path.substr(0, at);
            if (mkdir(part.c_str(), 0777) != 0 && errno != EEXIST)
                break;
            part = path;
        }
    struct stat sb;
    if (part == path && stat(path.c_str(), &sb) == 0 && S_ISDIR(sb.st_mode))
        return true;
    if (failed)
        *failed = part;
    return false;
}

// The n bytes at `data` as the file `path`.  false: it cannot be opened (*opened says whether it was), or not all of it was written
inline bool writeFile(const std::string &path, const unsigned char *data, size_t n, bool *opened = nullptr)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (opened)
        *opened = f != nullptr;
    if (!f)
        return false;
    const bool ok = fwrite(data, 1, n, f) == n;
    return fclose(f) == 0 && ok;
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

// A file through its parser; one that cannot be read counts as empty
inline void readWhole(Parser &p, const std::string &ev, const std::string &name, std::vector<unsigned char> &file)
{
    file.clear();
    long long size = -1;
    try {
        size = p.GetImageFileSize(ev, name);
        if (size <= 0 || size >= ((long long)1 << 30))
            return;
        file.resize((size_t)size);
        if (p.ReadImageFile(ev, name, file.data(), file.size()) != size)
            file.clear();
    } catch (...) {
        file.clear();
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
