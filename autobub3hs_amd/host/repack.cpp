// repack.cpp -- a run rewritten with its frames in the packed format (cv::abfEncode, DESIGN section 3, "Packed frames"): abub3hs --repack.
// Host only: no GPU, no analysis.  Everything is read through the Parser interface, so a directory and a zip archive
// repack alike; the result is always a directory.
#include <cerrno>
#include <cstdio>
#include <fstream>
#include <mutex>
#include <sstream>
#include <stdexcept>

#include <sys/stat.h>

#include "driver.hpp"
#include "framefiles.hpp"
#include "runbatch.hpp"

namespace abub {

namespace {

bool makeDirs(const std::string &path)
{
    for (size_t at = 1; at <= path.size(); ++at)
        if (at == path.size() || path[at] == '/') {
            const std::string part = path.substr(0, at);
            if (mkdir(part.c_str(), 0777) != 0 && errno != EEXIST)
                return false;
        }
    struct stat sb;
    return stat(path.c_str(), &sb) == 0 && S_ISDIR(sb.st_mode);
}

bool writeFile(const std::string &path, const unsigned char *data, size_t n)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f)
        return false;
    const bool ok = fwrite(data, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

std::string trimSlashes(std::string s)
{
    while (s.size() > 1 && s.back() == '/')
        s.pop_back();
    return s;
}

} // namespace

int RepackRun(Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir_,
              const std::string &imageFolder, int numCams, int nthreads, RepackStats *stats)
{
    const double t0 = nowMs();
    RepackStats st;
    const std::string dstRunDir = trimSlashes(dstRunDir_);
    {
        // the files keep their names: written into the source run they would replace the frames they are read from
        struct stat a, b;
        if (!srcRunDir.empty() && stat(srcRunDir.c_str(), &a) == 0 && stat(dstRunDir.c_str(), &b) == 0 && a.st_dev == b.st_dev &&
            a.st_ino == b.st_ino)
            throw std::runtime_error("repack: " + dstRunDir + " is the run that is being read");
    }
    std::vector<std::string> events = sortedEvents(*parser);
    struct Task {
        size_t ev;
        std::string name;
    };
    std::vector<Task> tasks;
    std::vector<std::string> dirs(events.size());
    bool failed = false;
    for (size_t e = 0; e < events.size(); ++e) {
        dirs[e] = trimSlashes(dstRunDir + "/" + events[e] + "/" + imageFolder);
        for (size_t at; (at = dirs[e].find("//")) != std::string::npos;)
            dirs[e].erase(at, 1);
        if (!makeDirs(dirs[e])) {
            failed = true;
            continue;
        }
        for (int c = 0; c < numCams; ++c) {
            std::vector<std::string> names;
            parser->ParseAndSortFramesInFolder(events[e], c, names);
            for (std::string &n : names)
                tasks.push_back(Task{e, std::move(n)});
        }
    }
    st.events = (int)events.size();

    // ---- the run's event file: the source's bytes where there is such a file, else one line per listed event ------------
    if (makeDirs(dstRunDir)) {
        const size_t slash = dstRunDir.find_last_of('/');
        const std::string runId = slash == std::string::npos ? dstRunDir : dstRunDir.substr(slash + 1);
        std::ifstream in(srcRunFile, std::ios::binary);
        std::ostringstream text;
        if (!srcRunFile.empty() && in)
            text << in.rdbuf();
        else {
            std::vector<std::string> listed;
            parser->GetRunFileInfo(listed);
            for (const std::string &ev : listed) // (the eleven columns GetRunFileInfo reads; the second is the event)
                text << runId << ' ' << ev << " 0 0 0 0 0 0 0 0 0\n";
        }
        const std::string s = text.str();
        if (!s.empty() && !writeFile(dstRunDir + "/" + runId + ".txt", (const unsigned char *)s.data(), s.size()))
            failed = true;
    } else
        failed = true;

    std::mutex mu;
    forEachTask(parser, nthreads, tasks.size(), [&](Parser &p, size_t i) {
        const Task &t = tasks[i];
        static thread_local std::vector<unsigned char> file, packed;
        const long long size = p.GetImageFileSize(events[t.ev], t.name);
        bool ok = size >= 0 && size < ((long long)1 << 30);
        bool isPacked = false;
        if (ok) {
            file.resize((size_t)size);
            ok = !size || p.ReadImageFile(events[t.ev], t.name, file.data(), file.size()) == size;
        }
        if (ok) {
            const cv::Mat m = size ? cv::imdecode(file.data(), file.size(), 0) : cv::Mat();
            isPacked = !m.empty() && cv::abfEncode(m.data, m.cols, m.rows, packed);
            // a file that does not decode is copied as it is: it stays undecodable
            const std::vector<unsigned char> &outv = isPacked ? packed : file;
            ok = writeFile(dirs[t.ev] + "/" + t.name, outv.data(), outv.size());
        }
        std::lock_guard<std::mutex> lock(mu);
        if (!ok)
            ++st.failed;
        else if (isPacked) {
            ++st.packed;
            st.bytesIn += size;
            st.bytesOut += (long long)packed.size();
        } else
            ++st.copied;
    });
    st.total_s = (nowMs() - t0) * 1e-3;
    if (stats)
        *stats = st;
    return failed || st.failed ? 1 : 0;
}

} // namespace abub
