// repack.cpp -- a run rewritten with its frames in the packed format (cv::abfEncode, DESIGN section 3, "Packed frames"): abub3hs --repack.
// No analysis.  Everything is read through the Parser interface, so a directory and a zip archive repack alike; the result
// is always a directory.  RepackRun is host only (cv::imdecode + cv::abfEncode on the pool's threads); RepackRunDevice
// (--repack-gpu) decodes the frames of the run's size with the GPU decoders and encodes them with abub_abf_encode_dev, and
// writes the same bytes.  What both share -- the refusal to write into the run being read, the directory layout, the run's
// event file, what becomes of a single file on a host thread, the exit status -- is one copy.
// UnpackRun / UnpackRunDevice (abub3hs --unpack [--unpack-gpu]) are the same two routes with another codec: every frame
// becomes a canonical Huffman-only PNG (cv::pngHuffEncode / abub_png_encode_dev; DESIGN section 3, "Unpacking a run").
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdexcept>

#include <sys/stat.h>

#include "driver.hpp"
#include "encodebatch.hpp"
#include "framefiles.hpp"
#include "runbatch.hpp"
#include "runframes.hpp"

namespace abub {

namespace {

// what became of one frame
struct Outcome {
    bool ok = false, packed = false;
    long long in = 0, out = 0; // of a packed frame: the source file's bytes, the packed file's
};

// The bytes of a source file on a host thread: decoded at whatever size the file has and packed, or, where they do not
// decode, copied as they are (the file stays undecodable)
Outcome packBytes(const Codec &codec, const unsigned char *data, size_t size, const std::string &path)
{
    static thread_local std::vector<unsigned char> packed;
    Outcome o;
    const cv::Mat m = size ? cv::imdecode(data, size, 0) : cv::Mat();
    o.packed = !m.empty() && codec.encode(m.data, m.cols, m.rows, packed);
    o.ok = o.packed ? writeFile(path, packed.data(), packed.size()) : writeFile(path, data, size);
    o.in = (long long)size;
    o.out = (long long)packed.size();
    return o;
}

// One frame read through the parser and packed on this thread
Outcome hostFrame(const Codec &codec, Parser &p, const std::string &ev, const std::string &name, const std::string &path)
{
    static thread_local std::vector<unsigned char> file;
    const long long size = p.GetImageFileSize(ev, name);
    if (size < 0 || size >= ((long long)1 << 30))
        return Outcome();
    file.resize((size_t)size);
    if (size && p.ReadImageFile(ev, name, file.data(), file.size()) != size)
        return Outcome();
    return packBytes(codec, file.data(), file.size(), path);
}

using Task = FrameTask;

// The part of a repack that is not its frames
struct Plan {
    std::string dstRunDir;
    std::vector<std::string> events, dirs; // dirs[e]: where the frames of events[e] go
    std::vector<Task> tasks;               // every frame, in event, camera and frame order
    bool failed = false;                   // a directory or the event file could not be written
    std::string pathOf(const Task &t) const { return dirs[t.ev] + "/" + t.name; }
};

Plan planRun(const Codec &codec, Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir_,
             const std::string &imageFolder, int numCams)
{
    Plan pl;
    pl.dstRunDir = trimSlashes(dstRunDir_);
    const std::string &dstRunDir = pl.dstRunDir;
    {
        // the files keep their names: written into the source run they would replace the frames they are read from
        struct stat a, b;
        if (!srcRunDir.empty() && stat(srcRunDir.c_str(), &a) == 0 && stat(dstRunDir.c_str(), &b) == 0 && a.st_dev == b.st_dev &&
            a.st_ino == b.st_ino)
            throw std::runtime_error(std::string(codec.what) + ": " + dstRunDir + " is the run that is being read");
    }
    pl.events = sortedEvents(*parser);
    const std::vector<std::string> &events = pl.events;
    pl.dirs.resize(events.size());
    for (size_t e = 0; e < events.size(); ++e) {
        std::string &dir = pl.dirs[e];
        dir = trimSlashes(dstRunDir + "/" + events[e] + "/" + imageFolder);
        for (size_t at; (at = dir.find("//")) != std::string::npos;)
            dir.erase(at, 1);
        if (!makeDirs(dir)) {
            pl.failed = true;
            continue;
        }
        appendEventFrames(*parser, events[e], e, numCams, pl.tasks);
    }

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
            pl.failed = true;
    } else
        pl.failed = true;
    return pl;
}

// The frames' outcomes summed into the stats, from any thread
struct Tally {
    RepackStats &st;
    std::mutex mu;
    void add(const Outcome &o, bool onGpu = false)
    {
        std::lock_guard<std::mutex> lock(mu);
        if (onGpu)
            ++st.framesGpuEncoded;
        else
            ++st.framesHostRoute;
        if (!o.ok)
            ++st.failed;
        else if (o.packed) {
            ++st.packed;
            st.bytesIn += o.in;
            st.bytesOut += o.out;
        } else
            ++st.copied;
    }
};

void hostFrames(const Codec &codec, Parser *parser, const Plan &pl, int nthreads, Tally &tally)
{
    forEachTask(parser, nthreads, pl.tasks.size(), [&](Parser &p, size_t i) {
        const Task &t = pl.tasks[i];
        tally.add(hostFrame(codec, p, pl.events[t.ev], t.name, pl.pathOf(t)));
    });
}

// The device route: the frames in batches of at most 4 per CU (ABUB_REPACK_BATCH=n, a test knob: of at most n, never more).  Per batch: the pool reads the files into a pinned buffer
// (and packs, on the spot, what is no file for the GPU decoders: a frame it had to decode itself, a frame of another size,
// a file that does not decode); upload; both decoders into a slab; the codec's device encoder over the frames that are in place
// (EncodeBatch, encodebatch.hpp: its files come back in pinned memory); the pool writes the files.
void deviceFrames(const Codec &codec, Parser *parser, const Plan &pl, int nthreads, int device, int W, int H, Tally &tally)
{
    RepackStats &st = tally.st;
    HIPOK(hipSetDevice(device));
    size_t perBatch = framesPerBatch(device);
    if (const char *e = getenv("ABUB_REPACK_BATCH")) { // (a test knob: several batches of a small run; it can only lower the size)
        const long v = atol(e);
        if (v > 0)
            perBatch = std::min(perBatch, (size_t)v);
    }
    const size_t P = (size_t)W * H;
    FileBatch B; // the batch's files, the decoders' scratch, the slab of decoded frames (frame i at i * P)
    std::vector<FileTask> &ft = B.ft;
    EncodeBatch enc; // the packed files of a batch
    Stream stream;
    hipStream_t cs = stream.get();
    B.sizer.reset(parser->clone());

    for (size_t i0 = 0; i0 < pl.tasks.size(); i0 += perBatch) {
        const size_t n = std::min(perBatch, pl.tasks.size() - i0);
        // ---- read -------------------------------------------------------------------------------------------------------
        double t0 = nowMs();
        B.begin();
        for (size_t i = 0; i < n; ++i)
            B.plan((int)i, 0, pl.events[pl.tasks[i0 + i].ev], pl.tasks[i0 + i].name);
        B.ready();
        const auto readOne = [&](Parser &p, size_t i) {
            const Task &t = pl.tasks[i0 + i];
            FileTask &f = ft[i];
            const std::string &ev = pl.events[t.ev];
            if (!B.read(p, i, ev, t.name, W, H) || f.onGpu()) // (not read yet: once more after the device's inflate)
                return;
            if (f.state == FileTask::HostDecoded) { // (16-bit, colour, BMP: this thread decoded it at W x H)
                static thread_local std::vector<unsigned char> packed;
                Outcome o;
                o.packed = codec.encode(f.pix.data(), W, H, packed);
                o.ok = o.packed && writeFile(pl.pathOf(t), packed.data(), packed.size());
                o.in = f.size;
                o.out = (long long)packed.size();
                tally.add(o);
            } else if (f.read) // another size, or a file that does not decode
                tally.add(packBytes(codec, B.h_files.get() + f.off, (size_t)f.size, pl.pathOf(t)));
            else               // a file the parser does not hand out in one piece
                tally.add(hostFrame(codec, p, ev, t.name, pl.pathOf(t)));
            f.pix = std::vector<uint8_t>();
            f.state = FileTask::Other;
        };
        forEachTask(parser, nthreads, n, readOne);
        B.inflate(parser, nthreads, cs, readOne);
        st.framesGpuUnzipped += B.unzip.unzipped;
        st.read_s += (nowMs() - t0) * 1e-3;

        // ---- upload and decode ------------------------------------------------------------------------------------------
        t0 = nowMs();
        std::vector<uint64_t> src;
        std::vector<size_t> slot;
        B.reset(n, n * P);
        B.upload(cs);
        if (B.launch(0, n, W, H, [&](int s, int) { return (uint64_t)s * P; }, cs)) {
            HIPOK(hipStreamSynchronize(cs));
            B.finish(W, H, cs);
            st.framesGpuPngDecoded = B.decodedBy[GpuPng];
            st.framesGpuUnpacked = B.decodedBy[GpuPacked];
            st.framesGpuBmpDecoded = B.decodedBy[GpuBmp];
            st.framesHostDecoded = B.hostDecoded;
            for (size_t i = 0; i < n; ++i)
                if (B.good[i]) {
                    src.push_back((uint64_t)i * P);
                    slot.push_back(i);
                }
        }
        HIPOK(hipStreamSynchronize(cs));
        st.decode_s += (nowMs() - t0) * 1e-3;

        // ---- encode and copy back (a packed frame is about the size of its PNG) ----------------------------------------------
        const size_t ng = src.size();
        enc.run(codec, B.slab.get(), n * P, src, W, H, B.total + 64 * ng, cs, st.encode_s, st.copy_s);

        // ---- write: the packed files, and on the host route what the decoders left (a PNG that is damaged behind its header) -
        t0 = nowMs();
        std::vector<size_t> fileOf(n, SIZE_MAX);
        for (size_t g = 0; g < ng; ++g)
            fileOf[slot[g]] = g;
        forEachTask(parser, nthreads, n, [&](Parser &, size_t i) {
            const Task &t = pl.tasks[i0 + i];
            if (ft[i].state == FileTask::Other)
                return; // (written by the thread that read it)
            if (fileOf[i] == SIZE_MAX) {
                tally.add(packBytes(codec, B.h_files.get() + ft[i].off, (size_t)ft[i].size, pl.pathOf(t)));
                return;
            }
            const EncodeBatch::File r = enc.file(fileOf[i]);
            Outcome o;
            o.packed = true;
            o.ok = r.status == 0 && writeFile(pl.pathOf(t), r.data, r.len);
            o.in = ft[i].size;
            o.out = r.len;
            tally.add(o, true);
        });
        st.write_s += (nowMs() - t0) * 1e-3;
        ++st.batches;
    }
}

int repackRun(const Codec &codec, Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir,
              const std::string &imageFolder, int numCams, int nthreads, int device, RepackStats *stats)
{
    const double t0 = nowMs();
    RepackStats st;
    if (device >= 0) // (before anything is written)
        requireDevice(device, codec.what, codec.noDevice);
    const Plan pl = planRun(codec, parser, srcRunDir, srcRunFile, dstRunDir, imageFolder, numCams);
    st.events = (int)pl.events.size();
    Tally tally{st, {}};
    int W = 0, H = 0;
    if (device >= 0 && firstFrameSize(parser, pl.events, pl.tasks, W, H) && decodersTakeWidth(W)) {
        st.device = device;
        st.W = W;
        st.H = H;
        deviceFrames(codec, parser, pl, nthreads, device, W, H, tally);
    } else
        hostFrames(codec, parser, pl, nthreads, tally);
    st.total_s = (nowMs() - t0) * 1e-3;
    if (stats)
        *stats = st;
    return pl.failed || st.failed ? 1 : 0;
}

} // namespace

int RepackRun(Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir,
              const std::string &imageFolder, int numCams, int nthreads, RepackStats *stats)
{
    return repackRun(kPacked, parser, srcRunDir, srcRunFile, dstRunDir, imageFolder, numCams, nthreads, -1, stats);
}

int RepackRunDevice(Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir,
                    const std::string &imageFolder, int numCams, int nthreads, int device, RepackStats *stats)
{
    if (device < 0)
        throw std::runtime_error("repack: no such HIP device: " + std::to_string(device));
    return repackRun(kPacked, parser, srcRunDir, srcRunFile, dstRunDir, imageFolder, numCams, nthreads, device, stats);
}

int UnpackRun(Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir,
              const std::string &imageFolder, int numCams, int nthreads, RepackStats *stats)
{
    return repackRun(kPng, parser, srcRunDir, srcRunFile, dstRunDir, imageFolder, numCams, nthreads, -1, stats);
}

int UnpackRunDevice(Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir,
                    const std::string &imageFolder, int numCams, int nthreads, int device, RepackStats *stats)
{
    if (device < 0)
        throw std::runtime_error("unpack: no such HIP device: " + std::to_string(device));
    return repackRun(kPng, parser, srcRunDir, srcRunFile, dstRunDir, imageFolder, numCams, nthreads, device, stats);
}

} // namespace abub
