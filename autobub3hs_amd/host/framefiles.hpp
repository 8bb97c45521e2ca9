// framefiles.hpp -- frames read as FILES for the GPU decoders (abub_png_decode_dev, abub_abf_decode_dev,
// abub_bmp_decode_dev), shared by the batched detect path (runbatch.cpp), device training (devtrain.cpp) and the device
// routes of repack, unpack and verify.  A host thread reads each file; a packed frame ("ABF1") whose header is valid for
// W x H goes to the packed decoder as it is, a PNG has its chunks walked (pngWalk), a BMP its header (bmpWalk, with
// ABUB_GPU_BMP=1; by default BMP files stay with the reading thread); a file none of them takes
// (16-bit, colour or interlaced PNG, compressed BMP, another size) gets the host decoder's answer at once, and so does a
// frame a kernel later returns a nonzero status for.  Each decoder is one lane (GpuCodec) of a batch: the placement of its
// frames, its descriptors, its status buffers and its count are indexed by it, and launch and finish loop over the lanes.
// FileBatch is the unit "one set of files on the device, decoded into one slab" of device training, repack, unpack and
// verify; RunBatched keeps its own slots (its upload runs on the look-ahead thread) and uses the lanes.  The decoders'
// width gate, the batch size and the ABUB_GPU_DECODE override are one copy here.  Internal to the host library.
#ifndef ABUB3HS_FRAMEFILES_HPP
#define ABUB3HS_FRAMEFILES_HPP

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "ParseFolder/Parser.hpp"
#include "abub_hip.h"
#include "bmpwalk.hpp"
#include "devctx.hpp"
#include "holders.hpp"
#include "pipeline.hpp"
#include "pngwalk.hpp"

namespace abub {

// fn(state, i) for every i < n on up to `nthreads` threads, each with a state of its own from make().  The first exception
// is re-thrown once every thread has been joined (the others stop at their next task).
template <class Make, class Fn>
void forEachTaskWith(int nthreads, size_t n, const Make &make, const Fn &fn)
{
    std::atomic<size_t> next{0};
    std::mutex errMu;
    std::exception_ptr err;
    std::vector<std::thread> th;
    for (int t = 0; t < std::max(1, (int)std::min<size_t>(nthreads, n)); ++t)
        th.emplace_back([&]() {
            try {
                auto state = make();
                for (size_t i; (i = next.fetch_add(1)) < n;)
                    fn(state, i);
            } catch (...) {
                std::lock_guard<std::mutex> lock(errMu);
                if (!err)
                    err = std::current_exception();
                next = n;
            }
        });
    for (auto &t : th)
        t.join();
    if (err)
        std::rethrow_exception(err);
}

// fn(parser, i) for every i < n, each thread with its own clone of `parser`
template <class Fn>
void forEachTask(Parser *parser, int nthreads, size_t n, const Fn &fn)
{
    forEachTaskWith(
        nthreads, n, [&]() { return std::unique_ptr<Parser>(parser->clone()); },
        [&](std::unique_ptr<Parser> &p, size_t i) { fn(*p, i); });
}

// The GPU decoders, in launch order
enum GpuCodec { GpuPng = 0, GpuPacked = 1, GpuBmp = 2, NGpuCodecs = 3 };

// the decoders' width gate (the PNG kernels'; it holds for every lane): a run outside it takes the host route whole
inline bool decodersTakeWidth(int W) { return (W & 3) == 0 && W >= 4 && W <= 2048; }

// Are the frames of a W-wide run decoded on the GPU?  optGpuDecode: the caller's option (0: off); ABUB_GPU_DECODE=0 turns it off
inline bool gpuDecodeWanted(int optGpuDecode, int W)
{
    const char *e = getenv("ABUB_GPU_DECODE");
    return optGpuDecode != 0 && decodersTakeWidth(W) && (!e || atoi(e) != 0);
}

// frames per batch of a device route: at most 4 per CU (the inflate kernel runs four streams per CU at a time, and a batch
// takes as long as its longest stream)
inline size_t framesPerBatch(int device)
{
    int ncu = 256, v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && v > 0)
        ncu = v;
    return (size_t)4 * ncu;
}

// One frame to be read: where it goes is decided by the caller (s, f); `state` says what became of it
struct FileTask {
    // Planned: to be read (planFileTask); OnGpu: read and taken by the decoder `codec`; Other: not a file task (the
    // caller's own work)
    enum { Planned = 0, HostDecoded = 1, Bad = 2, Other = 3, OnGpu = 4 };
    bool onGpu() const { return state == OnGpu; }
    int s = 0, f = 0;
    long long size = 0;
    size_t off = 0; // in the pinned file buffer
    int state = Other;
    GpuCodec codec = GpuPng;
    bool read = false; // the file's bytes are in the buffer (a Bad frame may still have been read)
    PngInfo info;
    BmpInfo bmp;
    std::vector<uint8_t> pix;
};

static_assert(sizeof(abub_bmp_frame) == 32, "abub_bmp_frame is the 32 bytes include/abub_hip.h states");

// Where one frame of a batch is and where it goes
struct Placed {
    int s, f;
    uint32_t off, len; // the file inside the file buffer
    uint64_t dst;      // the decoded frame's byte offset from the output
};

// The descriptors of one decode launch, and the frames a reading thread decoded itself
struct FileDescs {
    size_t bytes = 0, zbytes = 0;      // of the files; of the PNG decoder's stream buffer
    std::vector<Placed> lane[NGpuCodecs]; // the frames each decoder takes, in task order
    long long decodedBy[NGpuCodecs] = {}; // of them, decoded by the kernel (finishFileDecode)
    std::vector<uint8_t> luts[NGpuCodecs]; // palette -> grey tables, 256 bytes each (the packed decoder has none)
    // what the C ABI takes: element i describes lane[...][i]
    std::vector<abub_png_frame> png;
    std::vector<abub_png_seg> segs;
    std::vector<abub_abf_frame> abf;
    std::vector<abub_bmp_frame> bmp;
    size_t gpuFrames() const
    {
        size_t n = 0;
        for (const std::vector<Placed> &l : lane)
            n += l.size();
        return n;
    }
    long long decoded() const { return std::accumulate(decodedBy, decodedBy + NGpuCodecs, 0LL); }
    std::vector<std::vector<uint8_t>> hostPix;
    std::vector<Placed> host; // of hostPix[i] (no file)
    long long bad = 0;
    // the index of `table` (256 bytes) among the lane's tables, appended if it is new (the frames of a run share theirs)
    uint32_t intern(GpuCodec c, const uint8_t *table)
    {
        std::vector<uint8_t> &pool = luts[c];
        size_t l = 0;
        while (l < pool.size() / 256 && memcmp(&pool[l * 256], table, 256))
            ++l;
        if (l == pool.size() / 256)
            pool.insert(pool.end(), table, table + 256);
        return (uint32_t)l;
    }
};

// The file's size and its place in the buffer (`total` grows by the file rounded up to 16 bytes); Bad if the parser
// cannot hand it out
inline void planFileTask(Parser &sizer, const std::string &ev, const std::string &name, FileTask &t, size_t &total)
{
    t.size = sizer.GetImageFileSize(ev, name);
    t.state = (t.size > 0 && t.size < ((long long)1 << 30)) ? FileTask::Planned : FileTask::Bad;
    t.off = total;
    if (t.state == FileTask::Planned)
        total += ((size_t)t.size + 15) & ~(size_t)15;
}

// a packed frame ("ABF1") whose header is valid for W x H: one for abub_abf_decode_dev
inline bool packedFrameOf(const uint8_t *data, size_t size, int W, int H)
{
    int w = 0, h = 0;
    return cv::abfProbe(data, size, &w, &h) && w == W && h == H;
}

// ABUB_GPU_BMP=1: BMP files go to the GPU decoder.  Off by default (BMP files stay with the reading threads, RunBatched's
// probe does not accept them): results are the same, but the batched run of a BMP directory measured slower with it
// than without ("BMP frames on the GPU").
inline bool gpuBmpEnabled()
{
    const char *e = getenv("ABUB_GPU_BMP");
    return e && atoi(e) != 0;
}

// Does a GPU decoder take the W x H file?  Which one, and what its walk found, into t
inline bool gpuCodecOf(const uint8_t *data, size_t size, int W, int H, FileTask &t)
{
    if (packedFrameOf(data, size, W, H)) // (the file goes up as it is; the kernel checks the rest)
        t.codec = GpuPacked;
    else if (pngWalk(data, size, W, H, t.info))
        t.codec = GpuPng;
    else if (gpuBmpEnabled() && bmpWalk(data, size, W, H, t.bmp))
        t.codec = GpuBmp;
    else
        return false;
    return true;
}

// On a pool thread: the file into files + t.off, walked for the W x H GPU decoder, else decoded here
inline void readFileTask(Parser &p, const std::string &ev, const std::string &name, FileTask &t, uint8_t *files, int W, int H)
{
    if (t.state != FileTask::Planned)
        return;
    uint8_t *dst = files + t.off;
    long long got = -1;
    try {
        got = p.ReadImageFile(ev, name, dst, (size_t)t.size);
    } catch (...) {
        got = -1;
    }
    if (got != t.size) {
        t.state = FileTask::Bad;
        return;
    }
    t.read = true;
    try {
        if (gpuCodecOf(dst, (size_t)t.size, W, H, t)) {
            t.state = FileTask::OnGpu;
            return;
        }
        // not a file for the GPU decoders (16-bit, colour, interlaced, another size): the host decoder's answer
        t.pix.resize((size_t)W * H);
        t.state = cv::imdecodeInto(dst, (size_t)t.size, t.pix.data(), W, H) ? FileTask::HostDecoded : FileTask::Bad;
    } catch (...) { // (an allocation that fails inside a pool thread must not end the batch)
        t.state = FileTask::Bad;
    }
}

// The descriptors of the tasks' frames, in task order; dstOf(s, f): byte offset of the decoded frame from the output
// (tasks [first, last); the files of every task are in one buffer of totalFileBytes)
template <class DstOf>
void buildFileDescs(FileTask *first, FileTask *last, size_t totalFileBytes, FileDescs &r, const DstOf &dstOf)
{
    r.bytes = totalFileBytes + 16;
    size_t zoff = 0;
    for (FileTask *tp = first; tp != last; ++tp) {
        FileTask &t = *tp;
        if (t.state == FileTask::Bad)
            ++r.bad;
        if (t.state != FileTask::HostDecoded && t.state != FileTask::OnGpu)
            continue;
        const Placed at{t.s, t.f, (uint32_t)t.off, (uint32_t)t.size, (uint64_t)dstOf(t.s, t.f)};
        if (t.state == FileTask::HostDecoded) {
            r.hostPix.push_back(std::move(t.pix));
            r.host.push_back(at);
            continue;
        }
        r.lane[t.codec].push_back(at);
        if (t.codec == GpuPacked)
            r.abf.push_back(abub_abf_frame{at.off, at.len, at.dst});
        else if (t.codec == GpuBmp) {
            abub_bmp_frame b;
            b.off = at.off;
            b.len = at.len;
            b.data_off = t.bmp.dataOff;
            b.stride = t.bmp.stride;
            b.bpp = (uint16_t)t.bmp.bpp;
            b.flags = t.bmp.topDown ? 1 : 0;
            b.lut = t.bmp.bpp <= 8 && !t.bmp.identity ? r.intern(GpuBmp, t.bmp.lut) : 0xffffffffu;
            b.dst = at.dst;
            r.bmp.push_back(b);
        } else {
            abub_png_frame d;
            d.seg_begin = (uint32_t)r.segs.size();
            d.seg_count = (uint32_t)t.info.segs.size();
            d.zoff = (uint32_t)zoff;
            d.zlen = (uint32_t)t.info.zlen;
            d.lut = t.info.palette ? r.intern(GpuPng, t.info.lut) : 0xffffffffu;
            d.reserved = 0;
            d.dst = at.dst;
            for (const abub_png_seg &sg : t.info.segs)
                r.segs.push_back(abub_png_seg{(uint32_t)(t.off + sg.off), sg.len});
            zoff += (((size_t)d.zlen + 15) & ~(size_t)15) + 16;
            r.png.push_back(d);
        }
    }
    r.zbytes = zoff + 16;
    if (r.bytes >= ((size_t)1 << 32) || r.zbytes >= ((size_t)1 << 32))
        throw std::runtime_error("a batch of more than 4 GB of files (lower the batch size)");
}

// The decoders' scratch, kept from one launch to the next: per lane its descriptors, tables and statuses on the device and
// the statuses in pinned memory; the PNG decoder also has its stream buffer, its unfiltered rows and its segments
struct DecodeScratch {
    struct Lane {
        DeviceBuffer desc, luts, status;
        PinnedBuffer h_status;
    } lane[NGpuCodecs];
    DeviceBuffer z, raw, segs; // PNG only
};

// One launch of each decoder that has frames in r, PNG, then packed, then BMP, into `out` (out_bytes), the statuses copied
// back into sc.lane[...].h_status; all queued on `stream` (so they stay behind whatever the caller queued there before, the
// clear of the batch's slab for one), not waited for.  The files are already in d_files.
inline void launchFileDecode(const FileDescs &r, const uint8_t *d_files, int W, int H, uint8_t *out, size_t out_bytes,
                             DecodeScratch &sc, hipStream_t stream)
{
    const void *const desc[NGpuCodecs] = {r.png.data(), r.abf.data(), r.bmp.data()};
    const size_t descSize[NGpuCodecs] = {sizeof(abub_png_frame), sizeof(abub_abf_frame), sizeof(abub_bmp_frame)};
    for (int c = 0; c < NGpuCodecs; ++c) {
        const int nf = (int)r.lane[c].size();
        if (!nf)
            continue;
        DecodeScratch::Lane &l = sc.lane[c];
        const std::vector<uint8_t> &luts = r.luts[c];
        l.desc.grow(nf * descSize[c]);
        l.status.grow((size_t)nf * sizeof(int32_t));
        if (c != GpuPacked)
            l.luts.grow(luts.size() + 256);
        if (l.h_status.capacity() < (size_t)nf * sizeof(int32_t))
            l.h_status.allocate((size_t)nf * sizeof(int32_t) + 64);
        HIPOK(hipMemcpyAsync(l.desc.get(), desc[c], nf * descSize[c], hipMemcpyHostToDevice, stream));
        if (!luts.empty())
            HIPOK(hipMemcpyAsync(l.luts.get(), luts.data(), luts.size(), hipMemcpyHostToDevice, stream));
        int32_t *status = (int32_t *)l.status.get();
        if (c == GpuPng) {
            sc.z.grow(r.zbytes);
            sc.raw.grow((size_t)nf * abub_png_raw_stride(W, H));
            sc.segs.grow(r.segs.size() * sizeof(abub_png_seg) + 8);
            HIPOK(hipMemcpyAsync(sc.segs.get(), r.segs.data(), r.segs.size() * sizeof(abub_png_seg), hipMemcpyHostToDevice, stream));
            check(abub_png_decode_dev(d_files, r.bytes, (const abub_png_frame *)l.desc.get(), nf, (const abub_png_seg *)sc.segs.get(),
                                      (int)r.segs.size(), l.luts.get(), (int)(luts.size() / 256), W, H, sc.z.get(), sc.z.capacity(),
                                      sc.raw.get(), sc.raw.capacity(), out, out_bytes, status, stream),
                  "abub_png_decode_dev");
        } else if (c == GpuPacked)
            check(abub_abf_decode_dev(d_files, r.bytes, (const abub_abf_frame *)l.desc.get(), nf, W, H, out, out_bytes, status, stream),
                  "abub_abf_decode_dev");
        else
            check(abub_bmp_decode_dev(d_files, r.bytes, (const abub_bmp_frame *)l.desc.get(), nf, l.luts.get(), (int)(luts.size() / 256),
                                      W, H, out, out_bytes, status, stream),
                  "abub_bmp_decode_dev");
        HIPOK(hipMemcpyAsync(l.h_status.get(), status, (size_t)nf * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    }
}

// After the launches above have been waited for: a frame the kernels refused takes the host decoder's answer (the same
// image, or the same failure), and the reading threads' own frames are uploaded.  ok(s, f) is called for every frame that
// is in place.  A frame its kernel decoded counts in r.decodedBy[its codec], one a host thread decoded in onHost.
template <class Ok>
void finishFileDecode(FileDescs &r, const uint8_t *h_files, const DecodeScratch &sc, uint8_t *out, int W, int H, hipStream_t stream,
                      const Ok &ok, long long &onHost)
{
    const size_t P = (size_t)W * H;
    std::vector<uint8_t> pix;
    // the frame at `at` whose decoder answered `status`
    auto settle = [&](int32_t status, const Placed &at) {
        uint8_t *dst = out + at.dst;
        if (status == 0) {
            ok(at.s, at.f);
            return true;
        }
        pix.resize(P);
        if (cv::imdecodeInto(h_files + at.off, at.len, pix.data(), W, H)) {
            HIPOK(hipMemcpy(dst, pix.data(), P, hipMemcpyHostToDevice));
            ok(at.s, at.f);
            ++onHost;
        } else {
            HIPOK(hipMemsetAsync(dst, 0, P, stream)); // (a refused frame may be half written)
            ++r.bad;
        }
        return false;
    };
    for (int c = 0; c < NGpuCodecs; ++c) {
        const int32_t *status = (const int32_t *)sc.lane[c].h_status.get();
        for (size_t i = 0; i < r.lane[c].size(); ++i)
            r.decodedBy[c] += settle(status[i], r.lane[c][i]);
    }
    for (size_t i = 0; i < r.hostPix.size(); ++i) {
        HIPOK(hipMemcpy(out + r.host[i].dst, r.hostPix[i].data(), P, hipMemcpyHostToDevice));
        ok(r.host[i].s, r.host[i].f);
        ++onHost;
    }
}

// One set of files on the device, decoded into one slab: the unit of the device routes that wait for their own upload
// (device training, repack and unpack, each side of verify).  The caller plans ft[i] (planFileTask with `sizer`, `total`)
// and has its pool read them into h_files (readFileTask); then reset, upload, and launch + finish once over all tasks or
// once per range of them; good[s] says whether frame s is in place, `decodedBy` / `hostDecoded` sum over the finishes.
struct FileBatch {
    PinnedBuffer h_files;
    DeviceBuffer d_files, slab;
    DecodeScratch scratch;
    std::unique_ptr<Parser> sizer;
    std::vector<FileTask> ft;
    size_t total = 0, slabBytes = 0;
    FileDescs fd;
    std::vector<uint8_t> good;
    long long decodedBy[NGpuCodecs] = {}, hostDecoded = 0;

    // a slab of `bytes` for frames 0 .. nslots-1, none of them in place yet (its contents are the caller's to clear)
    void reset(size_t nslots, size_t bytes)
    {
        good.assign(nslots, 0);
        slab.grow(bytes);
        slabBytes = bytes;
    }
    // the files to the device, if a decoder took any
    void upload(hipStream_t cs)
    {
        if (std::none_of(ft.begin(), ft.end(), [](const FileTask &t) { return t.onGpu(); }))
            return;
        d_files.grow(total + 16);
        HIPOK(hipMemcpyAsync(d_files.get(), h_files.get(), total + 16, hipMemcpyHostToDevice, cs));
    }
    // the decoders over tasks [i0, i1), frame (s, f) to dstOf(s, f) in the slab; false if none of them is for a decoder
    template <class DstOf>
    bool launch(size_t i0, size_t i1, int W, int H, const DstOf &dstOf, hipStream_t cs)
    {
        fd = FileDescs();
        buildFileDescs(ft.data() + i0, ft.data() + i1, total, fd, dstOf);
        if (!fd.gpuFrames())
            return false;
        launchFileDecode(fd, d_files.get(), W, H, slab.get(), slabBytes, scratch, cs);
        return true;
    }
    // after the stream has been waited for
    void finish(int W, int H, hipStream_t cs)
    {
        finishFileDecode(fd, h_files.get(), scratch, slab.get(), W, H, cs, [&](int s, int) { good[s] = 1; }, hostDecoded);
        for (int c = 0; c < NGpuCodecs; ++c)
            decodedBy[c] += fd.decodedBy[c];
    }
};

} // namespace abub
#endif
