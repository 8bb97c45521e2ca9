// framefiles.hpp -- frames read as FILES for the GPU decoders (abub_png_decode_dev, abub_abf_decode_dev,
// abub_bmp_decode_dev), shared by the batched detect path (runbatch.cpp), device training (devtrain.cpp) and the device
// routes of repack, unpack and verify.  A host thread reads each file; a packed frame ("ABF1") whose header is valid for
// W x H goes to the packed decoder as it is, a PNG has its chunks walked (pngWalk), a BMP its header (bmpWalk, with
// ABUB_GPU_BMP=1; by default BMP files stay with the reading thread); a file none of them takes
// (16-bit, colour or interlaced PNG, compressed BMP, another size) gets the host decoder's answer at once, and so does a
// frame a kernel later returns a nonzero status for.  Internal to the host library.
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

// One frame to be read: where it goes is decided by the caller (s, f); `state` says what became of it
struct FileTask {
    // Gpu: planned for / taken by the PNG decoder, GpuPacked: taken by the packed decoder, GpuBmp: by the BMP decoder;
    // Other: not a file task (the caller's own work)
    enum { Gpu = 0, HostDecoded = 1, Bad = 2, Other = 3, GpuPacked = 4, GpuBmp = 5 };
    bool onGpu() const { return state == Gpu || state == GpuPacked || state == GpuBmp; }
    int s = 0, f = 0;
    long long size = 0;
    size_t off = 0; // in the pinned file buffer
    int state = Other;
    bool read = false; // the file's bytes are in the buffer (a Bad frame may still have been read)
    PngInfo info;
    BmpInfo bmp;
    std::vector<uint8_t> pix;
};

static_assert(sizeof(abub_bmp_frame) == 32, "abub_bmp_frame is the 32 bytes include/abub_hip.h states");

// The descriptors of one decode launch, and the frames a reading thread decoded itself
struct FileDescs {
    size_t bytes = 0, zbytes = 0;           // of the files; of the decoder's stream buffer
    std::vector<abub_png_frame> desc;       // the PNG frames the GPU decodes
    std::vector<std::pair<int, int>> where; // (s, f) of desc[i]
    std::vector<uint32_t> fileOff, fileLen; // of desc[i] inside the file buffer
    std::vector<abub_png_seg> segs;
    std::vector<uint8_t> luts;              // 256 bytes each
    std::vector<abub_abf_frame> abf;        // the packed frames the GPU decodes (file offset, length, destination)
    std::vector<std::pair<int, int>> abfWhere;
    long long unpacked = 0;                 // of them, decoded by the kernel (finishFileDecode)
    std::vector<abub_bmp_frame> bmp;        // the BMP frames the GPU decodes
    std::vector<std::pair<int, int>> bmpWhere;
    std::vector<uint8_t> bmpLuts;           // 256 bytes each
    long long bmpDecoded = 0;               // of them, decoded by the kernel (finishFileDecode)
    size_t gpuFrames() const { return desc.size() + abf.size() + bmp.size(); }
    std::vector<std::vector<uint8_t>> hostPix;
    std::vector<std::pair<int, int>> hostWhere;
    long long bad = 0;
};

// The file's size and its place in the buffer (`total` grows by the file rounded up to 16 bytes); Bad if the parser
// cannot hand it out
inline void planFileTask(Parser &sizer, const std::string &ev, const std::string &name, FileTask &t, size_t &total)
{
    t.size = sizer.GetImageFileSize(ev, name);
    t.state = (t.size > 0 && t.size < ((long long)1 << 30)) ? FileTask::Gpu : FileTask::Bad;
    t.off = total;
    if (t.state == FileTask::Gpu)
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

// On a pool thread: the file into files + t.off, walked for the W x H GPU decoder, else decoded here
inline void readFileTask(Parser &p, const std::string &ev, const std::string &name, FileTask &t, uint8_t *files, int W, int H)
{
    if (t.state != FileTask::Gpu)
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
        if (packedFrameOf(dst, (size_t)t.size, W, H)) {
            t.state = FileTask::GpuPacked; // (the file goes up as it is; the kernel checks the rest)
            return;
        }
        if (pngWalk(dst, (size_t)t.size, W, H, t.info))
            return;
        if (gpuBmpEnabled() && bmpWalk(dst, (size_t)t.size, W, H, t.bmp)) {
            t.state = FileTask::GpuBmp;
            return;
        }
        // not a file for the GPU decoders (16-bit, colour, interlaced, another size): the host decoder's answer
        t.pix.resize((size_t)W * H);
        t.state = cv::imdecodeInto(dst, (size_t)t.size, t.pix.data(), W, H) ? FileTask::HostDecoded : FileTask::Bad;
    } catch (...) { // (an allocation that fails inside a pool thread must not end the batch)
        t.state = FileTask::Bad;
    }
}

// The descriptors of the tasks' Gpu frames, in task order; dstOf(s, f): byte offset of the decoded frame from the output
// (tasks [first, last); the files of every task are in one buffer of totalFileBytes)
template <class DstOf>
void buildFileDescs(FileTask *first, FileTask *last, size_t totalFileBytes, FileDescs &r, const DstOf &dstOf)
{
    r.bytes = totalFileBytes + 16;
    size_t zoff = 0;
    for (FileTask *tp = first; tp != last; ++tp) {
        FileTask &t = *tp;
        if (t.state == FileTask::Other)
            continue;
        if (t.state == FileTask::Bad) {
            ++r.bad;
            continue;
        }
        if (t.state == FileTask::HostDecoded) {
            r.hostPix.push_back(std::move(t.pix));
            r.hostWhere.emplace_back(t.s, t.f);
            continue;
        }
        if (t.state == FileTask::GpuPacked) {
            r.abf.push_back(abub_abf_frame{(uint32_t)t.off, (uint32_t)t.size, dstOf(t.s, t.f)});
            r.abfWhere.emplace_back(t.s, t.f);
            continue;
        }
        if (t.state == FileTask::GpuBmp) {
            abub_bmp_frame b;
            b.off = (uint32_t)t.off;
            b.len = (uint32_t)t.size;
            b.data_off = t.bmp.dataOff;
            b.stride = t.bmp.stride;
            b.bpp = (uint16_t)t.bmp.bpp;
            b.flags = t.bmp.topDown ? 1 : 0;
            b.lut = 0xffffffffu;
            b.dst = dstOf(t.s, t.f);
            if (t.bmp.bpp <= 8 && !t.bmp.identity) { // (as the PNG tables below: the frames of a run share one)
                size_t nl = r.bmpLuts.size() / 256, l = 0;
                for (; l < nl; ++l)
                    if (!memcmp(&r.bmpLuts[l * 256], t.bmp.lut, 256))
                        break;
                if (l == nl)
                    r.bmpLuts.insert(r.bmpLuts.end(), t.bmp.lut, t.bmp.lut + 256);
                b.lut = (uint32_t)l;
            }
            r.bmp.push_back(b);
            r.bmpWhere.emplace_back(t.s, t.f);
            continue;
        }
        abub_png_frame d;
        d.seg_begin = (uint32_t)r.segs.size();
        d.seg_count = (uint32_t)t.info.segs.size();
        d.zoff = (uint32_t)zoff;
        d.zlen = (uint32_t)t.info.zlen;
        d.lut = 0xffffffffu;
        d.reserved = 0;
        d.dst = dstOf(t.s, t.f);
        if (t.info.palette) { // (the frames of a run share their palette: look for the table among those already kept)
            size_t nl = r.luts.size() / 256, l = 0;
            for (; l < nl; ++l)
                if (!memcmp(&r.luts[l * 256], t.info.lut, 256))
                    break;
            if (l == nl)
                r.luts.insert(r.luts.end(), t.info.lut, t.info.lut + 256);
            d.lut = (uint32_t)l;
        }
        for (const abub_png_seg &sg : t.info.segs)
            r.segs.push_back(abub_png_seg{(uint32_t)(t.off + sg.off), sg.len});
        zoff += (((size_t)d.zlen + 15) & ~(size_t)15) + 16;
        r.desc.push_back(d);
        r.where.emplace_back(t.s, t.f);
        r.fileOff.push_back((uint32_t)t.off);
        r.fileLen.push_back((uint32_t)t.size);
    }
    r.zbytes = zoff + 16;
    if (r.bytes >= ((size_t)1 << 32) || r.zbytes >= ((size_t)1 << 32))
        throw std::runtime_error("a batch of more than 4 GB of files (lower the batch size)");
}

// The decoders' scratch, kept from one launch to the next
struct PngScratch {
    DeviceBuffer z, raw, luts, desc, segs, status;
    PinnedBuffer h_status;
    DeviceBuffer abfDesc, abfStatus; // the packed decoder needs no more than its descriptors and statuses
    PinnedBuffer h_abfStatus;
    DeviceBuffer bmpDesc, bmpLuts, bmpStatus; // the BMP decoder: descriptors, tables, statuses
    PinnedBuffer h_bmpStatus;
};

// One abub_abf_decode_dev launch over r's packed frames, as launchPngDecode below
inline void launchAbfDecode(const FileDescs &r, const uint8_t *d_files, int W, int H, uint8_t *out, size_t out_bytes,
                            PngScratch &sc, hipStream_t stream)
{
    const int nf = (int)r.abf.size();
    if (!nf)
        return;
    sc.abfDesc.grow((size_t)nf * sizeof(abub_abf_frame));
    sc.abfStatus.grow((size_t)nf * sizeof(int32_t));
    if (sc.h_abfStatus.capacity() < (size_t)nf * sizeof(int32_t))
        sc.h_abfStatus.allocate((size_t)nf * sizeof(int32_t) + 64);
    HIPOK(hipMemcpyAsync(sc.abfDesc.get(), r.abf.data(), (size_t)nf * sizeof(abub_abf_frame), hipMemcpyHostToDevice, stream));
    check(abub_abf_decode_dev(d_files, r.bytes, (const abub_abf_frame *)sc.abfDesc.get(), nf, W, H, out, out_bytes,
                              (int32_t *)sc.abfStatus.get(), stream),
          "abub_abf_decode_dev");
    HIPOK(hipMemcpyAsync(sc.h_abfStatus.get(), sc.abfStatus.get(), (size_t)nf * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
}

// One abub_bmp_decode_dev launch over r's BMP frames, likewise
inline void launchBmpDecode(const FileDescs &r, const uint8_t *d_files, int W, int H, uint8_t *out, size_t out_bytes,
                            PngScratch &sc, hipStream_t stream)
{
    const int nf = (int)r.bmp.size();
    if (!nf)
        return;
    sc.bmpDesc.grow((size_t)nf * sizeof(abub_bmp_frame));
    sc.bmpStatus.grow((size_t)nf * sizeof(int32_t));
    sc.bmpLuts.grow(r.bmpLuts.size() + 256);
    if (sc.h_bmpStatus.capacity() < (size_t)nf * sizeof(int32_t))
        sc.h_bmpStatus.allocate((size_t)nf * sizeof(int32_t) + 64);
    HIPOK(hipMemcpyAsync(sc.bmpDesc.get(), r.bmp.data(), (size_t)nf * sizeof(abub_bmp_frame), hipMemcpyHostToDevice, stream));
    if (!r.bmpLuts.empty())
        HIPOK(hipMemcpyAsync(sc.bmpLuts.get(), r.bmpLuts.data(), r.bmpLuts.size(), hipMemcpyHostToDevice, stream));
    check(abub_bmp_decode_dev(d_files, r.bytes, (const abub_bmp_frame *)sc.bmpDesc.get(), nf, sc.bmpLuts.get(),
                              (int)(r.bmpLuts.size() / 256), W, H, out, out_bytes, (int32_t *)sc.bmpStatus.get(), stream),
          "abub_bmp_decode_dev");
    HIPOK(hipMemcpyAsync(sc.h_bmpStatus.get(), sc.bmpStatus.get(), (size_t)nf * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
}

// One launch of each decoder that has frames in r, into `out` (out_bytes), the statuses copied back into sc.h_status /
// sc.h_abfStatus / sc.h_bmpStatus; all queued on `stream` (so they stay behind whatever the caller queued there before, the
// clear of the batch's slab for one), not waited for.  The files are already in d_files.
inline void launchPngDecode(const FileDescs &r, const uint8_t *d_files, int W, int H, uint8_t *out, size_t out_bytes,
                            PngScratch &sc, hipStream_t stream);
inline void launchFileDecode(const FileDescs &r, const uint8_t *d_files, int W, int H, uint8_t *out, size_t out_bytes,
                             PngScratch &sc, hipStream_t stream)
{
    launchPngDecode(r, d_files, W, H, out, out_bytes, sc, stream);
    launchAbfDecode(r, d_files, W, H, out, out_bytes, sc, stream);
    launchBmpDecode(r, d_files, W, H, out, out_bytes, sc, stream);
}
inline void launchPngDecode(const FileDescs &r, const uint8_t *d_files, int W, int H, uint8_t *out, size_t out_bytes,
                            PngScratch &sc, hipStream_t stream)
{
    const int nf = (int)r.desc.size();
    if (!nf)
        return;
    sc.z.grow(r.zbytes);
    sc.raw.grow((size_t)nf * abub_png_raw_stride(W, H));
    sc.desc.grow((size_t)nf * sizeof(abub_png_frame));
    sc.segs.grow(r.segs.size() * sizeof(abub_png_seg) + 8);
    sc.luts.grow(r.luts.size() + 256);
    sc.status.grow((size_t)nf * sizeof(int32_t));
    if (sc.h_status.capacity() < (size_t)nf * sizeof(int32_t))
        sc.h_status.allocate((size_t)nf * sizeof(int32_t) + 64);
    HIPOK(hipMemcpyAsync(sc.desc.get(), r.desc.data(), (size_t)nf * sizeof(abub_png_frame), hipMemcpyHostToDevice, stream));
    HIPOK(hipMemcpyAsync(sc.segs.get(), r.segs.data(), r.segs.size() * sizeof(abub_png_seg), hipMemcpyHostToDevice, stream));
    if (!r.luts.empty())
        HIPOK(hipMemcpyAsync(sc.luts.get(), r.luts.data(), r.luts.size(), hipMemcpyHostToDevice, stream));
    check(abub_png_decode_dev(d_files, r.bytes, (const abub_png_frame *)sc.desc.get(), nf, (const abub_png_seg *)sc.segs.get(),
                              (int)r.segs.size(), sc.luts.get(), (int)(r.luts.size() / 256), W, H, sc.z.get(), sc.z.capacity(),
                              sc.raw.get(), sc.raw.capacity(), out, out_bytes, (int32_t *)sc.status.get(), stream),
          "abub_png_decode_dev");
    HIPOK(hipMemcpyAsync(sc.h_status.get(), sc.status.get(), (size_t)nf * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
}

// After the launches above have been waited for: a frame the kernels refused takes the host decoder's answer (the same
// image, or the same failure), and the reading threads' own frames are uploaded.  ok(s, f) is called for every frame that
// is in place; hostOffset(s, f): byte offset of the frame from `out`.  Packed frames the kernel decoded count in onGpu
// and in r.unpacked, BMP frames the kernel decoded in onGpu and in r.bmpDecoded.
template <class HostOffset, class Ok>
void finishFileDecode(FileDescs &r, const uint8_t *h_files, const PngScratch &sc, uint8_t *out, int W, int H,
                      hipStream_t stream, const HostOffset &hostOffset, const Ok &ok, long long &onGpu, long long &onHost)
{
    const size_t P = (size_t)W * H;
    std::vector<uint8_t> pix;
    // frame (s, f) of file [off, off + len) whose decoder answered `status`
    auto settle = [&](int32_t status, std::pair<int, int> w, uint64_t dstOff, uint32_t off, uint32_t len) {
        uint8_t *dst = out + dstOff;
        if (status == 0) {
            ok(w.first, w.second);
            ++onGpu;
            return true;
        }
        pix.resize(P);
        if (cv::imdecodeInto(h_files + off, len, pix.data(), W, H)) {
            HIPOK(hipMemcpy(dst, pix.data(), P, hipMemcpyHostToDevice));
            ok(w.first, w.second);
            ++onHost;
        } else {
            HIPOK(hipMemsetAsync(dst, 0, P, stream)); // (a refused frame may be half written)
            ++r.bad;
        }
        return false;
    };
    const int32_t *status = (const int32_t *)sc.h_status.get(), *abfStatus = (const int32_t *)sc.h_abfStatus.get();
    const int32_t *bmpStatus = (const int32_t *)sc.h_bmpStatus.get();
    for (size_t i = 0; i < r.desc.size(); ++i)
        settle(status[i], r.where[i], r.desc[i].dst, r.fileOff[i], r.fileLen[i]);
    for (size_t i = 0; i < r.abf.size(); ++i)
        r.unpacked += settle(abfStatus[i], r.abfWhere[i], r.abf[i].dst, r.abf[i].off, r.abf[i].len);
    for (size_t i = 0; i < r.bmp.size(); ++i)
        r.bmpDecoded += settle(bmpStatus[i], r.bmpWhere[i], r.bmp[i].dst, r.bmp[i].off, r.bmp[i].len);
    for (size_t i = 0; i < r.hostPix.size(); ++i) {
        HIPOK(hipMemcpy(out + hostOffset(r.hostWhere[i].first, r.hostWhere[i].second), r.hostPix[i].data(), P,
                        hipMemcpyHostToDevice));
        ok(r.hostWhere[i].first, r.hostWhere[i].second);
        ++onHost;
    }
}

} // namespace abub
#endif
