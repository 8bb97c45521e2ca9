// framefiles.hpp -- frames read as FILES for the GPU decoders (abub_png_decode_dev, abub_abf_decode_dev,
// abub_bmp_decode_dev), shared by the batched detect path (runbatch.cpp), device training (devtrain.cpp) and the device
// routes of repack, unpack, verify and survey.  A host thread reads each file; a packed frame ("ABF1") whose header is valid for
// W x H goes to the packed decoder as it is, a PNG has its chunks walked (pngWalk), a BMP its header (bmpWalk, with
// ABUB_GPU_BMP=1; by default BMP files stay with the reading thread); a file none of them takes
// (16-bit, colour or interlaced PNG -- ABUB_GPU_PNG_TYPES=1 and ABUB_GPU_PNG_ADAM7=1 take those too --, compressed BMP, another size)
// gets the host decoder's answer at once, and so does a
// frame a kernel later returns a nonzero status for.  Each decoder is one lane (GpuCodec) of a batch: the placement of its
// frames, its descriptors, its status buffers and its count are indexed by it, and launch and finish loop over the lanes.
// The decoders' width gate, the batch size and the ABUB_GPU_DECODE override are one copy here.  With ABUB_GPU_UNZIP=1 the
// zip layer of a deflated archive entry is inflated on the device between the read and the walk (GpuUnzip, abub_unzip_dev).
//
// FileBatch is the one way a route reads files for the decoders, and the protocol is its calls, in this order:
//   begin()              no tasks; the opt-in knobs (DecodeKnobs) are read from the environment, once per batch
//   plan(s, f, ...)      appends a task: the file's size and place, and its place in the inflate stage; a task the route does
//                        not want read stays Other (its own work) or is set Bad
//   ready()              the pinned buffers
//   read(parser, i, ...) inside the route's pool function, which then deals with what came out (OnGpu, HostDecoded, Bad);
//                        false: the task waits for the inflate, the pool function returns and is called for it once more
//   inflate(..., fn)     the device's inflate, then the pool function `fn` once more over pending() (verify, whose pool
//                        runs over pairs, calls inflateOnDevice on both sides and makes that round itself)
//   upload; launch, finish   over all tasks or per range of them, into the batch's own slab; or describe, launchInto, finishInto
//                        with the caller's output and scratch (RunBatched: two slots share a scratch and own their frames)
// Internal to the host library.
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
#include "decodeknobs.hpp"
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
    // Planned: to be read (FileBatch::plan); OnGpu: read and taken by the decoder `codec`; Other: not a file task (the
    // caller's own work)
    enum { Planned = 0, HostDecoded = 1, Bad = 2, Other = 3, OnGpu = 4 };
    bool onGpu() const { return state == OnGpu; }
    int s = 0, f = 0;
    long long size = 0;
    size_t off = 0; // in the pinned file buffer
    int state = Other;
    GpuCodec codec = GpuPng;
    bool read = false; // the file's bytes are in the buffer (a Bad frame may still have been read)
    // ABUB_GPU_UNZIP=1, an archive entry of method 8 (GpuUnzip below).  ZipPlanned: its compressed bytes are to be read to
    // `coff` of the compressed buffer; ZipRead: they are there, the file waits for the device's inflate (state stays Planned);
    // ZipInflated: the kernel has put the file at `off` of the file buffer, what follows a read is still to do
    enum { ZipNone = 0, ZipPlanned = 1, ZipRead = 2, ZipInflated = 3 };
    int zip = ZipNone;
    size_t coff = 0;
    uint32_t clen = 0, crc = 0;
    PngInfo info;
    BmpInfo bmp;
    std::vector<uint8_t> pix;
};

static_assert(sizeof(abub_zip_entry) == 24, "abub_zip_entry is the 24 bytes include/abub_hip.h states");
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

// a packed frame ("ABF1") whose header is valid for W x H: one for abub_abf_decode_dev
inline bool packedFrameOf(const uint8_t *data, size_t size, int W, int H)
{
    int w = 0, h = 0;
    return cv::abfProbe(data, size, &w, &h) && w == W && h == H;
}

// Does a GPU decoder take the W x H file?  Which one, and what its walk found, into t
inline bool gpuCodecOf(const uint8_t *data, size_t size, int W, int H, FileTask &t, const DecodeKnobs &knobs)
{
    if (packedFrameOf(data, size, W, H)) // (the file goes up as it is; the kernel checks the rest)
        t.codec = GpuPacked;
    else if (pngWalk(data, size, W, H, t.info, knobs.pngTypes, knobs.pngAdam7))
        t.codec = GpuPng;
    else if (knobs.bmp && bmpWalk(data, size, W, H, t.bmp))
        t.codec = GpuBmp;
    else
        return false;
    return true;
}

// The inflate of a batch's deflated archive entries on the device (ABUB_GPU_UNZIP=1), between the pool's read and the walk
// of the files; FileBatch drives it.  An entry of method 8 gets a place in the pinned buffer of compressed bytes when its
// task is planned, the pool reads those bytes instead of the file, and inflate() sends them up: abub_unzip_dev inflates every
// entry to its file's place in d_files, and the files come back into the pinned file buffer (pngWalk needs the chunk
// headers, the fallback decoder the file).  An entry the kernel refuses, for any status, is read by the host as ever
// (ReadImageFile).
struct GpuUnzip {
    long long unzipped = 0; // entries the kernel inflated with status 0, since the batch began
    double device_s = 0;    // wall time of inflate(): the upload of the compressed bytes, the kernels, the copy back, the wait

private:
    friend struct FileBatch;
    PinnedBuffer h_comp, h_status;
    DeviceBuffer d_comp, d_ent, d_status;
    size_t compTotal = 0;
    std::vector<size_t> idx;
    std::vector<abub_zip_entry> ent;

    // t has been planned: is its entry one for the kernel?
    void plan(Parser &sizer, const std::string &ev, const std::string &name, FileTask &t)
    {
        Parser::EntryInfo e;
        if (t.state != FileTask::Planned || !sizer.GetImageEntryInfo(ev, name, e) || e.method != 8 ||
            e.compressedSize >= (1ull << 28) || e.uncompressedSize >= (1ull << 28) || (long long)e.uncompressedSize != t.size ||
            compTotal >= ((size_t)1 << 32) - ((size_t)1 << 29))
            return;
        t.zip = FileTask::ZipPlanned;
        t.coff = compTotal;
        t.clen = (uint32_t)e.compressedSize;
        t.crc = e.crc32;
        compTotal += (((size_t)t.clen + 15) & ~(size_t)15) + 16;
    }
    // tasks first[0 .. n), their files in h_files / d_files (total bytes planned); queued on `stream` and waited for.
    // Afterwards `idx` holds the tasks whose read is to be finished (false: none)
    bool inflate(FileTask *first, size_t n, uint8_t *h_files, DeviceBuffer &d_files, size_t total, hipStream_t stream)
    {
        idx.clear();
        ent.clear();
        for (size_t i = 0; i < n; ++i)
            if (first[i].zip == FileTask::ZipRead) {
                const FileTask &t = first[i];
                idx.push_back(i);
                ent.push_back(abub_zip_entry{(uint32_t)t.coff, t.clen, (uint32_t)t.size, t.crc, (uint64_t)t.off});
            }
        if (idx.empty())
            return false;
        const double t0 = nowMs();
        const size_t ne = ent.size();
        d_comp.grow(compTotal + 16);
        d_files.grow(total + 16);
        d_ent.grow(ne * sizeof(abub_zip_entry));
        d_status.grow(ne * sizeof(int32_t));
        if (h_status.capacity() < ne * sizeof(int32_t))
            h_status.allocate(ne * sizeof(int32_t) + 64);
        HIPOK(hipMemcpyAsync(d_comp.get(), h_comp.get(), compTotal, hipMemcpyHostToDevice, stream));
        HIPOK(hipMemcpyAsync(d_ent.get(), ent.data(), ne * sizeof(abub_zip_entry), hipMemcpyHostToDevice, stream));
        check(abub_unzip_dev(d_comp.get(), compTotal, (const abub_zip_entry *)d_ent.get(), (int)ne, d_files.get(), total + 16,
                             (int32_t *)d_status.get(), stream),
              "abub_unzip_dev");
        HIPOK(hipMemcpyAsync(h_status.get(), d_status.get(), ne * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        // the files back, one copy per run of entries whose files lie next to each other (a file between two of them that is
        // not this stage's is in h_files only); a refused entry's bytes too: the host's read overwrites them
        for (size_t k = 0; k < ne;) {
            const uint64_t from = ent[k].dst;
            uint64_t upto = from + ent[k].ulen;
            for (++k; k < ne && ent[k].dst == ((upto + 15) & ~(uint64_t)15); ++k)
                upto = ent[k].dst + ent[k].ulen;
            HIPOK(hipMemcpyAsync(h_files + from, d_files.get() + from, upto - from, hipMemcpyDeviceToHost, stream));
        }
        HIPOK(hipStreamSynchronize(stream));
        const int32_t *status = (const int32_t *)h_status.get();
        for (size_t k = 0; k < ne; ++k) {
            first[idx[k]].zip = status[k] == 0 ? FileTask::ZipInflated : FileTask::ZipNone;
            unzipped += status[k] == 0;
        }
        device_s += (nowMs() - t0) * 1e-3;
        return true;
    }
};

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
            d.kind = t.info.kind;
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
            // typed frames (ABUB_GPU_PNG_TYPES=1) or interlaced ones (ABUB_GPU_PNG_ADAM7=1) among them: every frame gets the
            // raw bytes of the largest kind present
            bool typed = false, adam7 = false;
            size_t stride = abub_png_raw_stride(W, H);
            for (const abub_png_frame &d : r.png)
                if (d.kind) {
                    typed = true;
                    adam7 |= (d.kind & ABUB_PNG_KIND_ADAM7) != 0;
                    stride = std::max(stride, abub_png_raw_stride_adam7(W, H, d.kind));
                }
            sc.z.grow(r.zbytes);
            sc.raw.grow((size_t)nf * stride);
            sc.segs.grow(r.segs.size() * sizeof(abub_png_seg) + 8);
            HIPOK(hipMemcpyAsync(sc.segs.get(), r.segs.data(), r.segs.size() * sizeof(abub_png_seg), hipMemcpyHostToDevice, stream));
            if (typed)
                check((adam7 ? abub_png_decode_adam7_dev : abub_png_decode_typed_dev)(
                          d_files, r.bytes, (const abub_png_frame *)l.desc.get(), nf, (const abub_png_seg *)sc.segs.get(),
                          (int)r.segs.size(), l.luts.get(), (int)(luts.size() / 256), W, H, sc.z.get(), sc.z.capacity(), sc.raw.get(),
                          sc.raw.capacity(), stride, out, out_bytes, status, stream),
                      adam7 ? "abub_png_decode_adam7_dev" : "abub_png_decode_typed_dev");
            else
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

// One set of files read for the GPU decoders and decoded on the device: the only way a route reads them (the protocol is
// at the top of this file).  `sizer` is the caller's to set, a clone of the parser the files are read through.  good[s] says
// whether frame s is in place in the batch's own slab; `decodedBy` / `hostDecoded` sum over the finishes and are the
// caller's to zero.
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
    DecodeKnobs knobs;
    GpuUnzip unzip; // what the inflate stage counted (unzipped, device_s); the stage itself is driven from here

    // no tasks yet; the knobs are read here, once per batch
    void begin()
    {
        knobs = DecodeKnobs::fromEnv();
        ft.clear();
        total = 0;
        fd = FileDescs();
        unzip.compTotal = 0;
        unzip.unzipped = 0;
        unzip.device_s = 0;
    }
    // The next task, frame (s, f).  Wanted: its file gets its size and its place in the buffer (`total` grows by the file
    // rounded up to 16 bytes; Bad if the parser cannot hand it out) and, where it is a deflated archive entry and the knob is
    // on, a place in the inflate stage.  Not wanted: it stays Other, the caller's own work.  (The reference holds until the
    // next call.)
    FileTask &plan(int s, int f, const std::string &ev, const std::string &name, bool wanted = true)
    {
        ft.emplace_back();
        FileTask &t = ft.back();
        t.s = s;
        t.f = f;
        if (!wanted)
            return t;
        t.size = sizer->GetImageFileSize(ev, name);
        t.state = (t.size > 0 && t.size < ((long long)1 << 30)) ? FileTask::Planned : FileTask::Bad;
        t.off = total;
        if (t.state == FileTask::Planned)
            total += ((size_t)t.size + 15) & ~(size_t)15;
        if (knobs.unzip)
            unzip.plan(*sizer, ev, name, t);
        return t;
    }
    // every task is planned: the buffers the pool reads into
    void ready()
    {
        if (total)
            h_files.grow(total + 16);
        if (unzip.compTotal)
            unzip.h_comp.grow(unzip.compTotal + 16);
    }
    // On a pool thread: task i's file into h_files + its offset, walked for the W x H GPU decoders, else decoded here.  A task
    // planned for the device's inflate only has its compressed bytes read and stays Planned: false, it is to be read once more
    // after the inflate, which does the rest (the file is in place: ZipInflated) or all of it (ZipNone).
    bool read(Parser &p, size_t i, const std::string &ev, const std::string &name, int W, int H)
    {
        FileTask &t = ft[i];
        if (t.state != FileTask::Planned)
            return true;
        uint8_t *dst = h_files.get() + t.off;
        long long got = -1;
        if (t.zip == FileTask::ZipPlanned) {
            try {
                got = p.ReadImageEntryRaw(ev, name, unzip.h_comp.get() + t.coff, t.clen);
            } catch (...) {
                got = -1;
            }
            t.zip = got == (long long)t.clen ? FileTask::ZipRead : FileTask::ZipNone;
        }
        if (t.zip == FileTask::ZipRead)
            return false;
        if (t.zip == FileTask::ZipInflated)
            got = t.size;
        else
            try {
                got = p.ReadImageFile(ev, name, dst, (size_t)t.size);
            } catch (...) {
                got = -1;
            }
        t.read = got == t.size;
        try {
            if (!t.read)
                t.state = FileTask::Bad;
            else if (gpuCodecOf(dst, (size_t)t.size, W, H, t, knobs))
                t.state = FileTask::OnGpu;
            else { // not a file for the GPU decoders (16-bit, colour, interlaced, another size): the host decoder's answer
                t.pix.resize((size_t)W * H);
                t.state = cv::imdecodeInto(dst, (size_t)t.size, t.pix.data(), W, H) ? FileTask::HostDecoded : FileTask::Bad;
            }
        } catch (...) { // (an allocation that fails inside a pool thread must not end the batch)
            t.state = FileTask::Bad;
        }
        return true;
    }
    // After the pool: the waiting tasks' entries inflated on the device, queued on `cs` and waited for; false if none waited
    bool inflateOnDevice(hipStream_t cs) { return unzip.inflate(ft.data(), ft.size(), h_files.get(), d_files, total, cs); }
    // the tasks that waited for the last inflateOnDevice, in ascending order: each is to be read once more
    const std::vector<size_t> &pending() const { return unzip.idx; }
    // inflateOnDevice, then `readOne` -- the caller's pool function -- once more over the pending tasks
    template <class Fn>
    void inflate(Parser *parser, int nthreads, hipStream_t cs, const Fn &readOne)
    {
        if (inflateOnDevice(cs))
            forEachTask(parser, nthreads, pending().size(), [&](Parser &p, size_t k) { readOne(p, pending()[k]); });
    }
    // a slab of `bytes` for frames 0 .. nslots-1, none of them in place yet (its contents are the caller's to clear)
    void reset(size_t nslots, size_t bytes)
    {
        good.assign(nslots, 0);
        slab.grow(bytes);
        slabBytes = bytes;
    }
    // the files to the device, if a decoder took any (false: none did, nothing was queued)
    bool upload(hipStream_t cs)
    {
        if (std::none_of(ft.begin(), ft.end(), [](const FileTask &t) { return t.onGpu(); }))
            return false;
        d_files.grow(total + 16);
        HIPOK(hipMemcpyAsync(d_files.get(), h_files.get(), total + 16, hipMemcpyHostToDevice, cs));
        return true;
    }
    // fd: the descriptors of tasks [i0, i1), frame (s, f) to byte dstOf(s, f) of the output
    template <class DstOf>
    void describe(size_t i0, size_t i1, const DstOf &dstOf)
    {
        fd = FileDescs();
        buildFileDescs(ft.data() + i0, ft.data() + i1, total, fd, dstOf);
    }
    // the decoders over the described tasks into `out` (out_bytes) with the scratch `sc`, queued on `cs`; false if none of
    // the tasks is for a decoder
    bool launchInto(int W, int H, uint8_t *out, size_t out_bytes, DecodeScratch &sc, hipStream_t cs)
    {
        if (!fd.gpuFrames())
            return false;
        launchFileDecode(fd, d_files.get(), W, H, out, out_bytes, sc, cs);
        return true;
    }
    // after the stream has been waited for: the refused frames and the reading threads' own into `out`; ok(s, f) for every
    // frame that is in place
    template <class Ok>
    void finishInto(int W, int H, uint8_t *out, const DecodeScratch &sc, hipStream_t cs, const Ok &ok)
    {
        finishFileDecode(fd, h_files.get(), sc, out, W, H, cs, ok, hostDecoded);
        for (int c = 0; c < NGpuCodecs; ++c)
            decodedBy[c] += fd.decodedBy[c];
    }
    // the same two into the batch's own slab with its own scratch, over tasks [i0, i1)
    template <class DstOf>
    bool launch(size_t i0, size_t i1, int W, int H, const DstOf &dstOf, hipStream_t cs)
    {
        describe(i0, i1, dstOf);
        return launchInto(W, H, slab.get(), slabBytes, scratch, cs);
    }
    void finish(int W, int H, hipStream_t cs)
    {
        finishInto(W, H, slab.get(), scratch, cs, [&](int s, int) { good[s] = 1; });
    }
};

} // namespace abub
#endif
