// runbatch.cpp -- RunBatched (runbatch.hpp): a run from a Parser through the batched pipeline.  Replaces the detect loop of
// the reference's main program (AutoBubStart3.cpp:338-388): same per-(event, camera) analyses, same output blocks in the
// same order, but the frames of a whole batch of events are decoded once (the reference decodes a frame up to three
// times: main loop, look-ahead, localizer), uploaded once and processed with a handful of launches.
//
// A batch of G events has a GPU share, its first Ggpu events, whose files host threads read into one pinned buffer for
// abub_png_decode_dev, and a host share, the others, which host threads decode straight into a pinned frame slab.
// Ggpu = 0 is the host-decode mode.  A look-ahead thread reads batch b + 1 while batch b is on the GPU.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "AlgorithmTraining/Trainer.hpp"
#include "ParseFolder/Parser.hpp"
#include "PICOFormatWriter/PICOFormatWriterV4.hpp"
#include "devctx.hpp"
#include "holders.hpp"
#include "pipeline.hpp"
#include "pngwalk.hpp"
#include "runbatch.hpp"

namespace abub {
namespace {

// fn(parser, i) for every i < n on up to `nthreads` threads, each with its own clone of `parser`.  The first exception is
// re-thrown once every thread has been joined (the others stop at their next task).
template <class Fn>
void forEachTask(Parser *parser, int nthreads, size_t n, const Fn &fn)
{
    std::atomic<size_t> next{0};
    std::mutex errMu;
    std::exception_ptr err;
    std::vector<std::thread> th;
    for (int t = 0; t < std::max(1, (int)std::min<size_t>(nthreads, n)); ++t)
        th.emplace_back([&]() {
            try {
                std::unique_ptr<Parser> p(parser->clone());
                for (size_t i; (i = next.fetch_add(1)) < n;)
                    fn(*p, i);
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

// Frame f of stack m decoded by the host into its slot (W x H bytes at dst), or the slot zeroed: a frame that does not
// decode (missing, undecodable, of another size) would otherwise keep the bytes of an earlier batch or half a decode.
// Results never use them, but dense garbage costs the trigger search's kernels time that varies from run to run.
bool decodeFrame(Parser &p, StackMeta &m, int f, uint8_t *dst, int W, int H)
{
    int rc = -1;
    try {
        rc = p.GetImageInto(m.eventID, m.names[f], dst, W, H); // decoded in place, no per-frame allocation
    } catch (...) {
        rc = -1;
    }
    if (rc != 1) { // (anything but 1 = undecodable, like EventOnDevice)
        std::memset(dst, 0, (size_t)W * H);
        return false;
    }
    m.ok[f] = 1;
    return true;
}

// One of a worker's two batch buffers, and what the reading threads found out about the batch that is in it
struct Slot {
    PinnedBuffer h_frames;     // the host share's frames
    DeviceBuffer d_frames;     // the whole batch, [G][C][Fmax][H][W]
    PinnedBuffer h_files;      // the GPU share's files, each at a 16-byte boundary ...
    DeviceBuffer d_files;      // ... uploaded by the reading thread: the copy runs beside the GPU work of the batch before
    std::exception_ptr err;    // of the look-ahead thread that read the batch
    struct Read {
        std::vector<StackMeta> meta;
        size_t bytes = 0, zbytes = 0;           // of the files; of the decoder's stream buffer
        std::vector<abub_png_frame> desc;       // the frames the GPU decodes
        std::vector<std::pair<int, int>> where; // (stack, frame) of desc[i]
        std::vector<uint32_t> fileOff, fileLen; // of desc[i] inside h_files
        std::vector<abub_png_seg> segs;
        std::vector<uint8_t> luts;              // 256 bytes each
        // frames of the GPU share a reading thread decoded (files the GPU path does not take): pixels + (stack, frame)
        std::vector<std::vector<uint8_t>> hostPix;
        std::vector<std::pair<int, int>> hostWhere;
        double ms = 0;
        long long bad = 0, hostGood = 0;
    } r;
};

} // namespace

int RunBatched(Parser *parser, const std::vector<std::string> &EventList, const std::vector<Trainer *> &Trainers,
               int numCams, const std::string &out_dir, const std::string &run_number, int frameOffset,
               const BatchedRunOptions &opt, BatchedRunStats *stats, std::string *why)
{
    const double tAll = nowMs();
    auto refuse = [&](const char *msg) {
        if (why)
            *why = msg;
        return 1;
    };
    const int C = numCams;
    if (C <= 0 || (int)Trainers.size() != C)
        return refuse("one trainer per camera expected");
    const int W = Trainers[0]->TrainedAvgImage.cols, H = Trainers[0]->TrainedAvgImage.rows;
    if (W <= 0 || H <= 0)
        return refuse("untrained model");
    for (Trainer *t : Trainers)
        if (t->TrainedAvgImage.cols != W || t->TrainedAvgImage.rows != H || t->TrainedSigmaImage.cols != W ||
            t->TrainedSigmaImage.rows != H)
            return refuse("cameras with different image sizes");
    const size_t P = (size_t)W * H;
    std::vector<int> mine; // indices into EventList handled by this process
    for (int i = 0; i < (int)EventList.size(); ++i)
        if (opt.shardWorld <= 1 || i % opt.shardWorld == opt.shardRank)
            mine.push_back(i);
    BatchedRunStats st;
    st.W = W;
    st.H = H;
    st.events = (int)mine.size();
    if (mine.empty()) {
        if (stats)
            *stats = st;
        return 0;
    }
    const int ndec = std::max(1, opt.decodeThreads);

    // ---- frame lists of every (event, camera), in the Parser's (lexicographic) order -------------------------------
    double t0 = nowMs();
    std::vector<std::vector<std::vector<std::string>>> lists(mine.size(), std::vector<std::vector<std::string>>(C));
    forEachTask(parser, ndec, mine.size(), [&](Parser &p, size_t k) {
        for (int c = 0; c < C; ++c)
            p.ParseAndSortFramesInFolder(EventList[mine[k]], c, lists[k][c]);
    });
    int Fmax = 1;
    for (auto &ev : lists)
        for (auto &l : ev)
            Fmax = std::max(Fmax, (int)l.size());
    st.list_s = (nowMs() - t0) * 1e-3;
    if (Fmax > 1024)
        return refuse("more than 1024 frames in one stack");
    st.Fmax = Fmax;
    const size_t perEvent = (size_t)C * Fmax * P;
    int G = (int)std::max<size_t>(1, std::min<size_t>(opt.batchBytes / perEvent, mine.size()));
    // A run that would fit a few batches is cut into at least twelve per GPU (of at least four events): decoding batch
    // b + 1 then overlaps the GPU work of batch b, and the two pinned slabs stay small -- page-locking 2.6 GB takes about
    // as long as decoding it on 16 cores (measured: 1.0 s of a 2.8 s run of 96 events with batches of 24).
    {
        const int ng = std::max(1, opt.ngpus);
        const int want = std::max(4, (int)((mine.size() + (size_t)12 * ng - 1) / ((size_t)12 * ng)));
        G = std::max(1, std::min(G, want));
    }
    G = std::min(G, 512);
    // ---- where the frames are decoded --------------------------------------------------------------------------------
    // On the GPU (abub_png.hip) when the parser hands out the files as they are stored and the first frame is a PNG the
    // kernels take; a host thread still reads each file and walks its chunks, and decodes the odd frame the GPU path
    // refuses.  Otherwise host threads decode every frame (GetImageInto).
    bool devDecode = opt.gpuDecode != 0 && (W & 3) == 0 && W >= 4 && W <= 2048;
    if (const char *e = getenv("ABUB_GPU_DECODE"))
        devDecode = devDecode && atoi(e) != 0;
    if (devDecode) {
        devDecode = false;
        for (size_t k = 0; k < lists.size() && !devDecode; ++k)
            for (int c = 0; c < C && !devDecode; ++c)
                if (!lists[k][c].empty()) {
                    std::unique_ptr<Parser> p(parser->clone());
                    const long long sz = p->GetImageFileSize(EventList[mine[k]], lists[k][c][0]);
                    if (sz > 0 && sz < ((long long)1 << 30)) {
                        std::vector<unsigned char> buf((size_t)sz);
                        PngInfo info;
                        devDecode = p->ReadImageFile(EventList[mine[k]], lists[k][c][0], buf.data(), buf.size()) == sz &&
                                    pngWalk(buf.data(), buf.size(), W, H, info);
                    }
                    k = lists.size(); // (one probe decides)
                    break;
                }
    }
    int Ggpu = 0; // the first Ggpu events of a batch are decoded on the GPU, the others by the host threads
    if (devDecode) {
        // The inflate kernel runs four streams per CU at a time (1024 on an MI355X) and a batch takes as long as its longest
        // stream: batches carry that many frames for the GPU, not one more.
        int ncu = 256;
        {
            int dev0 = opt.firstDevice, v = 0, nd = 0;
            if (hipGetDeviceCount(&nd) == hipSuccess && nd > 0 &&
                hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev0 % nd) == hipSuccess && v > 0)
                ncu = v;
        }
        const int perEv = std::max(1, C * Fmax);
        const int capG = (int)std::max<size_t>(1, opt.batchBytes / perEvent);
        Ggpu = std::max(1, std::min((4 * ncu) / perEv, std::min(capG, (int)mine.size())));
        if (const char *e = getenv("ABUB_GPU_DECODE_EVENTS")) // (tests: a small GPU share)
            Ggpu = std::max(1, std::min(Ggpu, atoi(e)));
        // The host threads can decode the frames of a few more events per batch while the GPU works (they only READ the
        // files otherwise): ABUB_HOST_DECODE_EVENTS=n.  Off by default -- measured on a 96-event run (16 threads): 8.1 k
        // frames/s without, 7.5 k with n = 4, 7.3 k with n = 8: the first batch's host share is not overlapped with
        // anything, the GPU decode slows by 10 - 15 % beside 16 busy cores, and a run of eight batches never makes that up.
        int Ghost = 0;
        if (const char *e = getenv("ABUB_HOST_DECODE_EVENTS"))
            Ghost = std::max(0, atoi(e));
        Ghost = std::max(0, std::min(Ghost, std::min(capG, (int)mine.size()) - Ggpu));
        G = Ggpu + Ghost;
    }
    const int nb = ((int)mine.size() + G - 1) / G;
    int ndev = 0;
    HIPOK(hipGetDeviceCount(&ndev));
    if (ndev <= 0)
        throw std::runtime_error("RunBatched: no GPU");
    const int ngpus = std::max(1, std::min(opt.ngpus, nb));
    st.gpus = ngpus;
    st.batches = nb;
    st.eventsPerBatch = G;

    std::mutex turnMu;
    std::condition_variable turnCv;
    int turn = 0;       // next batch to be written (output is in event order, AutoBubStart3.cpp:380-383)
    bool failed = false;
    std::vector<std::string> errors(ngpus);
    std::mutex statMu;

    // ---- batch b read into `sl` (on the look-ahead thread, with the worker's device current) -----------------------------
    auto readBatch = [&](int b, Slot &sl, int nthreads, int dev, Stream &upStream) {
        const double td = nowMs();
        (void)hipSetDevice(dev);
        const int e0 = b * G, nEv = std::min(G, (int)mine.size() - e0);
        Slot::Read &r = sl.r;
        r = Slot::Read();
        r.meta.assign((size_t)G * C, StackMeta());
        struct Task {
            int s, f;
            long long size = 0;
            size_t off = 0;
            int state; // 0 = a file for the GPU, 1 = decoded here, 2 = missing / undecodable, 3 = host share
            PngInfo info;
            std::vector<uint8_t> pix;
        };
        std::vector<Task> tasks; // (in stack order: the GPU's files are read first, its work can start before the host's is done)
        std::unique_ptr<Parser> sizer(Ggpu ? parser->clone() : nullptr);
        size_t total = 0;
        for (int k = 0; k < G; ++k)
            for (int c = 0; c < C; ++c) {
                StackMeta &m = r.meta[(size_t)k * C + c];
                if (k >= nEv) {
                    m.eventID = "_pad" + std::to_string(k); // filler of the last batch: no frames -> -9, never written
                    continue;
                }
                m.eventID = EventList[mine[e0 + k]];
                m.names = lists[e0 + k][c];
                m.ok.assign(m.names.size(), 0);
                for (int f = 0; f < (int)m.names.size(); ++f) {
                    Task t;
                    t.s = k * C + c;
                    t.f = f;
                    t.state = 3;
                    if (k < Ggpu) {
                        t.size = sizer->GetImageFileSize(m.eventID, m.names[f]);
                        t.state = (t.size > 0 && t.size < ((long long)1 << 30)) ? 0 : 2;
                        t.off = total;
                        if (t.state == 0)
                            total += ((size_t)t.size + 15) & ~(size_t)15;
                    }
                    tasks.push_back(std::move(t));
                }
            }
        r.bytes = total + 16;
        if (Ggpu)
            sl.h_files.grow(r.bytes);
        std::atomic<long long> hostGood{0}, hostBad{0};
        forEachTask(parser, nthreads, tasks.size(), [&](Parser &p, size_t i) {
            Task &t = tasks[i];
            if (t.state == 3) { // the host share: straight into the pinned slab
                uint8_t *dst = sl.h_frames.get() + ((size_t)(t.s - Ggpu * C) * Fmax + t.f) * P;
                ++(decodeFrame(p, r.meta[t.s], t.f, dst, W, H) ? hostGood : hostBad);
                return;
            }
            if (t.state != 0)
                return;
            uint8_t *dst = sl.h_files.get() + t.off;
            long long got = -1;
            try {
                got = p.ReadImageFile(r.meta[t.s].eventID, r.meta[t.s].names[t.f], dst, (size_t)t.size);
            } catch (...) {
                got = -1;
            }
            if (got != t.size) {
                t.state = 2;
                return;
            }
            try {
                if (!pngWalk(dst, (size_t)t.size, W, H, t.info)) {
                    // not a file for the GPU decoder (BMP, 16-bit, colour, interlaced, another size): the host decoder's answer
                    t.pix.resize(P);
                    t.state = cv::imdecodeInto(dst, (size_t)t.size, t.pix.data(), W, H) ? 1 : 2;
                }
            } catch (...) { // (an allocation that fails inside a pool thread must not end the batch)
                t.state = 2;
            }
        });
        r.bad = hostBad;
        r.hostGood = hostGood;
        size_t zoff = 0;
        for (Task &t : tasks) {
            if (t.state == 3)
                continue;
            if (t.state == 2) {
                ++r.bad;
                continue;
            }
            if (t.state == 1) {
                r.hostPix.push_back(std::move(t.pix));
                r.hostWhere.emplace_back(t.s, t.f);
                continue;
            }
            abub_png_frame d;
            d.seg_begin = (uint32_t)r.segs.size();
            d.seg_count = (uint32_t)t.info.segs.size();
            d.zoff = (uint32_t)zoff;
            d.zlen = (uint32_t)t.info.zlen;
            d.lut = 0xffffffffu;
            d.reserved = 0;
            d.dst = ((uint64_t)t.s * Fmax + t.f) * P;
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
            throw std::runtime_error("RunBatched: a batch of more than 4 GB of files (lower the batch size)");
        r.ms = nowMs() - td;
        if (!r.desc.empty()) {
            sl.d_files.grow(r.bytes);
            HIPOK(hipMemcpyAsync(sl.d_files.get(), sl.h_files.get(), r.bytes, hipMemcpyHostToDevice, upStream.get()));
            HIPOK(hipStreamSynchronize(upStream.get()));
        }
    };

    auto worker = [&](int g) {
        // Everything the look-ahead thread touches lives outside the try block, and the thread is joined after it on every
        // path.  (Declaration order: the streams are finished before the buffers they use are freed.)
        Slot slots[2];
        DeviceBuffer d_model, d_z, d_raw, d_luts, d_desc, d_segs, d_status; // the model; the GPU decoder's scratch
        PinnedBuffer h_status;
        Stream copyStream, upStream;
        const int nthr = std::max(1, ndec / ngpus);
        std::thread dec;
        auto fail = [&](const std::string &msg) {
            errors[g] = msg;
            {
                std::lock_guard<std::mutex> lock(turnMu);
                failed = true;
            }
            turnCv.notify_all();
        };
        try {
            const int dev = (opt.firstDevice + g) % ndev;
            HIPOK(hipSetDevice(dev));
            const int nslots = g + ngpus < nb ? 2 : 1; // a worker with a single batch needs no second buffer
            for (int k = 0; k < nslots; ++k) {
                if (G > Ggpu)
                    slots[k].h_frames.allocate((size_t)(G - Ggpu) * perEvent);
                slots[k].d_frames.allocate((size_t)G * perEvent);
            }
            d_model.allocate(3 * (size_t)C * P); // mu | sigma | sigma6
            uint8_t *d_mu = d_model.get(), *d_sigma = d_mu + (size_t)C * P, *d_s6 = d_mu + 2 * (size_t)C * P;
            std::vector<int> tss(C);
            for (int c = 0; c < C; ++c) {
                HIPOK(hipMemcpy(d_mu + (size_t)c * P, Trainers[c]->TrainedAvgImage.data, P, hipMemcpyHostToDevice));
                HIPOK(hipMemcpy(d_sigma + (size_t)c * P, Trainers[c]->TrainedSigmaImage.data, P, hipMemcpyHostToDevice));
                tss[c] = Trainers[c]->TrainingSetSize;
            }
            check(abub_sigma6_dev(d_sigma, d_s6, (size_t)C * P, copyStream.get()), "abub_sigma6_dev");
            HIPOK(hipStreamSynchronize(copyStream.get()));
            const bool trace = getenv("ABUB_INGEST_TRACE") != nullptr;
            if (trace)
                fprintf(stderr, "worker %d: buffers and model on the device at %.1f ms\n", g, nowMs() - tAll);
            RunPipelinePtr pipe = newRunPipeline(dev, W, H, Fmax, G, C, tss.data(), std::max(1, opt.hostThreads), opt.maskDir.c_str());
            setSigmaRaw(*pipe, d_sigma);
            if (trace)
                fprintf(stderr, "worker %d: pipeline of %d events ready at %.1f ms\n", g, G, nowMs() - tAll);
            int slot = 0;
            // (an exception of the look-ahead thread -- a failed allocation, a throwing parser -- is carried over and re-thrown here)
            auto startRead = [&](int bb, int sl) {
                slots[sl].err = nullptr;
                dec = std::thread([&, bb, sl, dev, nthr]() {
                    try {
                        readBatch(bb, slots[sl], nthr, dev, upStream);
                    } catch (...) {
                        slots[sl].err = std::current_exception();
                    }
                });
            };
            if (g < nb)
                startRead(g, slot);
            if (Ggpu) {
                // (the decoder's scratch while the first batch's files are being read: sizes from the batch's frame count; the
                // stream buffer from a guess that regrows if a batch proves it wrong)
                const size_t nfMax = (size_t)Ggpu * C * Fmax;
                d_raw.grow(nfMax * abub_png_raw_stride(W, H));
                d_desc.grow(nfMax * sizeof(abub_png_frame));
                d_status.grow(nfMax * sizeof(int32_t));
                h_status.allocate(nfMax * sizeof(int32_t) + 64);
                d_z.grow(nfMax * (P / 4 * 3));
                if (trace)
                    fprintf(stderr, "worker %d: decoder scratch ready at %.1f ms\n", g, nowMs() - tAll);
            }
            for (int b = g; b < nb; b += ngpus) {
                const double tj = nowMs();
                dec.join();
                if (trace)
                    fprintf(stderr, "batch %d: waited %.1f ms for its files at %.1f ms\n", b, nowMs() - tj, nowMs() - tAll);
                Slot &S = slots[slot];
                Slot::Read &R = S.r;
                if (S.err)
                    std::rethrow_exception(S.err);
                const int bn = b + ngpus;
                if (bn < nb)
                    startRead(bn, slot ^ 1);
                const double tg = nowMs();
                const int nEv = std::min(G, (int)mine.size() - b * G), nEvGpu = std::min(nEv, Ggpu);
                const int nf = (int)R.desc.size();
                uint8_t *d_frames = S.d_frames.get();
                hipStream_t cs = copyStream.get();
                // the GPU share starts at zero (frames nobody decodes stay so, see decodeFrame); the host share is uploaded
                if (nEvGpu)
                    HIPOK(hipMemsetAsync(d_frames, 0, (size_t)nEvGpu * perEvent, cs));
                if (nEv > nEvGpu)
                    HIPOK(hipMemcpyAsync(d_frames + (size_t)nEvGpu * perEvent, S.h_frames.get(), (size_t)(nEv - nEvGpu) * perEvent,
                                         hipMemcpyHostToDevice, cs));
                const double tp = nowMs();
                if (nf) {
                    d_z.grow(R.zbytes);
                    d_raw.grow((size_t)nf * abub_png_raw_stride(W, H));
                    d_desc.grow((size_t)nf * sizeof(abub_png_frame));
                    d_segs.grow(R.segs.size() * sizeof(abub_png_seg) + 8);
                    d_luts.grow(R.luts.size() + 256);
                    HIPOK(hipMemcpyAsync(d_desc.get(), R.desc.data(), (size_t)nf * sizeof(abub_png_frame), hipMemcpyHostToDevice, cs));
                    HIPOK(hipMemcpyAsync(d_segs.get(), R.segs.data(), R.segs.size() * sizeof(abub_png_seg), hipMemcpyHostToDevice, cs));
                    if (!R.luts.empty())
                        HIPOK(hipMemcpyAsync(d_luts.get(), R.luts.data(), R.luts.size(), hipMemcpyHostToDevice, cs));
                    check(abub_png_decode_dev(S.d_files.get(), R.bytes, (const abub_png_frame *)d_desc.get(), nf,
                                              (const abub_png_seg *)d_segs.get(), (int)R.segs.size(), d_luts.get(),
                                              (int)(R.luts.size() / 256), W, H, d_z.get(), d_z.capacity(), d_raw.get(),
                                              d_raw.capacity(), d_frames, (size_t)nEv * perEvent, (int32_t *)d_status.get(), cs),
                          "abub_png_decode_dev");
                    HIPOK(hipMemcpyAsync(h_status.get(), d_status.get(), (size_t)nf * sizeof(int32_t), hipMemcpyDeviceToHost, cs));
                }
                // every write below lands after the clear above
                HIPOK(hipStreamSynchronize(cs));
                // a frame the kernels refused: the host decoder's answer (the same image, or the same failure)
                long long onGpu = 0, onHost = R.hostGood;
                std::vector<uint8_t> pix;
                for (int i = 0; i < nf; ++i) {
                    StackMeta &m = R.meta[R.where[i].first];
                    uint8_t *dst = d_frames + R.desc[i].dst;
                    if (((const int32_t *)h_status.get())[i] == 0) {
                        m.ok[R.where[i].second] = 1;
                        ++onGpu;
                        continue;
                    }
                    pix.resize(P);
                    if (cv::imdecodeInto(S.h_files.get() + R.fileOff[i], R.fileLen[i], pix.data(), W, H)) {
                        HIPOK(hipMemcpy(dst, pix.data(), P, hipMemcpyHostToDevice));
                        m.ok[R.where[i].second] = 1;
                        ++onHost;
                    } else {
                        HIPOK(hipMemsetAsync(dst, 0, P, cs)); // (a refused frame may be half written)
                        ++R.bad;
                    }
                }
                for (size_t i = 0; i < R.hostPix.size(); ++i) {
                    const size_t at = ((size_t)R.hostWhere[i].first * Fmax + R.hostWhere[i].second) * P;
                    HIPOK(hipMemcpy(d_frames + at, R.hostPix[i].data(), P, hipMemcpyHostToDevice));
                    R.meta[R.hostWhere[i].first].ok[R.hostWhere[i].second] = 1;
                    ++onHost;
                }
                const double pngms = Ggpu ? nowMs() - tp : 0;
                if (trace)
                    fprintf(stderr, "batch %d: %d frames for the GPU (%zu MB of files), %lld decoded by host threads, read + host decode %.1f ms, "
                                    "upload + GPU decode %.1f ms\n", b, nf, R.bytes >> 20, R.hostGood, R.ms, pngms);
                setStackMeta(*pipe, std::move(R.meta));
                if (const char *tf = getenv("ABUB_TEST_FAIL_BATCH")) // test hook: a batch fails while the next one decodes
                    if (atoi(tf) == b)
                        throw std::runtime_error("injected failure of batch " + std::to_string(b) + " (ABUB_TEST_FAIL_BATCH)");
                run(*pipe, d_frames, d_mu, d_s6, cs);
                const double gms = nowMs() - tg;
                double wms = 0;
                {
                    std::unique_lock<std::mutex> lock(turnMu);
                    turnCv.wait(lock, [&] { return turn == b || failed; });
                    if (failed)
                        break;
                    const double tw = nowMs();
                    for (int k = 0; k < nEv; ++k) {
                        OutputWriter out(out_dir, run_number, frameOffset, C);
                        writeEvent(*pipe, k, atoi(EventList[mine[b * G + k]].c_str()), out);
                    }
                    wms = nowMs() - tw;
                    ++turn;
                }
                turnCv.notify_all();
                {
                    std::lock_guard<std::mutex> lock(statMu);
                    st.decode_s += R.ms * 1e-3;
                    st.gpu_s += gms * 1e-3;
                    st.write_s += wms * 1e-3;
                    st.frames += onGpu + onHost;
                    st.framesFailed += R.bad;
                    st.bellowsVetoed += bellowsVetoed(*pipe);
                    st.framesGpuDecoded += onGpu;
                    st.framesHostDecoded += onHost;
                    st.gpudecode_s += pngms * 1e-3;
                }
                slot ^= 1;
            }
        } catch (std::exception &e) {
            fail(e.what());
        } catch (...) {
            fail("unknown exception");
        }
        if (dec.joinable())
            dec.join();
    };
    std::vector<std::thread> th;
    for (int g = 1; g < ngpus; ++g)
        th.emplace_back(worker, g);
    worker(0);
    for (auto &t : th)
        t.join();
    for (const std::string &e : errors)
        if (!e.empty())
            throw std::runtime_error("RunBatched: " + e);
    st.total_s = (nowMs() - tAll) * 1e-3;
    if (stats)
        *stats = st;
    return 0;
}

} // namespace abub
