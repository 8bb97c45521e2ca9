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
#include <future>
#include <iostream>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "AlgorithmTraining/Trainer.hpp"
#include "BubbleLocalizer/L3Localizer.hpp"
#include "ParseFolder/Parser.hpp"
#include "ParseFolder/RawParser.hpp"
#include "ParseFolder/ZipParser.hpp"
#include "PICOFormatWriter/PICOFormatWriterV4.hpp"
#include "devctx.hpp"
#include "devtrain.hpp"
#include "driver.hpp"
#include "framefiles.hpp"
#include "holders.hpp"
#include "peek.hpp"
#include "pipeline.hpp"
#include "pngwalk.hpp"
#include "stackresult.hpp"
#include "runbatch.hpp"

namespace abub {
namespace {

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
    FileBatch batch;           // the GPU share's files, read, inflated and uploaded by the reading thread (the copy runs beside
                               // the GPU work of the batch before), and their descriptors (fd); its slab and scratch stay empty
    std::exception_ptr err;    // of the look-ahead thread that read the batch
    struct Read {
        std::vector<StackMeta> meta;
        double ms = 0;
        long long hostGood = 0;
        long long unzipped = 0; // archive entries abub_unzip_dev inflated
        double unzip_s = 0;     // ... and what the device's part of that took (GpuUnzip::device_s)
    } r;
};

// A worker's buffers, streams and pipelines, kept from one run to the next (RunCampaign) or for one run (RunBatched).
// Declaration order: the pipelines go first, then the streams (they finish their work), then the buffers.
struct WorkerCache {
    Slot slots[2];
    DeviceBuffer d_model; // mu | sigma | sigma6
    DecodeScratch scratch; // the GPU decoders' scratch
    Stream copyStream, upStream;
    struct Pipe {
        std::vector<long long> key;
        RunPipelinePtr pipe;
    };
    std::vector<Pipe> pipes; // the last two shapes (a run of another size does not throw away the campaign's pipeline)
};

// the worker caches of a campaign (one per GPU) and how many pipelines they built
struct Workers {
    std::vector<std::unique_ptr<WorkerCache>> w;
    int pipelinesBuilt = 0;
};

// at least `bytes`, allocated exactly when it has to grow (pinned memory is page-locked, every byte costs)
template <bool Pinned>
void fit(Buffer<Pinned> &b, size_t bytes)
{
    if (b.capacity() < bytes)
        b.allocate(bytes);
}

// RunBatched on the workers `ws` (their buffers and pipelines are reused where they fit, and kept for the next run)
int runBatchedOn(Workers &ws, Parser *parser, const std::vector<std::string> &EventList, const std::vector<Trainer *> &Trainers,
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
    // On the GPU (abub_png.hip, abub_abf.hip, abub_bmp.hip) when the parser hands out the files as they are stored and the
    // first frame is a PNG the kernels take, a packed frame or, with ABUB_GPU_BMP=1, a BMP the host decoder reads; a host
    // thread still reads each file, walks a PNG's chunks or a BMP's header, and decodes the odd frame the GPU path refuses.
    // Otherwise host threads decode every frame (GetImageInto).  The width gate is the
    // PNG kernels': it holds for packed frames too, although abub_abf_decode_dev takes any width.
    bool devDecode = gpuDecodeWanted(opt.gpuDecode, W);
    if (devDecode) {
        devDecode = false;
        for (size_t k = 0; k < lists.size() && !devDecode; ++k)
            for (int c = 0; c < C && !devDecode; ++c)
                if (!lists[k][c].empty()) {
                    std::unique_ptr<Parser> p(parser->clone());
                    const long long sz = p->GetImageFileSize(EventList[mine[k]], lists[k][c][0]);
                    if (sz > 0 && sz < ((long long)1 << 30)) {
                        std::vector<unsigned char> buf((size_t)sz);
                        FileTask probe;
                        devDecode = p->ReadImageFile(EventList[mine[k]], lists[k][c][0], buf.data(), buf.size()) == sz &&
                                    gpuCodecOf(buf.data(), buf.size(), W, H, probe, DecodeKnobs::fromEnv());
                    }
                    k = lists.size(); // (one probe decides)
                    break;
                }
    }
    int Ggpu = 0; // the first Ggpu events of a batch are decoded on the GPU, the others by the host threads
    if (devDecode) {
        // batches carry framesPerBatch frames for the GPU (1024 on an MI355X), not one more
        int nd = 0;
        const int perBatch = (int)framesPerBatch(hipGetDeviceCount(&nd) == hipSuccess && nd > 0 ? opt.firstDevice % nd : 0);
        const int perEv = std::max(1, C * Fmax);
        const int capG = (int)std::max<size_t>(1, opt.batchBytes / perEvent);
        Ggpu = std::max(1, std::min(perBatch / perEv, std::min(capG, (int)mine.size())));
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
    // --peek: where the images go and which route forms them
    const bool peekOn = !opt.peekDir.empty();
    const std::string peekRunDir = opt.peekDir + (opt.peekDir.empty() || opt.peekDir.back() == '/' ? "" : "/") + run_number + "/";
    bool peekGpu = opt.peekGpu != 0;
    int peekMaxStacks = opt.peekMaxStacks;
    if (peekOn) {
        if (const char *e = getenv("ABUB_PEEK_GPU"))
            if (opt.peekGpu < 0)
                peekGpu = atoi(e) != 0;
        if (const char *e = getenv("ABUB_PEEK_BATCH"))
            peekMaxStacks = std::max(1, atoi(e));
        st.peekGpu = peekGpu ? 1 : 0;
    }
    int ndev = 0;
    HIPOK(hipGetDeviceCount(&ndev));
    if (ndev <= 0)
        throw std::runtime_error("RunBatched: no GPU");
    const int ngpus = std::max(1, std::min(opt.ngpus, nb));
    st.gpus = ngpus;
    while ((int)ws.w.size() < ngpus)
        ws.w.emplace_back(new WorkerCache());
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
        FileBatch &B = sl.batch; // (tasks in stack order: the GPU's files are read first, its work can start before the host's is done)
        B.sizer.reset(Ggpu ? parser->clone() : nullptr);
        std::fill(B.decodedBy, B.decodedBy + NGpuCodecs, 0);
        B.hostDecoded = 0;
        B.begin();
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
                for (int f = 0; f < (int)m.names.size(); ++f) // (the host share's tasks stay Other)
                    B.plan(k * C + c, f, m.eventID, m.names[f], k < Ggpu);
            }
        B.ready();
        std::atomic<long long> hostGood{0}, hostBad{0};
        const auto readOne = [&](Parser &p, size_t i) {
            const FileTask &t = B.ft[i];
            StackMeta &m = r.meta[t.s];
            if (t.state == FileTask::Other) { // the host share: straight into the pinned slab
                uint8_t *dst = sl.h_frames.get() + ((size_t)(t.s - Ggpu * C) * Fmax + t.f) * P;
                ++(decodeFrame(p, m, t.f, dst, W, H) ? hostGood : hostBad);
                return;
            }
            B.read(p, i, m.eventID, m.names[t.f], W, H); // (what a decoder does not take is uploaded by the worker, FileBatch::finishInto)
        };
        forEachTask(parser, nthreads, B.ft.size(), readOne);
        B.inflate(parser, nthreads, upStream.get(), readOne);
        r.unzipped = B.unzip.unzipped;
        r.unzip_s = B.unzip.device_s;
        B.describe(0, B.ft.size(), [&](int s, int f) { return ((uint64_t)s * Fmax + f) * P; });
        B.fd.bad += hostBad;
        r.hostGood = hostGood;
        r.ms = nowMs() - td;
        if (B.upload(upStream.get()))
            HIPOK(hipStreamSynchronize(upStream.get()));
    };

    auto worker = [&](int g) {
        // Everything the look-ahead thread touches lives outside the try block (in the worker's cache), and the thread is
        // joined after it on every path.
        WorkerCache &wc = *ws.w[g];
        Slot *slots = wc.slots;
        DecodeScratch &scratch = wc.scratch;
        Stream &copyStream = wc.copyStream, &upStream = wc.upStream;
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
                    fit(slots[k].h_frames, (size_t)(G - Ggpu) * perEvent);
                fit(slots[k].d_frames, (size_t)G * perEvent);
            }
            fit(wc.d_model, 3 * (size_t)C * P); // mu | sigma | sigma6
            uint8_t *d_mu = wc.d_model.get(), *d_sigma = d_mu + (size_t)C * P, *d_s6 = d_mu + 2 * (size_t)C * P;
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
            // a pipeline of this shape from an earlier run takes the new model's training-set sizes; otherwise one is built
            RunPipeline *pipe = nullptr;
            {
                const std::vector<long long> key = {dev, W, H, Fmax, G, C, std::max(1, opt.hostThreads)};
                for (size_t i = 0; i < wc.pipes.size() && !pipe; ++i)
                    if (wc.pipes[i].key == key && setTrainingSetSizes(*wc.pipes[i].pipe, tss.data())) {
                        std::rotate(wc.pipes.begin(), wc.pipes.begin() + i, wc.pipes.begin() + i + 1); // (most recent first)
                        pipe = wc.pipes[0].pipe.get();
                    }
                if (!pipe) {
                    if (wc.pipes.size() >= 2)
                        wc.pipes.pop_back();
                    WorkerCache::Pipe np;
                    np.key = key;
                    np.pipe = newRunPipeline(dev, W, H, Fmax, G, C, tss.data(), std::max(1, opt.hostThreads), opt.maskDir.c_str());
                    wc.pipes.insert(wc.pipes.begin(), std::move(np));
                    pipe = wc.pipes[0].pipe.get();
                    std::lock_guard<std::mutex> lock(statMu);
                    ++ws.pipelinesBuilt;
                }
            }
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
                scratch.raw.grow(nfMax * abub_png_raw_stride(W, H));
                scratch.lane[GpuPng].desc.grow(nfMax * sizeof(abub_png_frame));
                scratch.lane[GpuPng].status.grow(nfMax * sizeof(int32_t));
                fit(scratch.lane[GpuPng].h_status, nfMax * sizeof(int32_t) + 64);
                scratch.z.grow(nfMax * (P / 4 * 3));
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
                FileBatch &B = S.batch;
                const int nf = (int)B.fd.gpuFrames();
                uint8_t *d_frames = S.d_frames.get();
                hipStream_t cs = copyStream.get();
                // the GPU share starts at zero (frames nobody decodes stay so, see decodeFrame); the host share is uploaded
                if (nEvGpu)
                    HIPOK(hipMemsetAsync(d_frames, 0, (size_t)nEvGpu * perEvent, cs));
                if (nEv > nEvGpu)
                    HIPOK(hipMemcpyAsync(d_frames + (size_t)nEvGpu * perEvent, S.h_frames.get(), (size_t)(nEv - nEvGpu) * perEvent,
                                         hipMemcpyHostToDevice, cs));
                const double tp = nowMs();
                B.launchInto(W, H, d_frames, (size_t)nEv * perEvent, scratch, cs);
                // every write below lands after the clear above (waited for whether a decoder was launched or not)
                HIPOK(hipStreamSynchronize(cs));
                B.finishInto(W, H, d_frames, scratch, cs, [&](int s, int f) { R.meta[s].ok[f] = 1; });
                const long long onHost = R.hostGood + B.hostDecoded, onGpu = B.fd.decoded();
                const double pngms = Ggpu ? nowMs() - tp : 0;
                if (trace)
                    fprintf(stderr, "batch %d: %d frames for the GPU (%zu MB of files), %lld decoded by host threads, read + host decode %.1f ms, "
                                    "upload + GPU decode %.1f ms\n", b, nf, B.fd.bytes >> 20, R.hostGood, R.ms, pngms);
                setStackMeta(*pipe, std::move(R.meta));
                if (const char *tf = getenv("ABUB_TEST_FAIL_BATCH")) // test hook: a batch fails while the next one decodes
                    if (atoi(tf) == b)
                        throw std::runtime_error("injected failure of batch " + std::to_string(b) + " (ABUB_TEST_FAIL_BATCH)");
                run(*pipe, d_frames, d_mu, d_s6, cs);
                // ---- the DebugPeek images of the batch's accepted stacks, while its frames are still resident -------------------
                PeekStats ps;
                double pms = 0;
                if (peekOn) {
                    const double tk = nowMs();
                    std::vector<PeekStack> accepted;
                    for (int s = 0; s < nEv * C; ++s) {
                        const StackResult &res = stackResult(*pipe, s);
                        if (res.staged != 0 || res.bubbles.empty())
                            continue;
                        PeekStack ks;
                        ks.eventID = stackEventID(*pipe, s);
                        ks.cam = s % C;
                        ks.trigFrame = (uint32_t)(s * Fmax + res.trig);
                        ks.preFrame = (uint32_t)(s * Fmax + peekPreFrame(res.trig, tss[s % C]));
                        ks.loc_thres = res.loc_thres;
                        ks.rects = res.rects;
                        accepted.push_back(std::move(ks));
                    }
                    writePeekImages(W, H, C, d_frames, (size_t)nEv * perEvent, d_mu, d_s6, accepted, peekRunDir, peekGpu,
                                    std::max<size_t>(opt.batchBytes / 8, (size_t)64 << 20), peekMaxStacks, nthr, cs, ps);
                    pms = nowMs() - tk;
                }
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
                    st.framesFailed += B.fd.bad;
                    st.bellowsVetoed += bellowsVetoed(*pipe);
                    st.framesGpuDecoded += onGpu;
                    st.framesHostDecoded += onHost;
                    st.framesGpuUnpacked += B.fd.decodedBy[GpuPacked];
                    st.framesGpuBmp += B.fd.decodedBy[GpuBmp];
                    st.framesGpuUnzipped += R.unzipped;
                    st.unzip_s += R.unzip_s;
                    st.gpudecode_s += pngms * 1e-3;
                    st.peekStacks += ps.stacks;
                    st.peekFiles += ps.files;
                    st.peekBytes += ps.bytes;
                    st.peekSubBatches += ps.subBatches;
                    st.peek_s += pms * 1e-3;
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

} // namespace

int RunBatched(Parser *parser, const std::vector<std::string> &EventList, const std::vector<Trainer *> &Trainers,
               int numCams, const std::string &out_dir, const std::string &run_number, int frameOffset,
               const BatchedRunOptions &opt, BatchedRunStats *stats, std::string *why)
{
    Workers ws;
    return runBatchedOn(ws, parser, EventList, Trainers, numCams, out_dir, run_number, frameOffset, opt, stats, why);
}

void RunPerEvent(Parser *parser, const std::vector<std::string> &EventList, const std::vector<Trainer *> &Trainers,
                 int numCams, const std::string &eventDir, const std::string &out_dir, const std::string &run_number,
                 int frameOffset, const std::string &maskDir, int nthreads, int eventUser, int debugMode, int shardRank,
                 int shardWorld)
{
    // events in parallel, output appended in event order (the `ordered` clause :380-383)
    std::cout << "Total threads: " << nthreads << std::endl;
    std::vector<Trainer *> trainers = Trainers; // (L3Localizer takes Trainer **)
    std::atomic<int> next{0};
    std::mutex turnMutex;
    std::condition_variable turnCv;
    int turn = 0;
    auto worker = [&]() {
        for (;;) {
            const int evi = next.fetch_add(1);
            if (evi >= (int)EventList.size())
                break;
            const bool skip = (eventUser >= 0 && evi != eventUser) // compares the loop index, like upstream (:350)
                              || (shardWorld > 1 && evi % shardWorld != shardRank);
            OutputWriter *out = nullptr;
            std::vector<AnalyzerUnit *> Analyzers;
            if (!skip) {
                out = new OutputWriter(out_dir, run_number, frameOffset, numCams);
                const std::string imageDir = eventDir + EventList[evi] + "/Images/";
                const int actualEventNumber = atoi(EventList[evi].c_str());
                for (int icam = 0; icam < numCams; icam++) {
                    Analyzers.push_back(new L3Localizer(EventList[evi], imageDir, icam, debugMode / 100 ? false : true,
                                                        &trainers[icam], maskDir, parser->clone()));
                    AnyCamAnalysis(Analyzers[icam], icam, debugMode % 10 ? false : true, out, out_dir, actualEventNumber);
                }
            }
            {
                std::unique_lock<std::mutex> lock(turnMutex);
                turnCv.wait(lock, [&] { return turn == evi; });
                if (out)
                    out->writeCameraOutput();
                ++turn;
            }
            turnCv.notify_all();
            delete out;
            for (AnalyzerUnit *A : Analyzers)
                delete A;
        }
    };
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back(worker);
    for (auto &t : th)
        t.join();
}

PreparedRun::PreparedRun() = default;
PreparedRun::PreparedRun(PreparedRun &&) = default;
PreparedRun &PreparedRun::operator=(PreparedRun &&) = default;
PreparedRun::~PreparedRun() = default;

void PrintBatchedLine(const BatchedRunStats &bs)
{
    printf("batched detect: %d events in %d batches of <= %d on %d GPU(s), %lld frames %dx%d decoded (%lld on the GPU, %lld on "
           "host threads; %lld undecodable), %.2f s total (list %.2f, read/decode %.2f, upload+GPU+host stages %.2f of which "
           "GPU decode %.2f, write %.2f) = %.1f frames/s ingest-inclusive\n",
           bs.events, bs.batches, bs.eventsPerBatch, bs.gpus, bs.frames, bs.W, bs.H, bs.framesGpuDecoded, bs.framesHostDecoded,
           bs.framesFailed, bs.total_s, bs.list_s, bs.decode_s, bs.gpu_s, bs.gpudecode_s, bs.write_s,
           bs.total_s > 0 ? (bs.frames + bs.framesFailed) / bs.total_s : 0.0);
    if (bs.peekGpu >= 0)
        printf("peek: %lld stacks, %lld files, %lld bytes, %s\n", bs.peekStacks, bs.peekFiles, bs.peekBytes, bs.peekGpu ? "gpu" : "host");
}

// (a line for stdout, or held back in pr.log)
static void say(PreparedRun &pr, bool buffered, const std::string &line)
{
    if (buffered)
        pr.log += line;
    else {
        fputs(line.c_str(), stdout);
        fflush(stdout);
    }
}

PreparedRun PrepareRun(const RunSpec &r, const BatchedRunOptions &opt, int trainerDebug, DeviceTrainBuffers *buffers,
                       bool buffered)
{
    PreparedRun pr;
    const int C = r.numCams;
    try {
        if (r.zipped)
            pr.parser.reset(new ZipParser(r.eventDir, r.imageFolder, r.imageFormat));
        else
            pr.parser.reset(new RawParser(r.eventDir, r.imageFolder, r.imageFormat));
        pr.parser->GetEventDirLists(pr.events);
    } catch (...) {
        say(pr, buffered, "Failed to read the images from run " + r.runId + ". Autobub cannot continue.\n");
        pr.rc = -5;
        return pr;
    }
    sortEvents(pr.events);

    say(pr, buffered, "**Starting training. AutoBub is in learn mode**\n");
    const double t0 = nowMs();
    for (int icam = 0; icam < C; icam++) {
        pr.owned.emplace_back(new Trainer(icam, pr.events, r.eventDir, r.imageFormat, r.imageFolder, pr.parser->clone(),
                                          trainerDebug != 0));
        pr.trainers.push_back(pr.owned.back().get());
    }
    int declined = 1;
    if (opt.trainOnGpu) {
        int ndev = 0;
        HIPOK(hipGetDeviceCount(&ndev));
        if (ndev <= 0)
            throw std::runtime_error("TrainOnDevice: no GPU");
        DeviceTrainOptions to;
        to.device = opt.firstDevice % ndev;
        to.threads = std::max(1, opt.decodeThreads / 4); // (the detect of the run before reads with the others)
        to.capBytes = opt.batchBytes;
        to.gpuDecode = opt.gpuDecode;
        to.buffers = buffers;
        to.log = buffered ? &pr.log : nullptr;
        std::string why;
        DeviceTrainStats ts;
        declined = TrainOnDevice(pr.parser.get(), pr.events, pr.trainers, to, &ts, &why);
        pr.trainGpuUnzipped = ts.framesGpuUnzipped;
        if (declined)
            say(pr, buffered, "device training not used (" + why + "): training on host threads\n");
    }
    if (declined) {
        // (the host Trainer prints its own lines as it goes: they are not held back)
        pr.hostTrained = true;
        std::vector<std::thread> th; // one thread per camera, like `#pragma omp parallel for` (:304-307)
        for (int icam = 0; icam < C; icam++)
            th.emplace_back([&, icam]() {
                try {
                    pr.trainers[icam]->MakeAvgSigmaImage(false);
                } catch (std::exception &e) {
                    std::cout << e.what() << '\n';
                    pr.trainers[icam]->StatusCode = -7;
                }
            });
        for (auto &t : th)
            t.join();
    }
    pr.train_s = (nowMs() - t0) * 1e-3;
    for (Trainer *t : pr.trainers)
        if (t->StatusCode)
            pr.rc = -7;
    say(pr, buffered, pr.rc ? "Failed to train on images from run " + r.runId + ". Autobub cannot continue.\n"
                            : std::string("***Training complete. AutoBub is now in detect mode***\n"));
    return pr;
}

void CommitRun(const RunSpec &r, const BatchedRunOptions &opt, PreparedRun &pr)
{
    if (!pr.log.empty()) {
        fputs(pr.log.c_str(), stdout);
        fflush(stdout);
        pr.log.clear();
    }
    const int C = r.numCams;
    OutputWriter header(opt.outDir, r.runId, r.frameOffset, C);
    header.writeHeader();
    if (pr.rc == -5 && opt.shardRank == 0) { // (one block for the run: it goes into part 0 of a sharded run)
        for (int icam = 0; icam < C; icam++)
            header.stageCameraOutputError(icam, -5, -1);
        header.writeCameraOutput();
    }
    if (pr.rc == -7)
        for (size_t evi = 0; evi < pr.events.size(); evi++) {
            if (opt.shardWorld > 1 && (int)(evi % (size_t)opt.shardWorld) != opt.shardRank)
                continue;
            for (int icam = 0; icam < C; icam++)
                header.stageCameraOutputError(icam, -7, atoi(pr.events[evi].c_str()));
            header.writeCameraOutput();
        }
}

int RunCampaign(const std::vector<RunSpec> &runs, const BatchedRunOptions &opt, CampaignStats *stats)
{
    const double tAll = nowMs();
    CampaignStats cs;
    cs.status.assign(runs.size(), 0);
    Workers ws;
    DeviceTrainBuffers trainBuffers; // (one run is prepared at a time: the next starts once the last one was taken)
    // run k + 1 is listed and trained while run k is detected: at most one run ahead.  Nothing of it is written, and its
    // device-training lines are held back, until run k is done.
    auto prepare = [&](size_t k) {
        return std::async(std::launch::async, [&, k]() { return PrepareRun(runs[k], opt, 0, &trainBuffers, true); });
    };
    std::future<PreparedRun> next;
    if (!runs.empty())
        next = prepare(0);
    size_t k = 0;
    for (; k < runs.size(); ++k) {
        const RunSpec &r = runs[k];
        const double tw = nowMs();
        PreparedRun pr;
        try {
            pr = next.get();
        } catch (std::exception &e) { // (a HIP failure of device training)
            std::cout << "training failed: " << e.what() << std::endl;
            cs.status[k] = -6;
            ++cs.runs;
            break;
        }
        cs.trainExposed_s += (nowMs() - tw) * 1e-3;
        ++cs.runs;
        if (k + 1 < runs.size())
            next = prepare(k + 1);
        cs.train_s += pr.train_s;
        cs.trainedOnHost += pr.hostTrained ? 1 : 0;
        cs.trainGpuUnzipped += pr.trainGpuUnzipped;
        CommitRun(r, opt, pr);
        if (pr.rc) {
            cs.status[k] = pr.rc;
            continue;
        }
        BatchedRunStats bs;
        std::string why;
        int rc = 1;
        try {
            rc = runBatchedOn(ws, pr.parser.get(), pr.events, pr.trainers, r.numCams, opt.outDir, r.runId, r.frameOffset, opt,
                              &bs, &why);
        } catch (std::exception &e) {
            std::cout << "batched detect failed: " << e.what() << std::endl;
            cs.status[k] = -6;
            break;
        }
        if (rc == 0) {
            PrintBatchedLine(bs);
            cs.frames += bs.frames + bs.framesFailed;
            cs.framesGpuUnzipped += bs.framesGpuUnzipped;
        } else {
            std::cout << "batched detect not used (" << why << "): falling back to the per-event loop" << std::endl;
            RunPerEvent(pr.parser.get(), pr.events, pr.trainers, r.numCams, r.eventDir, opt.outDir, r.runId, r.frameOffset,
                        opt.maskDir, std::max(1, opt.perEventThreads), -1, 0, opt.shardRank, opt.shardWorld);
        }
        printf("run complete.\n");
        printf("AutoBub done analyzing this run. Thank you.\n");
    }
    if (k < runs.size()) { // ended by a failure: the run prepared ahead is neither written nor detected
        if (next.valid()) {
            try {
                next.get();
            } catch (...) {
            }
        }
        for (size_t j = k + 1; j < runs.size(); ++j)
            cs.notRun.push_back(runs[j].runId);
    }
    cs.pipelinesBuilt = ws.pipelinesBuilt;
    cs.total_s = (nowMs() - tAll) * 1e-3;
    if (stats)
        *stats = cs;
    for (int st : cs.status)
        if (st)
            return st;
    return 0;
}

} // namespace abub
