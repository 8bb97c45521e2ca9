// devtrain.cpp -- TrainOnDevice (devtrain.hpp).  The frames, their order and the skip rules are those of
// Trainer::MakeAvgSigmaImage: for every event of EventList, the frames TrainingSequence = {0, 1} of the camera's sorted
// frame list; an event without frames, a frame that is missing or does not decode drops the event's pair; a pair whose
// 16-bin entropy of sat(f1 - f0) is above 0.0005 is vetoed; the kept frames, in event order, make the float Welford model.
//
// Slab layout: slot (c * E + e) * 2 + q holds frame TrainingSequence[q] of event e, camera c (W x H bytes each; slots of
// frames that do not exist stay zero and are never used).
#include "devtrain.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <iostream>
#include <sstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "AlgorithmTraining/Trainer.hpp"
#include "ParseFolder/Parser.hpp"
#include "framefiles.hpp"
#include "hostlogic.hpp"

namespace abub {

int TrainOnDevice(Parser *parser, const std::vector<std::string> &EventList, std::vector<Trainer *> &Trainers,
                  const DeviceTrainOptions &opt, DeviceTrainStats *stats, std::string *why)
{
    const double tAll = nowMs();
    auto refuse = [&](const std::string &msg) {
        if (why)
            *why = msg;
        return 1;
    };
    const int C = (int)Trainers.size(), E = (int)EventList.size(), Q = 2;
    for (Trainer *t : Trainers)
        if (t->TrainingSequence.size() != (size_t)Q)
            return refuse("a training sequence of other than two frames");
    const int nthr = std::max(1, opt.threads);

    // ---- frame lists of every (camera, event); a parser exception fails the camera (the CLI's catch: -7) ----------------
    std::vector<std::vector<std::vector<std::string>>> lists((size_t)C, std::vector<std::vector<std::string>>((size_t)E));
    std::vector<std::string> camError((size_t)C);
    {
        std::vector<std::string> errs((size_t)C * E);
        forEachTask(parser, nthr, (size_t)C * E, [&](Parser &p, size_t i) {
            try {
                p.ParseAndSortFramesInFolder(EventList[i % E], (int)(i / E), lists[i / E][i % E]);
            } catch (std::exception &e) {
                errs[i] = e.what();
            } catch (...) {
                errs[i] = "unknown exception";
            }
        });
        for (int c = 0; c < C; ++c)
            for (int e = 0; e < E && camError[c].empty(); ++e)
                camError[c] = errs[(size_t)c * E + e];
    }
    auto nameOf = [&](int c, int e, int q) -> const std::string * {
        const int which = Trainers[c]->TrainingSequence[q];
        const auto &l = lists[c][e];
        return which >= 0 && which < (int)l.size() ? &l[which] : nullptr;
    };

    // ---- the frame size: the first training frame that decodes (every camera must share it) ---------------------------
    int W = 0, H = 0;
    {
        std::unique_ptr<Parser> p(parser->clone());
        for (int c = 0; c < C; ++c) {
            if (!camError[c].empty())
                continue;
            int cw = 0, ch = 0;
            for (int e = 0; e < E && !cw; ++e)
                for (int q = 0; q < Q && !cw; ++q)
                    if (const std::string *n = nameOf(c, e, q)) {
                        cv::Mat m;
                        try {
                            if (p->GetImage(EventList[e], *n, m) != -1 && !m.empty()) {
                                cw = m.cols;
                                ch = m.rows;
                            }
                        } catch (...) {
                        }
                    }
            if (!cw)
                continue; // (nothing decodes: the camera's training set is empty)
            if (!W) {
                W = cw;
                H = ch;
            } else if (cw != W || ch != H)
                return refuse("cameras with different frame sizes");
        }
    }
    const size_t P = (size_t)W * H;
    const size_t nslots = (size_t)C * E * Q;
    const size_t slab = nslots * P;
    if (slab > opt.capBytes)
        return refuse("training slab of " + std::to_string(slab >> 20) + " MB above the cap of " +
                      std::to_string(opt.capBytes >> 20) + " MB");

    // ---- read / walk / decode ------------------------------------------------------------------------------------------
    // GPU decode where the parser hands out the files and the width is one the PNG kernels take (packed frames too); other frames are decoded by
    // the reading threads (GetImage, as the host path does)
    const bool devDecode = gpuDecodeWanted(opt.gpuDecode, W);
    DeviceTrainBuffers own;
    DeviceTrainBuffers &B = opt.buffers ? *opt.buffers : own;
    FileBatch &batch = B.batch;
    std::vector<FileTask> &tasks = batch.ft;
    const std::vector<uint8_t> &good = batch.good;
    std::vector<uint8_t> otherSize(nslots, 0);
    std::vector<std::string> frameError(nslots);
    std::fill(batch.decodedBy, batch.decodedBy + NGpuCodecs, 0);
    batch.hostDecoded = 0;
    batch.begin();
    if (W) {
        batch.sizer.reset(parser->clone());
        for (int c = 0; c < C; ++c)
            for (int e = 0; e < E && camError[c].empty(); ++e)
                for (int q = 0; q < Q; ++q)
                    if (const std::string *n = nameOf(c, e, q)) {
                        FileTask &t = batch.plan((c * E + e) * Q + q, 0, EventList[e], *n, devDecode);
                        if (t.state == FileTask::Bad)
                            t.state = FileTask::Other; // decoded by GetImage below (a parser that has no files to hand out)
                    }
    }
    batch.ready();
    const auto readOne = [&](Parser &p, size_t i) {
        FileTask &t = tasks[i];
        const int c = t.s / (E * Q), e = t.s / Q % E, q = t.s % Q;
        const std::string &n = *nameOf(c, e, q);
        if (t.state != FileTask::Other) {
            batch.read(p, i, EventList[e], n, W, H);
            if (t.state == FileTask::Bad && t.read) { // refused at W x H: a frame of another size is not a corrupt one
                cv::Mat m = cv::imdecode(batch.h_files.get() + t.off, (size_t)t.size, 0);
                otherSize[t.s] = !m.empty() && (m.cols != W || m.rows != H);
            }
            return;
        }
        cv::Mat m;
        try {
            if (p.GetImage(EventList[e], n, m) != -1 && !m.empty()) {
                if (m.cols != W || m.rows != H)
                    otherSize[t.s] = 1;
                else {
                    t.pix.assign(m.data, m.data + P);
                    t.state = FileTask::HostDecoded;
                }
            }
        } catch (std::exception &ex) {
            frameError[t.s] = ex.what();
        } catch (...) {
            frameError[t.s] = "unknown exception";
        }
    };
    forEachTask(parser, nthr, tasks.size(), readOne);

    DeviceTrainStats st;
    st.slabBytes = slab;
    std::ostringstream msg; // (the host path's lines, printed or handed to opt.log at the end)
    if (W) {
        HIPOK(hipSetDevice(opt.device));
        hipStream_t cs = B.stream.get();
        batch.inflate(parser, nthr, cs, readOne);
        batch.reset(nslots, slab);
        HIPOK(hipMemsetAsync(batch.slab.get(), 0, slab, cs)); // (frames nobody decodes stay zero)
        batch.upload(cs);
        // decode launches of at most 4 frames per CU, as RunBatched's batches: the decoder's scratch stays bounded
        const size_t perLaunch = framesPerBatch(opt.device);
        for (size_t i0 = 0; i0 < tasks.size();) {
            size_t i1 = i0, ngpu = 0;
            for (; i1 < tasks.size() && (ngpu < perLaunch || !tasks[i1].onGpu()); ++i1)
                ngpu += tasks[i1].onGpu();
            st.decodeLaunches += batch.launch(i0, i1, W, H, [&](int s, int) { return (uint64_t)s * P; }, cs);
            HIPOK(hipStreamSynchronize(cs));
            batch.finish(W, H, cs);
            st.framesGpuDecoded = std::accumulate(batch.decodedBy, batch.decodedBy + NGpuCodecs, 0LL);
            st.framesGpuUnpacked = batch.decodedBy[GpuPacked];
            st.framesGpuBmp = batch.decodedBy[GpuBmp];
            st.framesGpuUnzipped = batch.unzip.unzipped;
            st.framesHostDecoded = batch.hostDecoded;
            i0 = i1;
        }
        HIPOK(hipStreamSynchronize(cs));
        st.frames = st.framesGpuDecoded + st.framesHostDecoded;

        // ---- the veto: one histogram of sat(f1 - f0) per (camera, event) whose two frames are there ---------------------
        std::vector<abub_job> pairs;
        std::vector<int> pairOf((size_t)C * E, -1);
        for (int c = 0; c < C; ++c)
            for (int e = 0; e < E; ++e) {
                const int s = (c * E + e) * Q;
                if (good[s] && good[s + 1]) {
                    pairOf[(size_t)c * E + e] = (int)pairs.size();
                    // (`out` counts within a launch of at most 65535 pairs, the launcher's grid limit)
                    pairs.push_back(abub_job{(uint32_t)s + 1, (uint32_t)s, 0, (uint32_t)(pairs.size() % 65535)});
                }
            }
        std::vector<uint32_t> hist(pairs.size() * 256);
        if (!pairs.empty()) {
            B.pairs.grow(pairs.size() * sizeof(abub_job));
            B.hist.grow(hist.size() * sizeof(uint32_t));
            HIPOK(hipMemcpyAsync(B.pairs.get(), pairs.data(), pairs.size() * sizeof(abub_job), hipMemcpyHostToDevice, cs));
            for (size_t k0 = 0; k0 < pairs.size(); k0 += 65535) {
                const int n = (int)std::min<size_t>(65535, pairs.size() - k0);
                check(abub_pair_hist_dev(batch.slab.get(), (const abub_job *)B.pairs.get() + k0, n, W, H,
                                         (uint32_t *)B.hist.get() + k0 * 256, cs),
                      "abub_pair_hist_dev");
            }
            HIPOK(hipMemcpyAsync(hist.data(), B.hist.get(), hist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, cs));
            HIPOK(hipStreamSynchronize(cs));
        }

        // ---- per camera, in event order: the host path's messages, the kept frames, the Welford pass --------------------
        B.idx.grow((size_t)E * Q * sizeof(uint32_t) + 256);
        B.mu.grow(P);
        B.sigma.grow(P);
        for (int c = 0; c < C; ++c) {
            Trainer &T = *Trainers[c];
            msg << "Camera " << c << " training ... ";
            if (!camError[c].empty()) {
                msg << camError[c] << '\n';
                T.StatusCode = -7;
                continue;
            }
            std::vector<uint32_t> kept;
            std::string failed;
            for (int e = 0; e < E && failed.empty(); ++e) {
                const int s = (c * E + e) * Q;
                bool ok = true, sized = false;
                for (int q = 0; q < Q && failed.empty(); ++q)
                    failed = frameError[s + q]; // (re-thrown at its event, before the event's messages)
                if (!failed.empty())
                    break;
                if (!lists[c][e].empty()) {
                    for (int q = 0; q < Q; ++q) {
                        sized = sized || otherSize[s + q];
                        if (!good[s + q] && !otherSize[s + q]) {
                            msg << "Skipping corrupted image for training.\n";
                            ok = false;
                        }
                    }
                } else {
                    msg << "Event " << EventList[e] << " is nonexistant on the disk. Skipping training on this event\n";
                    ok = false;
                }
                if (ok && sized) { // (both frames decode, not both at the camera's size; see devtrain.hpp)
                    failed = "Trainer: training frames differ in size";
                    break;
                }
                float entropy = 0.f;
                if (ok)
                    entropy = entropyFromHist(&hist[(size_t)pairOf[(size_t)c * E + e] * 256], 16, P);
                if (entropy <= 0.0005 && ok)
                    for (int q = 0; q < Q; ++q)
                        kept.push_back((uint32_t)(s + q));
            }
            if (!failed.empty()) {
                msg << failed << '\n';
                T.StatusCode = -7;
                continue;
            }
            if (kept.empty()) {
                msg << "Training image set for camera " << c << " has 0 frames. This means that the event is malformed.\n";
                T.StatusCode = -7;
                continue;
            }
            HIPOK(hipMemcpyAsync(B.idx.get(), kept.data(), kept.size() * sizeof(uint32_t), hipMemcpyHostToDevice, cs));
            check(abub_train_dev(batch.slab.get(), (const uint32_t *)B.idx.get(), (int)kept.size(), W, H, B.mu.get(),
                                 B.sigma.get(), cs),
                  "abub_train_dev");
            T.TrainedAvgImage.create(H, W, CV_8U);
            T.TrainedSigmaImage.create(H, W, CV_8U);
            HIPOK(hipMemcpyAsync(T.TrainedAvgImage.data, B.mu.get(), P, hipMemcpyDeviceToHost, cs));
            HIPOK(hipMemcpyAsync(T.TrainedSigmaImage.data, B.sigma.get(), P, hipMemcpyDeviceToHost, cs));
            HIPOK(hipStreamSynchronize(cs)); // (kept and the index buffer are reused by the next camera)
            T.TrainingSetSize = (int)kept.size();
            T.StatusCode = 0;
            T.ModelId = Trainer::NextModelId();
            msg << "complete.\n";
        }
    } else {
        // no camera has a frame that decodes: every camera fails as the host path does
        for (int c = 0; c < C; ++c) {
            msg << "Camera " << c << " training ... ";
            if (!camError[c].empty()) {
                msg << camError[c] << '\n';
                Trainers[c]->StatusCode = -7;
                continue;
            }
            for (int e = 0; e < E; ++e) {
                if (lists[c][e].empty()) {
                    msg << "Event " << EventList[e] << " is nonexistant on the disk. Skipping training on this event\n";
                    continue;
                }
                for (int q = 0; q < Q; ++q)
                    msg << "Skipping corrupted image for training.\n";
            }
            msg << "Training image set for camera " << c << " has 0 frames. This means that the event is malformed.\n";
            Trainers[c]->StatusCode = -7;
        }
    }
    if (opt.log)
        *opt.log += msg.str();
    else {
        fputs(msg.str().c_str(), stdout);
        fflush(stdout);
    }
    st.total_s = (nowMs() - tAll) * 1e-3;
    if (stats)
        *stats = st;
    return 0;
}

} // namespace abub
