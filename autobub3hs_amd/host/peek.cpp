// peek.cpp -- writePeekImages (peek.hpp): the six DebugPeek images of the accepted stacks of a resident batch.  What
// L3Localizer::CalculateInitialBubbleParams writes on the analyzer's thread with cv::imwrite (L3Localizer.cpp:222-257, 397,
// 448), for a whole batch: one store-mode K2 launch for D(trig, pre) and its histogram, the Otsu cut on the host, then
// either abub_peek_planes_dev + the PNG encoder through EncodeBatch (encodebatch.hpp; files come back finished) or, as the
// definition, host threads that form the planes from frames copied back and encode with cv::pngHuffEncode.  Both routes
// write the same bytes.
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstring>
#include <stdexcept>

#include "abub_hip.h"
#include "devctx.hpp"
#include "encodebatch.hpp"
#include "framefiles.hpp"
#include "holders.hpp"
#include "hostlogic.hpp"
#include "peek.hpp"
#include "runframes.hpp"

namespace abub {

void peekPlanesHost(const uint8_t *D, const uint8_t *trig, int W, int H, int cut, const std::vector<cv::Rect> &rects, uint8_t *thr,
                    uint8_t *pres)
{
    const size_t P = (size_t)W * H;
    for (size_t i = 0; i < P; ++i)
        thr[i] = (int)D[i] > cut ? 255 : 0;
    cv::Mat m(H, W, CV_8U);
    std::memcpy(m.data, trig, P);
    for (const cv::Rect &r : rects)
        cv::rectangle(m, r, cv::Scalar(255, 255, 255), 1, 8, 0);
    std::memcpy(pres, m.data, P);
}

namespace {

const char *const kSuffix[6] = {"000_AvgImage", "00_PreTrigFrame", "0_TrigFrame", "02_OvrThe6Sigma", "3_OtsuThresholded",
                                "4_BubbleDetected"};

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

void makeDirsOrThrow(const std::string &dir)
{
    std::string part;
    if (!makeDirs(dir, &part))
        throw std::runtime_error("peek: cannot create " + part + ": " + strerror(errno));
}

void writeBytes(const std::string &path, const uint8_t *p, size_t n)
{
    bool opened;
    if (!writeFile(path, p, n, &opened))
        throw std::runtime_error(opened ? "peek: short write of " + path : "peek: cannot write " + path + ": " + strerror(errno));
}

std::string fileOf(const std::string &dir, const PeekStack &s, int which)
{
    return dir + "ev" + s.eventID + "_cam" + std::to_string(s.cam) + "_" + kSuffix[which] + ".png";
}

// The device buffers of the post-pass, kept over the sub-batches of a call
struct PeekBuffers {
    DeviceBuffer work;    // [n] D planes, then [n][2] peek planes, each at a multiple of 16
    DeviceBuffer meta;    // jobs | hist | items | rects | status
    PinnedBuffer h_meta;
};

// the PNG encoder with peek's own words for a batch that outgrows its regrown buffer
const Codec kPeekPng = [] {
    Codec c = kPng;
    c.outgrew = "peek: the encoded files outgrew their regrown buffer";
    return c;
}();

// pixels + src[f] for every f as PNG files in e (a first guess at their room: half a byte per pixel); a refused frame throws
void encode(EncodeBatch &e, const uint8_t *pixels, size_t pixelsBytes, const std::vector<uint64_t> &src, int W, int H, hipStream_t cs)
{
    double encode_s = 0, copy_s = 0; // (not reported)
    e.run(kPeekPng, pixels, pixelsBytes, src, W, H, src.size() * align16((size_t)W * H / 2 + 1024), cs, encode_s, copy_s);
    for (size_t f = 0; f < e.count(); ++f)
        if (e.file(f).status != 0)
            throw std::runtime_error("peek: abub_png_encode_dev refused a plane (status " + std::to_string(e.file(f).status) + ")");
}

} // namespace

void writePeekImages(int W, int H, int C, const uint8_t *d_frames, size_t framesBytes, const uint8_t *d_mu, const uint8_t *d_sigma6,
                     const std::vector<PeekStack> &stacks, const std::string &dir, bool gpu, size_t budgetBytes, int maxStacks,
                     int nthreads, hipStream_t cs, PeekStats &stats)
{
    if (stacks.empty())
        return;
    const size_t P = (size_t)W * H, P16 = align16(P);
    makeDirsOrThrow(dir);
    // per stack on the device: D and two planes, their files (at most abub_png_file_bound each, five of them) and the
    // encoder's scratch; the sub-batch takes what the budget allows
    const size_t perStack = 3 * P16 + 5 * align16(abub_png_file_bound(W, H)) + abub_png_encode_scratch_bytes(5, W, H) + 2048;
    size_t sub = std::max<size_t>(1, budgetBytes / perStack);
    if (maxStacks > 0)
        sub = std::min<size_t>(sub, (size_t)maxStacks);
    sub = std::min(sub, stacks.size());
    PeekBuffers b;
    EncodeBatch encF, encW; // the files that are alive at once: a sub-batch's frames and its planes
    std::atomic<long long> files{0}, bytes{0};
    auto put = [&](const std::string &path, const uint8_t *p, size_t n) {
        writeBytes(path, p, n);
        ++files;
        bytes += (long long)n;
    };

    // the model mean of every camera, one file's bytes per camera
    std::vector<std::vector<uint8_t>> muPng((size_t)C);
    if (gpu) {
        std::vector<uint64_t> src;
        for (int c = 0; c < C; ++c)
            src.push_back((uint64_t)c * P);
        EncodeBatch encMu; // (its files are copied: one per camera, written once per stack)
        encode(encMu, d_mu, (size_t)C * P, src, W, H, cs);
        for (int c = 0; c < C; ++c)
            muPng[c].assign(encMu.file(c).data, encMu.file(c).data + encMu.file(c).len);
    } else {
        std::vector<uint8_t> mu((size_t)C * P);
        HIPOK(hipMemcpyAsync(mu.data(), d_mu, mu.size(), hipMemcpyDeviceToHost, cs));
        HIPOK(hipStreamSynchronize(cs));
        for (int c = 0; c < C; ++c)
            if (!cv::pngHuffEncode(mu.data() + (size_t)c * P, W, H, muPng[c]))
                throw std::runtime_error("peek: cv::pngHuffEncode failed");
    }

    for (size_t i0 = 0; i0 < stacks.size(); i0 += sub) {
        const size_t n = std::min(sub, stacks.size() - i0);
        const PeekStack *S = stacks.data() + i0;
        // ---- D(trig, pre) and its histogram: one store-mode launch ------------------------------------------------------
        size_t nr = 0;
        for (size_t k = 0; k < n; ++k)
            nr += S[k].rects.size();
        const size_t jobsAt = 0, histAt = align16(n * sizeof(abub_job)), itemsAt = histAt + n * 256 * sizeof(uint32_t),
                     rectsAt = itemsAt + n * sizeof(abub_peek_item), statusAt = rectsAt + align16(nr * sizeof(abub_peek_rect)),
                     metaBytes = statusAt + n * sizeof(int32_t);
        b.meta.grow(metaBytes);
        b.h_meta.grow(metaBytes);
        const size_t planesAt = align16(n * P); // D planes packed at k * P, as K2 stores them; then the peek planes
        b.work.grow(planesAt + 2 * n * P16);
        uint8_t *hm = b.h_meta.get();
        abub_job *jobs = (abub_job *)(hm + jobsAt);
        for (size_t k = 0; k < n; ++k) {
            if (((size_t)std::max(S[k].trigFrame, S[k].preFrame) + 1) * P > framesBytes)
                throw std::runtime_error("peek: a trigger frame outside the batch");
            jobs[k].cur = S[k].trigFrame;
            jobs[k].ref = S[k].preFrame;
            jobs[k].model = (uint32_t)S[k].cam;
            jobs[k].out = (uint32_t)k;
        }
        HIPOK(hipMemcpyAsync(b.meta.get() + jobsAt, hm + jobsAt, n * sizeof(abub_job), hipMemcpyHostToDevice, cs));
        uint8_t *d_D = b.work.get();
        check(abub_diff_hist_dev(d_frames, d_sigma6, (const abub_job *)(b.meta.get() + jobsAt), (int)n, W, H,
                                 (uint32_t *)(b.meta.get() + histAt), d_D, 0, cs),
              "abub_diff_hist_dev");
        HIPOK(hipMemcpyAsync(hm + histAt, b.meta.get() + histAt, n * 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, cs));
        HIPOK(hipStreamSynchronize(cs));
        std::vector<int> cut(n);
        for (size_t k = 0; k < n; ++k)
            cut[k] = binarizeThresholdFromHist((const uint32_t *)(hm + histAt) + k * 256, P, S[k].loc_thres);

        if (gpu) {
            // ---- the two planes, then every file of the sub-batch --------------------------------------------------------
            abub_peek_item *items = (abub_peek_item *)(hm + itemsAt);
            abub_peek_rect *rects = (abub_peek_rect *)(hm + rectsAt);
            size_t r = 0;
            for (size_t k = 0; k < n; ++k) {
                items[k].diff = k * P;
                items[k].frame = (uint64_t)S[k].trigFrame * P;
                items[k].thr_out = 2 * k * P16; // (from the planes' part of the slab)
                items[k].pres_out = (2 * k + 1) * P16;
                items[k].thr = cut[k];
                items[k].rect_begin = (int32_t)r;
                items[k].rect_count = (int32_t)S[k].rects.size();
                items[k].reserved = 0;
                for (const cv::Rect &q : S[k].rects)
                    rects[r++] = abub_peek_rect{q.x, q.y, q.width, q.height};
            }
            HIPOK(hipMemcpyAsync(b.meta.get() + itemsAt, hm + itemsAt, statusAt - itemsAt, hipMemcpyHostToDevice, cs));
            check(abub_peek_planes_dev(d_D, n * P, d_frames, framesBytes, (const abub_peek_item *)(b.meta.get() + itemsAt), (int)n,
                                       nr ? (const abub_peek_rect *)(b.meta.get() + rectsAt) : nullptr, (int)nr, W, H,
                                       b.work.get() + planesAt, 2 * n * P16, (int32_t *)(b.meta.get() + statusAt), cs),
                  "abub_peek_planes_dev");
            std::vector<int32_t> status(n);
            HIPOK(hipMemcpyAsync(status.data(), b.meta.get() + statusAt, n * sizeof(int32_t), hipMemcpyDeviceToHost, cs));
            HIPOK(hipStreamSynchronize(cs));
            for (size_t k = 0; k < n; ++k)
                if (status[k] != 0)
                    throw std::runtime_error("peek: abub_peek_planes_dev refused an item (status " + std::to_string(status[k]) + ")");
            // the frames where they lie; D and the planes in the work slab
            std::vector<uint64_t> srcF, srcW;
            for (size_t k = 0; k < n; ++k) {
                srcF.push_back((uint64_t)S[k].preFrame * P);
                srcF.push_back((uint64_t)S[k].trigFrame * P);
                srcW.push_back(k * P);
                srcW.push_back(planesAt + 2 * k * P16);
                srcW.push_back(planesAt + (2 * k + 1) * P16);
            }
            encode(encF, d_frames, framesBytes, srcF, W, H, cs);
            encode(encW, b.work.get(), b.work.capacity(), srcW, W, H, cs);
            forEachTaskWith(
                nthreads, n, []() { return 0; },
                [&](int &, size_t k) {
                    put(fileOf(dir, S[k], 0), muPng[S[k].cam].data(), muPng[S[k].cam].size());
                    for (int j = 0; j < 2; ++j)
                        put(fileOf(dir, S[k], 1 + j), encF.file(2 * k + j).data, encF.file(2 * k + j).len);
                    for (int j = 0; j < 3; ++j)
                        put(fileOf(dir, S[k], 3 + j), encW.file(3 * k + j).data, encW.file(3 * k + j).len);
                });
        } else {
            // ---- the definition: D and the two frames back, planes and files on host threads ----------------------------
            std::vector<uint8_t> host(n * 3 * P);
            HIPOK(hipMemcpyAsync(host.data(), d_D, n * P, hipMemcpyDeviceToHost, cs));
            for (size_t k = 0; k < n; ++k) {
                HIPOK(hipMemcpyAsync(host.data() + (n + 2 * k) * P, d_frames + (size_t)S[k].preFrame * P, P, hipMemcpyDeviceToHost, cs));
                HIPOK(hipMemcpyAsync(host.data() + (n + 2 * k + 1) * P, d_frames + (size_t)S[k].trigFrame * P, P, hipMemcpyDeviceToHost, cs));
            }
            HIPOK(hipStreamSynchronize(cs));
            forEachTaskWith(
                nthreads, n, []() { return 0; },
                [&](int &, size_t k) {
                    const uint8_t *D = host.data() + k * P, *pre = host.data() + (n + 2 * k) * P, *trig = pre + P;
                    std::vector<uint8_t> planes(2 * P), png;
                    peekPlanesHost(D, trig, W, H, cut[k], S[k].rects, planes.data(), planes.data() + P);
                    const uint8_t *img[6] = {nullptr, pre, trig, D, planes.data(), planes.data() + P};
                    put(fileOf(dir, S[k], 0), muPng[S[k].cam].data(), muPng[S[k].cam].size());
                    for (int j = 1; j < 6; ++j) {
                        if (!cv::pngHuffEncode(img[j], W, H, png))
                            throw std::runtime_error("peek: cv::pngHuffEncode failed");
                        put(fileOf(dir, S[k], j), png.data(), png.size());
                    }
                });
        }
        ++stats.subBatches;
    }
    stats.stacks += (long long)stacks.size();
    stats.files += files;
    stats.bytes += bytes;
}

} // namespace abub
