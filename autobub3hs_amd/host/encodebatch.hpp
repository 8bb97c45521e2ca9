// encodebatch.hpp -- frames that are resident on the device, written as FILES by one of the GPU encoders (abub_abf_encode_dev,
// abub_png_encode_dev): the writing counterpart of FileBatch (framefiles.hpp), shared by the device routes of repack and
// unpack (repack.cpp) and by the peek images (peek.cpp).  Codec is what differs between the two formats; EncodeBatch is the
// one way a route calls an encoder: the call's buffers, its redo when the files outgrow their room, the files back on the
// host.  Internal to the host library.
#ifndef ABUB3HS_ENCODEBATCH_HPP
#define ABUB3HS_ENCODEBATCH_HPP

#include <cstdint>
#include <cstring>
#include <vector>

#include "abub_hip.h"
#include "cvlite.hpp"
#include "devctx.hpp"
#include "holders.hpp"
#include "pipeline.hpp"

namespace abub {

// The frame format a run is rewritten in: what differs between --repack and --unpack
struct Codec {
    const char *what;                                                           // "repack" / "unpack", in messages
    bool (*encode)(const uchar *pixels, int W, int H, std::vector<uchar> &out); // on a host thread
    int (*encodeDev)(const uint8_t *, size_t, const uint64_t *, int, int, int, uint8_t *, size_t, abub_abf_file *, uint64_t *, void *,
                     size_t, void *);
    size_t (*scratchBytes)(int nframes, int W, int H);
    const char *devName, *noDevice, *outgrew; // the device entry's name; what requireDevice adds to its message; the
                                              // message when a batch's files do not fit their regrown buffer
};
inline const Codec kPacked = {"repack", cv::abfEncode, abub_abf_encode_dev, abub_abf_encode_scratch_bytes, "abub_abf_encode_dev",
                              "; without --repack-gpu the run is repacked on the host",
                              "repack: the packed files of a batch outgrew their buffer twice"};
inline const Codec kPng = {"unpack", cv::pngHuffEncode, abub_png_encode_dev, abub_png_encode_scratch_bytes, "abub_png_encode_dev",
                           "; without --unpack-gpu the run is unpacked on the host",
                           "unpack: the PNG files of a batch outgrew their buffer twice"};

// One call of a codec's device encoder and its files, which stay on the host until the next call
struct EncodeBatch {
    struct File {
        int32_t status;      // 0, ABUB_ABF_ENC_E_SRC, ABUB_ABF_ENC_E_CAP: what becomes of a refused frame is the caller's policy
        const uint8_t *data; // `len` bytes in pinned memory (status 0)
        uint32_t len;
    };
    size_t count() const { return n_; }
    File file(size_t f) const
    {
        const abub_abf_file &r = records()[f];
        return File{r.status, h_out.get() + r.off, r.len};
    }

    // The frames of W x H at pixels + src[f] (pixelsBytes: what may be read there) into files that stay ON THE DEVICE: file f
    // is record(f).len bytes at deviceFiles() + record(f).off (a multiple of 16), of deviceBytes() in all, until the next
    // call; only the records come back.  The meta buffer is [src | records | total]; the files go into `out`, at least
    // `firstReserve` bytes of it, and when they outgrow it the list grows to the true total and the call is redone, once
    // (Growable::fit; codec.outgrew is thrown after that).  Queued on `cs` and waited for.  The time, with every allocation,
    // is added to encode_s.
    void encode(const Codec &codec, const uint8_t *pixels, size_t pixelsBytes, const std::vector<uint64_t> &src, int W, int H,
                size_t firstReserve, hipStream_t cs, double &encode_s)
    {
        const double t0 = nowMs();
        const size_t n = n_ = src.size();
        bytes_ = 0;
        if (!n)
            return;
        const size_t metaBytes = n * (sizeof(uint64_t) + sizeof(abub_abf_file)) + sizeof(uint64_t);
        h_meta.grow(metaBytes);
        d_meta.grow(metaBytes);
        scratch.grow(codec.scratchBytes((int)n, W, H));
        std::memcpy(h_meta.get(), src.data(), n * sizeof(uint64_t));
        HIPOK(hipMemcpyAsync(d_meta.get(), h_meta.get(), n * sizeof(uint64_t), hipMemcpyHostToDevice, cs));
        abub_abf_file *d_rec = (abub_abf_file *)(d_meta.get() + n * sizeof(uint64_t));
        uint64_t bytes = 0;
        out.newBatch();
        out.reserve(firstReserve);
        do {
            check(codec.encodeDev(pixels, pixelsBytes, (const uint64_t *)d_meta.get(), (int)n, W, H, out.d.get(), out.cap(), d_rec,
                                  (uint64_t *)(d_rec + n), scratch.get(), scratch.capacity(), cs),
                  codec.devName);
            HIPOK(hipMemcpyAsync(h_meta.get() + n * sizeof(uint64_t), d_rec, n * sizeof(abub_abf_file) + sizeof(uint64_t),
                                 hipMemcpyDeviceToHost, cs));
            HIPOK(hipStreamSynchronize(cs));
            std::memcpy(&bytes, records() + n, sizeof bytes);
        } while (!out.fit((size_t)bytes, codec.outgrew));
        bytes_ = (size_t)bytes;
        encode_s += (nowMs() - t0) * 1e-3;
    }
    struct Record {
        int32_t status;
        uint64_t off;
        uint32_t len;
    };
    Record record(size_t f) const { return Record{records()[f].status, records()[f].off, records()[f].len}; }
    const uint8_t *deviceFiles() const { return out.d.get(); }
    size_t deviceBytes() const { return bytes_; }

    // encode(), then the files to the host (file(f)); the time of their copy is added to copy_s
    void run(const Codec &codec, const uint8_t *pixels, size_t pixelsBytes, const std::vector<uint64_t> &src, int W, int H,
             size_t firstReserve, hipStream_t cs, double &encode_s, double &copy_s)
    {
        encode(codec, pixels, pixelsBytes, src, W, H, firstReserve, cs, encode_s);
        if (!n_)
            return;
        double t0 = nowMs();
        h_out.grow(bytes_); // (an allocation: encode_s, as ever)
        encode_s += (nowMs() - t0) * 1e-3;
        t0 = nowMs();
        HIPOK(hipMemcpyAsync(h_out.get(), out.d.get(), bytes_, hipMemcpyDeviceToHost, cs));
        HIPOK(hipStreamSynchronize(cs));
        copy_s += (nowMs() - t0) * 1e-3;
    }

private:
    const abub_abf_file *records() const { return (const abub_abf_file *)(h_meta.get() + n_ * sizeof(uint64_t)); }
    // The files of a call on the device: a list under the one redo rule (Growable, holders.hpp: newBatch / reserve / fit).
    // Not a GrowList, whose pinned mirror is as large as the list: the files' pinned copy takes what a call wrote (the peek
    // images, whose three batches are made anew for every batch of a run, spent 4 % more time with mirrors of full size)
    struct DeviceList final : Growable {
        DeviceList() : Growable(4096, SIZE_MAX) {}
        DeviceBuffer d;

    private:
        void allocateEntries(size_t n) override { d.allocate(n + 256); }
    } out;
    PinnedBuffer h_meta, h_out; // (h_out: the files on the host, as many bytes as a call wrote)
    DeviceBuffer d_meta, scratch;
    size_t n_ = 0, bytes_ = 0;
};

} // namespace abub
#endif
