// repack.cpp -- a run rewritten with its frames in the packed format (cv::abfEncode, DESIGN section 3, "Packed frames"): abub3hs --repack.
// No analysis.  Everything is read through the Parser interface, so a directory and a zip archive repack alike; the result
// is a directory or, with an ArchiveTarget (--archive), the one canonical archive of zipwrite.hpp with the same files as its
// entries (ArchiveOut below: on the device route the resident files become entries on the device, abub_zip_pack_dev, and a
// batch goes to disk in one write).  RepackRun is host only (cv::imdecode + cv::abfEncode on the pool's threads); RepackRunDevice
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
#include "zipwrite.hpp"

namespace abub {

namespace {

// what became of one frame
struct Outcome {
    bool ok = false, packed = false;
    long long in = 0, out = 0; // of a packed frame: the source file's bytes, the packed file's
};

// Where a file's bytes go: the file `path`, or, for the archive, `keep` until the batch's segment is formed
struct Sink {
    std::string path;
    std::vector<unsigned char> *keep = nullptr;
    bool put(const unsigned char *data, size_t n) const
    {
        if (!keep)
            return writeFile(path, data, n);
        keep->assign(data, data + n);
        return true;
    }
};

// The bytes of a source file on a host thread: decoded at whatever size the file has and packed, or, where they do not
// decode, copied as they are (the file stays undecodable)
Outcome packBytes(const Codec &codec, const unsigned char *data, size_t size, const Sink &to)
{
    static thread_local std::vector<unsigned char> packed;
    Outcome o;
    const cv::Mat m = size ? cv::imdecode(data, size, 0) : cv::Mat();
    o.packed = !m.empty() && codec.encode(m.data, m.cols, m.rows, packed);
    o.ok = o.packed ? to.put(packed.data(), packed.size()) : to.put(data, size);
    o.in = (long long)size;
    o.out = (long long)packed.size();
    return o;
}

// One frame read through the parser and packed on this thread
Outcome hostFrame(const Codec &codec, Parser &p, const std::string &ev, const std::string &name, const Sink &to)
{
    static thread_local std::vector<unsigned char> file;
    const long long size = p.GetImageFileSize(ev, name);
    if (size < 0 || size >= ((long long)1 << 30))
        return Outcome();
    file.resize((size_t)size);
    if (size && p.ReadImageFile(ev, name, file.data(), file.size()) != size)
        return Outcome();
    return packBytes(codec, file.data(), file.size(), to);
}

using Task = FrameTask;

// The part of a repack that is not its frames
struct Plan {
    std::string dstRunDir;
    std::vector<std::string> events, dirs; // dirs[e]: where the frames of events[e] go
    std::vector<Task> tasks;               // every frame, in event, camera and frame order
    bool failed = false;                   // a directory or the event file could not be written
    std::string pathOf(const Task &t) const { return dirs[t.ev] + "/" + t.name; }
    // --archive: the archive, the run's ID, the event file's bytes, and per event the names of its directory entries
    // (<run>/<event>/, then one per level of the image folder; the frames' names begin with the last of them)
    bool archive = false;
    std::string zipPath, runId, eventText;
    std::vector<std::vector<std::string>> dirEntries;
    std::string entryOf(const Task &t) const { return dirEntries[t.ev].back() + t.name; }
};

// does `path` name the file or directory `other` (both exist)?
bool sameInode(const std::string &path, const std::string &other)
{
    struct stat a, b;
    return !path.empty() && !other.empty() && stat(path.c_str(), &a) == 0 && stat(other.c_str(), &b) == 0 && a.st_dev == b.st_dev &&
           a.st_ino == b.st_ino;
}

Plan planRun(const Codec &codec, Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir_,
             const std::string &imageFolder, int numCams, const ArchiveTarget &archive)
{
    Plan pl;
    pl.dstRunDir = trimSlashes(dstRunDir_);
    const std::string &dstRunDir = pl.dstRunDir;
    const size_t slash = dstRunDir.find_last_of('/');
    pl.runId = slash == std::string::npos ? dstRunDir : dstRunDir.substr(slash + 1);
    pl.archive = archive.on;
    pl.zipPath = dstRunDir + ".zip";
    // the files keep their names: written into the source run they would replace the frames they are read from (and an
    // archive renamed over the archive that is being read would replace all of them)
    if (!archive.on && sameInode(srcRunDir, dstRunDir))
        throw std::runtime_error(std::string(codec.what) + ": " + dstRunDir + " is the run that is being read");
    if (archive.on && sameInode(archive.srcArchive, pl.zipPath))
        throw std::runtime_error(std::string(codec.what) + ": " + pl.zipPath + " is the run that is being read");
    pl.events = sortedEvents(*parser);
    const std::vector<std::string> &events = pl.events;
    pl.dirs.resize(events.size());
    pl.dirEntries.resize(events.size());
    for (size_t e = 0; e < events.size(); ++e) {
        if (archive.on) {
            std::string name = pl.runId + "/" + events[e] + "/";
            pl.dirEntries[e].push_back(name);
            for (size_t at = 0; at < imageFolder.size();) { // one entry per level of the image folder
                const size_t to = std::min(imageFolder.find('/', at), imageFolder.size());
                if (to > at) {
                    name += imageFolder.substr(at, to - at) + "/";
                    pl.dirEntries[e].push_back(name);
                }
                at = to + 1;
            }
        } else {
            std::string &dir = pl.dirs[e];
            dir = trimSlashes(dstRunDir + "/" + events[e] + "/" + imageFolder);
            for (size_t at; (at = dir.find("//")) != std::string::npos;)
                dir.erase(at, 1);
            if (!makeDirs(dir)) {
                pl.failed = true;
                continue;
            }
        }
        appendEventFrames(*parser, events[e], e, numCams, pl.tasks);
    }

    // ---- the run's event file: the source's bytes where there is such a file, else one line per listed event ------------
    if (archive.on || makeDirs(dstRunDir)) {
        std::ifstream in(srcRunFile, std::ios::binary);
        std::ostringstream text;
        if (!srcRunFile.empty() && in)
            text << in.rdbuf();
        else {
            std::vector<std::string> listed;
            parser->GetRunFileInfo(listed);
            for (const std::string &ev : listed) // (the eleven columns GetRunFileInfo reads; the second is the event)
                text << pl.runId << ' ' << ev << " 0 0 0 0 0 0 0 0 0\n";
        }
        pl.eventText = text.str();
        const std::string &s = pl.eventText;
        if (!archive.on && !s.empty() && !writeFile(dstRunDir + "/" + pl.runId + ".txt", (const unsigned char *)s.data(), s.size()))
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

// The archive of a run (--archive) as it grows: <run>/ and the event file first, then batch by batch one SEGMENT of whole
// entries -- the frames that were written, in task order, each event's directory entries in front of its first frame (or
// where its frames would be) -- laid out from the archive offset reached so far, filled, and written with one write.  An
// entry's bytes are the host's (put into the segment here, with their CRC) or lie on the device: those entries are formed
// there (DevicePack below) and only hand their CRC over.
struct ArchiveOut {
    struct Slot {
        size_t entry;
        const unsigned char *data; // the host's bytes (an empty entry has none)
        bool onDevice;             // the device forms the entry
    };
    ZipWriter zw;
    const Plan &pl;
    size_t nextEvent = 0; // the events in front of it have their directory entries
    std::vector<Slot> slots;
    uint64_t segStart = 0;

    explicit ArchiveOut(const Plan &plan) : zw(plan.zipPath), pl(plan)
    {
        zw.add(pl.runId + "/", nullptr, 0);
        if (!pl.eventText.empty())
            zw.add(pl.runId + "/" + pl.runId + ".txt", (const unsigned char *)pl.eventText.data(), pl.eventText.size());
    }
    void begin()
    {
        slots.clear();
        segStart = zw.planned();
    }
    // the directory entries of the events in front of event `upTo`
    void dirs(size_t upTo)
    {
        for (; nextEvent < upTo; ++nextEvent)
            for (const std::string &name : pl.dirEntries[nextEvent])
                slots.push_back(Slot{zw.plan(name, 0), nullptr, false});
    }
    // the next frame (its event's directories first); returns the entry's index
    size_t frame(const Task &t, const unsigned char *data, size_t len, bool onDevice = false)
    {
        dirs(t.ev + 1);
        slots.push_back(Slot{zw.plan(pl.entryOf(t), len), data, onDevice});
        return slots.back().entry;
    }
    size_t segBytes() const { return (size_t)(zw.planned() - segStart); }
    // the host's entries into the segment (seg[0] is the archive's byte segStart), each with its CRC, on up to `nthreads`
    // threads (an entry is one thread's), then the write
    void flush(unsigned char *seg, int nthreads = 1)
    {
        forEachTaskWith(
            nthreads, slots.size(), []() { return 0; },
            [&](int &, size_t k) {
                const Slot &s = slots[k];
                if (!s.onDevice)
                    zw.putEntry(s.entry, s.data, seg + (zw.entry(s.entry).at.off - segStart));
            });
        zw.write(seg, segBytes());
    }
    void finish(RepackStats &st)
    {
        begin();
        dirs(pl.events.size()); // (events without a frame behind the last one that has any)
        std::vector<unsigned char> seg(segBytes());
        flush(seg.data());
        zw.finish();
        st.archiveBytes = (long long)zw.bytes();
        st.archiveEntries = (long long)zw.entries();
    }
};

// frames per batch at most: ABUB_REPACK_BATCH=n (a test knob) can only lower it
size_t batchKnob(size_t perBatch)
{
    if (const char *e = getenv("ABUB_REPACK_BATCH")) {
        const long v = atol(e);
        if (v > 0)
            perBatch = std::min(perBatch, (size_t)v);
    }
    return perBatch;
}

void hostFrames(const Codec &codec, Parser *parser, const Plan &pl, int nthreads, Tally &tally, ArchiveOut *ar)
{
    if (!ar) {
        forEachTask(parser, nthreads, pl.tasks.size(), [&](Parser &p, size_t i) {
            const Task &t = pl.tasks[i];
            tally.add(hostFrame(codec, p, pl.events[t.ev], t.name, Sink{pl.pathOf(t)}));
        });
        return;
    }
    // the archive: the pool's threads pack as above, a bounded batch at a time (8 files per thread are kept at most), and
    // the files are appended in task order, whichever thread finished first
    const size_t perBatch = batchKnob((size_t)8 * std::max(1, nthreads));
    std::vector<std::vector<unsigned char>> kept(perBatch);
    std::vector<Outcome> done(perBatch);
    std::unique_ptr<unsigned char[]> seg; // (grown, never cleared: every byte of a segment is an entry's)
    size_t segCap = 0;
    for (size_t i0 = 0; i0 < pl.tasks.size(); i0 += perBatch) {
        const size_t n = std::min(perBatch, pl.tasks.size() - i0);
        forEachTask(parser, nthreads, n, [&](Parser &p, size_t i) {
            const Task &t = pl.tasks[i0 + i];
            done[i] = hostFrame(codec, p, pl.events[t.ev], t.name, Sink{std::string(), &kept[i]});
        });
        ar->begin();
        for (size_t i = 0; i < n; ++i) {
            tally.add(done[i]);
            if (done[i].ok)
                ar->frame(pl.tasks[i0 + i], kept[i].data(), kept[i].size());
        }
        if (ar->segBytes() > segCap) {
            segCap = ar->segBytes() + ar->segBytes() / 4;
            seg.reset(new unsigned char[segCap]);
        }
        ar->flush(seg.get(), nthreads);
    }
}

// The device's part of a segment: the batch's files that are resident on the device (EncodeBatch::encode) become whole
// entries in a device buffer laid out like the segment (abub_zip_pack_dev), and the segment comes to the host in one copy.
// The device buffer begins at the multiple of 16 at or below the segment's archive offset, so that the data of every
// entry, which lies at a multiple of 16 in the archive, does so in the buffer; the host's entries fill the rest.
struct DevicePack {
    struct Item {
        size_t entry, file; // of the archive; of the encode batch
    };
    std::vector<Item> items;
    std::vector<abub_zip_item> desc;
    std::string names;
    PinnedBuffer h_up, h_res, h_seg;
    DeviceBuffer d_up, d_res, d_seg;

    void begin() { items.clear(); }
    // Packs, copies the segment to the host (h_seg: its first byte is the archive's byte ar.segStart) and hands the CRCs to the
    // archive.  Queued on `cs` and waited for
    void run(ArchiveOut &ar, const EncodeBatch &enc, hipStream_t cs, RepackStats &st)
    {
        const size_t n = items.size(), segBytes = ar.segBytes(), lead = (size_t)(ar.segStart & 15);
        h_seg.grow(segBytes + 16);
        if (!n)
            return;
        double t0 = nowMs();
        desc.resize(n);
        names.clear();
        for (size_t k = 0; k < n; ++k) {
            const ZipWriter::Entry &e = ar.zw.entry(items[k].entry);
            const EncodeBatch::Record r = enc.record(items[k].file);
            abub_zip_item &d = desc[k];
            d.src = r.off;
            d.dst = e.at.off - ar.segStart + lead;
            d.len = e.at.len;
            d.name = (uint32_t)names.size();
            d.name_len = e.at.nameLen;
            d.extra_len = e.at.extraLen;
            d.reserved = 0;
            names += e.name;
        }
        const size_t descBytes = n * sizeof(abub_zip_item), resBytes = n * (sizeof(uint32_t) + sizeof(int32_t));
        h_up.grow(descBytes + names.size());
        d_up.grow(descBytes + names.size());
        h_res.grow(resBytes);
        d_res.grow(resBytes);
        d_seg.grow(lead + segBytes + 16);
        std::memcpy(h_up.get(), desc.data(), descBytes);
        std::memcpy(h_up.get() + descBytes, names.data(), names.size());
        HIPOK(hipMemcpyAsync(d_up.get(), h_up.get(), descBytes + names.size(), hipMemcpyHostToDevice, cs));
        uint32_t *d_crc = (uint32_t *)d_res.get();
        int32_t *d_status = (int32_t *)(d_crc + n);
        check(abub_zip_pack_dev(enc.deviceFiles(), enc.deviceBytes(), (const abub_zip_item *)d_up.get(), (int)n, d_up.get() + descBytes,
                                names.size(), d_seg.get(), lead + segBytes, d_crc, d_status, cs),
              "abub_zip_pack_dev");
        HIPOK(hipMemcpyAsync(h_res.get(), d_res.get(), resBytes, hipMemcpyDeviceToHost, cs));
        HIPOK(hipStreamSynchronize(cs));
        st.pack_s += (nowMs() - t0) * 1e-3;
        t0 = nowMs();
        HIPOK(hipMemcpyAsync(h_seg.get(), d_seg.get() + lead, segBytes, hipMemcpyDeviceToHost, cs));
        HIPOK(hipStreamSynchronize(cs));
        st.copy_s += (nowMs() - t0) * 1e-3;
        const uint32_t *crc = (const uint32_t *)h_res.get();
        const int32_t *status = (const int32_t *)(crc + n);
        for (size_t k = 0; k < n; ++k) {
            if (status[k] != 0)
                throw std::runtime_error("abub_zip_pack_dev refused the entry " + ar.zw.entry(items[k].entry).name);
            ar.zw.setCrc(items[k].entry, crc[k]);
        }
    }
};

// The device route: the frames in batches of at most 4 per CU (ABUB_REPACK_BATCH=n, a test knob: of at most n, never more).  Per batch: the pool reads the files into a pinned buffer
// (and packs, on the spot, what is no file for the GPU decoders: a frame it had to decode itself, a frame of another size,
// a file that does not decode); upload; both decoders into a slab; the codec's device encoder over the frames that are in place
// (EncodeBatch, encodebatch.hpp: its files come back in pinned memory); the pool writes the files.  With the archive the
// files of the encoder stay on the device and the batch becomes one segment (ArchiveOut, DevicePack): layout on the host,
// abub_zip_pack_dev, one copy to the host, the host's own entries, one write.
void deviceFrames(const Codec &codec, Parser *parser, const Plan &pl, int nthreads, int device, int W, int H, Tally &tally,
                  ArchiveOut *ar)
{
    RepackStats &st = tally.st;
    HIPOK(hipSetDevice(device));
    const size_t perBatch = batchKnob(framesPerBatch(device)); // (the knob: several batches of a small run)
    const size_t P = (size_t)W * H;
    FileBatch B; // the batch's files, the decoders' scratch, the slab of decoded frames (frame i at i * P)
    std::vector<FileTask> &ft = B.ft;
    EncodeBatch enc; // the packed files of a batch
    DevicePack pack;
    std::vector<std::vector<unsigned char>> kept(ar ? perBatch : 0); // the archive: the files the host's threads made
    std::vector<unsigned char> ok(ar ? perBatch : 0);                // ... and whether frame i was written
    Stream stream;
    hipStream_t cs = stream.get();
    B.sizer.reset(parser->clone());

    for (size_t i0 = 0; i0 < pl.tasks.size(); i0 += perBatch) {
        const size_t n = std::min(perBatch, pl.tasks.size() - i0);
        std::fill(ok.begin(), ok.end(), 0);
        // where a host thread puts the file of frame i
        const auto sinkOf = [&](size_t i) { return ar ? Sink{std::string(), &kept[i]} : Sink{pl.pathOf(pl.tasks[i0 + i])}; };
        const auto settled = [&](size_t i, const Outcome &o, bool onGpu = false) {
            if (ar)
                ok[i] = o.ok;
            tally.add(o, onGpu);
        };
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
                o.ok = o.packed && sinkOf(i).put(packed.data(), packed.size());
                o.in = f.size;
                o.out = (long long)packed.size();
                settled(i, o);
            } else if (f.read) // another size, or a file that does not decode
                settled(i, packBytes(codec, B.h_files.get() + f.off, (size_t)f.size, sinkOf(i)));
            else               // a file the parser does not hand out in one piece
                settled(i, hostFrame(codec, p, ev, t.name, sinkOf(i)));
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

        // ---- encode, and copy back unless the files become archive entries on the device (a packed frame is about the size
        // of its PNG) ------------------------------------------------------------------------------------------------------
        const size_t ng = src.size();
        if (ar)
            enc.encode(codec, B.slab.get(), n * P, src, W, H, B.total + 64 * ng, cs, st.encode_s);
        else
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
                settled(i, packBytes(codec, B.h_files.get() + ft[i].off, (size_t)ft[i].size, sinkOf(i)));
                return;
            }
            Outcome o;
            o.packed = true;
            o.in = ft[i].size;
            if (ar) { // (the file stays where it is)
                const EncodeBatch::Record r = enc.record(fileOf[i]);
                o.ok = r.status == 0;
                o.out = r.len;
            } else {
                const EncodeBatch::File r = enc.file(fileOf[i]);
                o.ok = r.status == 0 && writeFile(pl.pathOf(t), r.data, r.len);
                o.out = r.len;
            }
            settled(i, o, true);
        });
        if (ar) { // the segment: its layout, the device's entries, the copy, the host's entries, the write
            ar->begin();
            pack.begin();
            for (size_t i = 0; i < n; ++i) {
                if (!ok[i])
                    continue; // (not written: no entry)
                const bool onDevice = ft[i].state != FileTask::Other && fileOf[i] != SIZE_MAX;
                if (onDevice)
                    pack.items.push_back(DevicePack::Item{ar->frame(pl.tasks[i0 + i], nullptr, enc.record(fileOf[i]).len, true), fileOf[i]});
                else
                    ar->frame(pl.tasks[i0 + i], kept[i].data(), kept[i].size());
            }
            st.write_s += (nowMs() - t0) * 1e-3;
            pack.run(*ar, enc, cs, st);
            t0 = nowMs();
            ar->flush(pack.h_seg.get(), nthreads);
        }
        st.write_s += (nowMs() - t0) * 1e-3;
        ++st.batches;
    }
}

int repackRun(const Codec &codec, Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir,
              const std::string &imageFolder, int numCams, int nthreads, int device, RepackStats *stats, const ArchiveTarget &archive)
{
    const double t0 = nowMs();
    RepackStats st;
    if (device >= 0) // (before anything is written)
        requireDevice(device, codec.what, codec.noDevice);
    const Plan pl = planRun(codec, parser, srcRunDir, srcRunFile, dstRunDir, imageFolder, numCams, archive);
    st.events = (int)pl.events.size();
    Tally tally{st, {}};
    std::unique_ptr<ArchiveOut> ar;
    if (archive.on) {
        const size_t slash = pl.zipPath.find_last_of('/');
        if (slash != std::string::npos && slash > 0)
            makeDirs(pl.zipPath.substr(0, slash)); // (where it cannot be made the archive cannot be opened either)
        ar.reset(new ArchiveOut(pl));
    }
    int W = 0, H = 0;
    if (device >= 0 && firstFrameSize(parser, pl.events, pl.tasks, W, H) && decodersTakeWidth(W)) {
        st.device = device;
        st.W = W;
        st.H = H;
        deviceFrames(codec, parser, pl, nthreads, device, W, H, tally, ar.get());
    } else
        hostFrames(codec, parser, pl, nthreads, tally, ar.get());
    if (ar)
        ar->finish(st);
    st.total_s = (nowMs() - t0) * 1e-3;
    if (stats)
        *stats = st;
    return pl.failed || st.failed ? 1 : 0;
}

} // namespace

int RepackRun(Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir,
              const std::string &imageFolder, int numCams, int nthreads, RepackStats *stats, const ArchiveTarget &archive)
{
    return repackRun(kPacked, parser, srcRunDir, srcRunFile, dstRunDir, imageFolder, numCams, nthreads, -1, stats, archive);
}

int RepackRunDevice(Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir,
                    const std::string &imageFolder, int numCams, int nthreads, int device, RepackStats *stats,
                    const ArchiveTarget &archive)
{
    if (device < 0)
        throw std::runtime_error("repack: no such HIP device: " + std::to_string(device));
    return repackRun(kPacked, parser, srcRunDir, srcRunFile, dstRunDir, imageFolder, numCams, nthreads, device, stats, archive);
}

int UnpackRun(Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir,
              const std::string &imageFolder, int numCams, int nthreads, RepackStats *stats, const ArchiveTarget &archive)
{
    return repackRun(kPng, parser, srcRunDir, srcRunFile, dstRunDir, imageFolder, numCams, nthreads, -1, stats, archive);
}

int UnpackRunDevice(Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir,
                    const std::string &imageFolder, int numCams, int nthreads, int device, RepackStats *stats,
                    const ArchiveTarget &archive)
{
    if (device < 0)
        throw std::runtime_error("unpack: no such HIP device: " + std::to_string(device));
    return repackRun(kPng, parser, srcRunDir, srcRunFile, dstRunDir, imageFolder, numCams, nthreads, device, stats, archive);
}

} // namespace abub
