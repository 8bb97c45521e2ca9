// runbatch.hpp -- a whole run from a Parser (directory tree or zip archive) through the batched GPU pipeline:
// the replacement of the reference's detect loop (AutoBubStart3.cpp:338-388) when the per-event drop-in path is
// not asked for.  Events are decoded on host threads straight into pinned buffers, uploaded batch by batch
// (decode of batch b+1 overlaps the GPU work of batch b), analysed by RunPipeline, and written through
// OutputWriter in event order.  With several GPUs the batches are dealt round-robin to one worker thread per GPU.
#ifndef ABUB3HS_RUNBATCH_HPP
#define ABUB3HS_RUNBATCH_HPP

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include <memory>

class Parser;
class Trainer;

namespace abub {

struct BatchedRunOptions {
    int ngpus = 1;                  // worker threads, one per GPU: device (firstDevice + g) % hipGetDeviceCount
    int firstDevice = 0;
    int hostThreads = 16;           // state machines / contour tracing per worker (RunPipeline's pool)
    int decodeThreads = 16;         // PNG / BMP decode threads, shared by the workers
    size_t batchBytes = (size_t)3 << 30; // frame bytes per batch; each worker holds two pinned and two HBM slabs of it
    int shardRank = 0, shardWorld = 1;   // this process takes events with index % shardWorld == shardRank
    std::string maskDir;
    int gpuDecode = -1;             // PNG frames decoded on the GPU (abub_png_decode_dev): 1 on, 0 off (host threads decode),
                                    // -1 = on where the parser hands out the files and the frames are 8-bit grey / palette
                                    // PNGs of a width the kernels take (ABUB_GPU_DECODE=0/1 overrides)
    // RunCampaign only
    std::string outDir;             // where every run's abub3hs_<run>.txt goes (ends with '/')
    int trainOnGpu = 1;             // 1: TrainOnDevice (the host Trainer where it declines a run); 0: the host Trainer
    int perEventThreads = 16;       // threads of the per-event loop of a run the batched path declines
    // abub3hs --peek DIR: the six DebugPeek images of every accepted stack (staged 0, at least one bubble) written to
    // <peekDir>/<run_number>/ by a post-pass per batch (peek.hpp); empty = off: no launch, no copy, no file
    std::string peekDir;
    int peekGpu = -1;               // 1: abub_peek_planes_dev + abub_png_encode_dev; 0: the host route, which is the definition;
                                    // -1: 1 unless ABUB_PEEK_GPU=0
    int peekMaxStacks = 0;          // stacks per sub-batch of the post-pass at most (0: what batchBytes / 8 allows;
                                    // ABUB_PEEK_BATCH=n, a test knob, overrides)
};

struct BatchedRunStats {
    double list_s = 0, decode_s = 0, gpu_s = 0, write_s = 0, total_s = 0; // decode/gpu: summed over batches (they overlap)
    long long frames = 0, framesFailed = 0;
    long long bellowsVetoed = 0; // stacks whose bellows-movement veto ran inside the batch (pipeline veto round)
    long long framesGpuDecoded = 0, framesHostDecoded = 0; // of `frames`: by the GPU decoders / by a host thread
    long long framesGpuUnpacked = 0;                       // of framesGpuDecoded: packed frames, by abub_abf_decode_dev
    long long framesGpuBmp = 0;                            // of framesGpuDecoded: BMP frames, by abub_bmp_decode_dev
    long long framesGpuUnzipped = 0;                       // ABUB_GPU_UNZIP=1: archive entries whose zip layer abub_unzip_dev inflated
    double unzip_s = 0;                                    // ... of decode_s: upload of the compressed bytes, kernels, copy back, wait
    double gpudecode_s = 0;                                // upload of the files + the decode kernels, summed over batches
    int events = 0, batches = 0, eventsPerBatch = 0, W = 0, H = 0, Fmax = 0, gpus = 0;
    long long peekStacks = 0, peekFiles = 0, peekBytes = 0; // peekDir: accepted stacks, files written, their bytes
    int peekGpu = -1, peekSubBatches = 0;                   // ... the route taken (-1: off, 0: host, 1: GPU), sub-batches of the post-pass
    double peek_s = 0;                                      // ... of gpu_s: the post-pass
};

// Detects every event of `EventList` (already in output order) with the trained `Trainers` (one per camera) and
// appends the blocks to <out_dir>abub3hs_<run_number>.txt.  Returns 0; or a positive code when the batched path
// cannot take this run (different image sizes per camera, no frames, ...) and nothing was written -- the caller
// then runs the per-event loop; throws std::runtime_error on GPU / IO failures.
int RunBatched(Parser *parser, const std::vector<std::string> &EventList, const std::vector<Trainer *> &Trainers,
               int numCams, const std::string &out_dir, const std::string &run_number, int frameOffset,
               const BatchedRunOptions &opt, BatchedRunStats *stats, std::string *why);

// The per-event loop of the reference's main program (AutoBubStart3.cpp:338-388): one analyzer per (event, camera), events on
// `nthreads` threads, blocks appended to <out_dir>abub3hs_<run_number>.txt in event order.  eventUser >= 0: only the event
// at that index; debugMode: the CLI's --debug digits.  The CLI's -e / --debug / --per-event path and the fallback of a
// run that RunBatched declines.
void RunPerEvent(Parser *parser, const std::vector<std::string> &EventList, const std::vector<Trainer *> &Trainers,
                 int numCams, const std::string &eventDir, const std::string &out_dir, const std::string &run_number,
                 int frameOffset, const std::string &maskDir, int nthreads, int eventUser, int debugMode, int shardRank,
                 int shardWorld);

// The "batched detect: ..." line of a run
void PrintBatchedLine(const BatchedRunStats &bs);

// One run of a campaign: what the CLI computes from -d / -D and the run ID (AutoBubStart3.cpp:212-245)
struct RunSpec {
    std::string runId, eventDir, imageFormat, imageFolder;
    int frameOffset = 30, numCams = 4;
    bool zipped = false;
};

struct DeviceTrainBuffers;

struct RepackStats {
    int events = 0;
    long long packed = 0, copied = 0, failed = 0; // frames written in the packed format / copied as they are / not written
    long long bytesIn = 0, bytesOut = 0;          // of the packed frames: the source files, the packed files
    double total_s = 0;
    // Of all frames (packed + copied + failed): framesGpuEncoded were packed by abub_abf_encode_dev, framesHostRoute by a
    // host thread (or copied, or not written) -- every frame of RepackRun, and of a run outside the decoders' width gate.
    // Of framesGpuEncoded: decoded by abub_png_decode_dev, by abub_abf_decode_dev, by abub_bmp_decode_dev, or by a host
    // thread after a kernel refused the file.
    long long framesGpuEncoded = 0, framesHostRoute = 0;
    long long framesGpuPngDecoded = 0, framesGpuUnpacked = 0, framesHostDecoded = 0, framesGpuBmpDecoded = 0;
    long long framesGpuUnzipped = 0; // ABUB_GPU_UNZIP=1: archive entries whose zip layer abub_unzip_dev inflated
    int device = -1, W = 0, H = 0, batches = 0;   // of the device route (device -1: it was not taken)
    double read_s = 0, decode_s = 0, encode_s = 0, copy_s = 0, write_s = 0; // its legs, summed over the batches
    // --archive: the archive's size and entry count; of the device route, the time of abub_zip_pack_dev (its launches and the
    // wait for them; the segment's copy to the host is copy_s, the host's own entries and the write are write_s)
    long long archiveBytes = 0, archiveEntries = 0;
    double pack_s = 0;
};
// --archive: the copy is the one file <dstRunDir>.zip (the canonical archive of zipwrite.hpp, DESIGN section 3, "A run as one
// archive") instead of the tree <dstRunDir>/.  srcArchive: the archive the parser reads, empty for a directory run; it is
// refused as the target like the source directory is
struct ArchiveTarget {
    bool on = false;
    std::string srcArchive;
};
// abub3hs --repack: every frame of every event and camera 0 .. numCams-1 that `parser` lists, written in the packed format
// (cv::abfEncode) to <dstRunDir>/<event>/<imageFolder>/<same name> on `nthreads` threads.  A source file that does not
// decode is copied byte for byte.  Every event gets its directory, frames or not.  The run's event file
// <dstRunDir>/<its last component>.txt takes the bytes of srcRunFile where that can be read, else one line per event
// that parser->GetRunFileInfo lists.  No GPU.  Returns 0, or 1 if anything could not be written; throws, before anything
// is written, when dstRunDir is srcRunDir (the directory the parser reads; empty for an archive).
int RepackRun(Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir,
              const std::string &imageFolder, int numCams, int nthreads, RepackStats *stats,
              const ArchiveTarget &archive = ArchiveTarget());
// abub3hs --repack --repack-gpu: the same files, byte for byte, with the frames of the run's size (that of the first frame
// that decodes) decoded by the GPU decoders and packed by abub_abf_encode_dev on `device`, in batches of at most 4 frames
// per CU (ABUB_REPACK_BATCH=n, a test knob: of at most n); the pool's threads read and write the files, and pack on the spot what the decoders do not take (a frame the
// thread had to decode itself, a frame of another size; a file that does not decode is copied).  A run whose width the
// decoders do not take (a multiple of 4 from 4 to 2048) goes the host route whole.  Throws, before anything is written,
// when there is no such device: there is no silent fall-back to the host route.
int RepackRunDevice(Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir,
                    const std::string &imageFolder, int numCams, int nthreads, int device, RepackStats *stats,
                    const ArchiveTarget &archive = ArchiveTarget());
// abub3hs --unpack [--unpack-gpu]: the way back.  RepackRun / RepackRunDevice with another frame format: every frame is
// written as a canonical Huffman-only PNG (cv::pngHuffEncode; on the device abub_png_encode_dev, the same bytes) under its
// own name, so that anything that reads PNG reads the run again; the source may be packed, PNG, BMP or mixed.  Layout,
// event file, refusals, return value and stats as there (packed / bytesOut count the PNG files written,
// framesGpuEncoded those abub_png_encode_dev wrote).
int UnpackRun(Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir,
              const std::string &imageFolder, int numCams, int nthreads, RepackStats *stats,
              const ArchiveTarget &archive = ArchiveTarget());
int UnpackRunDevice(Parser *parser, const std::string &srcRunDir, const std::string &srcRunFile, const std::string &dstRunDir,
                    const std::string &imageFolder, int numCams, int nthreads, int device, RepackStats *stats,
                    const ArchiveTarget &archive = ArchiveTarget());

// What verify says about one frame, an extra frame or event, or the event file
struct VerifyFinding {
    enum Verdict { Same, SameNotPacked, Copied, Differ, Missing, Undecodable, Extra, EventFileDiffers, EventFileMissing };
    int verdict = Same;
    std::string event, name; // name: the frame's file; empty for an extra event; the event file's name
    long long ndiff = 0;     // Differ with equal sizes: pixels that differ, the first of them in raster order, max |a - b|
    int x = -1, y = -1, maxAbs = 0;
    int w = 0, h = 0, otherW = 0, otherH = 0; // Differ with different sizes: the source's, the other run's (else 0)
    bool failure() const { return verdict != Same && verdict != SameNotPacked && verdict != Copied; }
    const char *verdictName() const; // "same", "same_not_packed", "copied", "differ", "missing", "undecodable", "extra",
                                     // "event_file_differs", "event_file_missing"
    std::string text() const;        // "3/cam1_image41.png: differ: 37 pixels, first at (x=12, y=3), max |a-b| = 5"
};
struct VerifyStats {
    enum EventFile { FileSame = 0, FileDiffers = 1, FileMissing = 2, FileNotCompared = 3 };
    int events = 0;          // of the source
    long long frames = 0;    // of the source: same + sameNotPacked + copied + differ + missing + undecodable
    long long same = 0, sameNotPacked = 0, copied = 0, differ = 0, missing = 0, undecodable = 0, extra = 0;
    int eventFile = FileNotCompared;
    double total_s = 0;
    // Of the device route (device -1: it was not taken).  Of `frames`: framesKernel were compared by
    // abub_frames_compare_dev, framesHostRoute by a host thread.  Of the frames the decoders were given, per side: by
    // abub_png_decode_dev, by abub_abf_decode_dev, by abub_bmp_decode_dev, or by a host thread (a file the kernels do not
    // take or refused).
    long long framesKernel = 0, framesHostRoute = 0;
    long long srcGpuPngDecoded = 0, srcGpuUnpacked = 0, srcHostDecoded = 0;
    long long otherGpuPngDecoded = 0, otherGpuUnpacked = 0, otherHostDecoded = 0;
    long long srcGpuBmpDecoded = 0, otherGpuBmpDecoded = 0;
    long long srcGpuUnzipped = 0, otherGpuUnzipped = 0; // ABUB_GPU_UNZIP=1: archive entries of each side abub_unzip_dev inflated
    int device = -1, W = 0, H = 0, batches = 0;
    double read_s = 0, decode_s = 0, compare_s = 0; // its legs, summed over the batches
    const char *eventFileName() const;              // "same", "differs", "missing", "not compared"
};
// abub3hs --verify-repack: is the run `other` reads, pixel for pixel, the run `src` reads?  The source is the authority:
// every frame it lists for cameras 0 .. numCams-1 gets one verdict, in event, camera and frame order, on `nthreads`
// threads; both files are decoded by the host decoder (cv::imdecode) and compared with memcmp.  same: identical pixels
// and the other file is a packed frame; same_not_packed: identical pixels, another format; copied: the source does not
// decode and the other file has its bytes; differ, missing, undecodable: failures.  A frame or an event only the other
// run lists is `extra`, a failure.  The event files srcRunFile and otherRunFile are compared byte for byte (not compared
// when one of the names is empty or the source's cannot be read).  `findings` (may be NULL) gets every failure and every
// same_not_packed frame in task order, then the extras, then the event file if it fails.  No GPU.  Returns 0 if nothing
// failed, else 1.
// otherIsArchive (--archive): the copy is an archive, and the event file is compared as bytes: the copy's side is what
// other->GetRunFileBytes hands out (missing where it has none), the source's its file srcRunFile or, for a zipped source,
// what src->GetRunFileBytes hands out (not compared where there is neither); otherRunFile only names the finding.
int VerifyRun(Parser *src, Parser *other, const std::string &srcRunFile, const std::string &otherRunFile, int numCams, int nthreads,
              VerifyStats *stats, std::vector<VerifyFinding> *findings, bool otherIsArchive = false);
// abub3hs --verify-repack --verify-gpu: the same verdicts, findings and counters.  The frames of the run's size (that of
// the source's first frame that decodes) are decoded on both sides by the GPU decoders on `device`, in batches of at most
// 4 frames per CU (ABUB_VERIFY_BATCH=n: of n), and compared by abub_frames_compare_dev; every other frame (a file that does
// not decode, another size, a file the parser does not hand out) gets its verdict from a host thread as in VerifyRun.  A
// run whose width the decoders do not take, or without a frame that decodes, goes the host route whole.  Throws, before
// anything else, when there is no such device: there is no silent fall-back to the host route.
int VerifyRunDevice(Parser *src, Parser *other, const std::string &srcRunFile, const std::string &otherRunFile, int numCams,
                    int nthreads, int device, VerifyStats *stats, std::vector<VerifyFinding> *findings, bool otherIsArchive = false);

// The record of one frame (abub_stat_result without its status; include/abub_hip.h): flags bit 0 says that nOut / sumOut
// are valid, bit 1 that nMoved / sumMoved are
struct FrameStats {
    uint32_t min = 0, max = 0, nZero = 0, nSat = 0, nOut = 0, nMoved = 0, flags = 0;
    uint64_t sum = 0, sumsq = 0, sumOut = 0, sumMoved = 0;
};
// The definition of abub_frame_stats_dev: over the n pixels p of `cur` the range, sum, sum of squares, pixels == 0 and
// == 255; with mu != NULL (sigma6 = min(6 sigma, 255) beside it) count and sum of sat(|p - mu| - sigma6); with mu and ref
// count and sum of sat(|p - ref| - sigma6).  Plain byte loops, the one copy: both survey routes and the tests use it.
FrameStats frameStatsHost(const unsigned char *cur, const unsigned char *ref, const unsigned char *mu, const unsigned char *sigma6,
                          size_t n);
// The definition of abub_pixel_activity_dev, the per-pixel terms of frameStatsHost summed over frames instead: one frame
// ADDED to the six u32 planes planes[k * n + i] (0 n_zero, 1 n_sat, 2 n_out, 3 sum_out, 4 n_moved, 5 sum_moved; DESIGN
// section 3, "Surveying a run per pixel").  mu == NULL: planes 2 to 5 are not touched; ref == NULL: planes 4 and 5 are not.
// Plain byte loops; the adds are relaxed atomics, so the rows of a camera may be added from many threads.  The one copy:
// the host route, the device route's host share and the tests use it.
void activityAddHost(uint32_t *planes, const unsigned char *cur, const unsigned char *ref, const unsigned char *mu,
                     const unsigned char *sigma6, size_t n);
// The definition of abub_frame_shift_dev ("Surveying a run for movement"): the SAD between the W x H frame
// p and the model plane m at every integer displacement within R, 1 <= R <= 8, W and H >= 2 R + 1.  Over the interior
// I = [R, W - R) x [R, H - R): sad[(dy + R) * (2 R + 1) + (dx + R)] = sum over I of |p(x + dx, y + dy) - m(x, y)|; every
// displacement sums the same |I| pixels.  Plain loops, the one copy: both survey routes and the tests use it.
void frameShiftHost(const unsigned char *p, const unsigned char *m, int W, int H, int R, uint64_t *sad);
// What a surface says: the displacement with the smallest sad; among equal ones the smaller dx^2 + dy^2, then the smaller
// dy, then the smaller dx (an all-equal surface gives (0, 0)).  atEdge: |dx| == R or |dy| == R, the true shift may be
// larger.  One host function for both routes: the kernel returns only the surface, so they cannot disagree on a tie.
struct ShiftBest {
    int dx = 0, dy = 0;
    bool atEdge = false;
    uint64_t sad0 = 0, sadBest = 0; // the surface at (0, 0) and at (dx, dy)
};
ShiftBest shiftBest(const uint64_t *sad, int R);
ShiftBest shiftBest(const uint32_t *sad, int R); // the same rule (one template) on a cell's u32 surface
// The definition of abub_frame_shift_cells_dev ("Surveying a run for local movement"): frameShiftHost's
// sums kept apart per whole cell of 128 x 128 interior pixels, on the grid abub_frame_cells_grid gives (the one copy of that
// rule, in the GPU library): sad[((cy * ncx + cx) * (2 R + 1) + (dy + R)) * (2 R + 1) + (dx + R)] = sum over the cell of
// |p(x + dx, y + dy) - m(x, y)|, u32.  Plain loops.  Returns the number of cells, 0 (nothing written) where the frame has none.
size_t fieldCellsHost(const unsigned char *p, const unsigned char *m, int W, int H, int R, uint32_t *sad);
// What a cell's surface says, five i32: dx, dy, sad0, sad_best (shiftBest's answer), sad_max (the largest entry)
enum { FieldRecordWords = 5 };
void fieldCell(const uint32_t *sad, int R, int32_t *rec);
// A cell is rated iff sad_max > 0 and 2 * sad_best <= sad_max: the best displacement explains at least half of the worst
// mismatch.  A flat cell, where every displacement scores alike, is not.
inline bool fieldRated(const int32_t *rec) { return rec[4] > 0 && 2 * (int64_t)rec[3] <= (int64_t)rec[4]; }

// The definition of abub_frame_light_cells_dev ("Surveying a run for lighting changes"): per cell of
// 128 x 128 pixels of the grid (ncx x ncy whole cells, the first at (x0, y0); the survey's is abub_frame_cells_grid's) six
// u32 over the cell's pixels p of the frame and m of mu: rec[(cy * ncx + cx) * 6 + 0 .. 5] = sum p, sum p^2, sum p m,
// sum |p - m|, pixels with p == 0, pixels with p == 255.  Plain loops; at most 16384 * 255^2 < 2^31.
enum { LightRecordWords = 6, LightModelWords = 3 };
void lightCellsHost(const unsigned char *p, const unsigned char *m, int W, int H, int x0, int y0, int ncx, int ncy, uint32_t *rec);
// The model's share, which depends on the camera alone: rec[(cy * ncx + cx) * 3 + 0 .. 2] = sum m, sum m^2, sum sigma6
void lightModelHost(const unsigned char *mu, const unsigned char *sigma6, int W, int H, int x0, int y0, int ncx, int ncy, uint32_t *rec);
// rdiv(a, b) = floor((2 a + b) / (2 b)), b > 0, floor toward minus infinity: a / b rounded to the nearest, a half upward
long long lightRdiv(__int128 a, __int128 b);
// What a cell says, from its frame record and its model record (one function for both routes; integers only).  With
// N = 16384: rated iff sm >= N and n_zero + n_sat <= N / 16; clipped iff sm >= N and not so; of a rated cell
// ratio = rdiv(1000 sp, sm), changed iff |sp - sm| > ss6 (its mean level moved by more than its mean 6 sigma), up iff sp > sm
struct LightCell {
    bool rated = false, clipped = false, changed = false, up = false;
    long long ratio = 0;
};
LightCell lightCell(const uint32_t *rec, const uint32_t *model);
// What a frame says, from its rated cells (n = N * rated, S* pooled over them): level_milli = rdiv(1000 (Ssp - Ssm), n),
// the range of the ratios, and the pooled fit p = gain * m + offset: var = n Ssmm - Ssm^2, cov = n Sspm - Ssp Ssm, with
// var > 0 gain_milli = rdiv(1000 cov, var) and offset_milli = rdiv(1000 Ssp - gain_milli Ssm, n), else hasGain false.
// kind: blind (no rated cell), steady (none of them changed), level (all changed, in one direction), uneven (the rest)
struct LightFrame {
    enum Kind { Blind = 0, Steady = 1, Level = 2, Uneven = 3 };
    int rated = 0, clipped = 0, changed = 0, up = 0, down = 0, kind = Blind;
    bool hasGain = false;
    long long levelMilli = 0, ratioMin = 0, ratioMax = 0, gainMilli = 0, offsetMilli = 0;
};
LightFrame lightFrame(const uint32_t *rec, const uint32_t *model, size_t cells);

// The definition of abub_frame_focus_cells_dev ("Surveying a run for lost focus"): per cell of 128 x 128
// pixels of the grid (ncx x ncy whole cells, the first at (x0, y0) with x0, y0 >= 1, x0 + 128 ncx + 1 <= W and so in y; the
// survey's is abub_frame_cells_grid's) five i32 over the cell's pixels, with the central differences
// gx = p(x + 1, y) - p(x - 1, y), gy = p(x, y + 1) - p(x, y - 1) of the frame and hx, hy of m = mu:
// rec[(cy * ncx + cx) * 5 + 0 .. 4] = sum gx^2, sum gy^2, sum gx hx, sum gy hy, pixels with p == 0 or p == 255.  Plain
// loops; a magnitude of at most 16384 * 255^2 < 2^31.
enum { FocusRecordWords = 5, FocusModelWords = 3 };
void focusCellsHost(const unsigned char *p, const unsigned char *m, int W, int H, int x0, int y0, int ncx, int ncy, int32_t *rec);
// The model's share, which depends on the camera alone: rec[(cy * ncx + cx) * 3 + 0 .. 2] = mxx = sum hx^2, myy = sum hy^2
// and nv = the sum over the cell K and its ring of one pixel of (s6(u) c(u))^2, where c(u) is the coefficient of p(u) in
// G = sum gx hx + sum gy hy: c(u) = [u - ex in K] hx(u - ex) - [u + ex in K] hx(u + ex) + [u - ey in K] hy(u - ey)
// - [u + ey in K] hy(u + ey).  With M = mxx + myy, G - M = sum (p - m)(u) c(u) exactly, so sqrt(nv) is six standard
// deviations of what independent pixel noise of the trained sigma does to G.  nv <= 16900 * (255 * 1020)^2 < 2^63.
void focusModelHost(const unsigned char *mu, const unsigned char *sigma6, int W, int H, int x0, int y0, int ncx, int ncy, int64_t *rec);
// What a cell says, from its frame record and its model record (one function for both routes; integers only, __int128).
// With N = 16384, G = gxm + gym and M = mxx + myy: clipped iff n_clip > N / 16; rated iff not clipped and M^2 > nv (a total
// loss of agreement could be told from noise); of a rated cell keep = rdiv(1000 G, M), energy = rdiv(1000 (gxx + gyy), M)
// (lightRdiv), changed iff (M - G)^2 > nv, and of a changed cell softer iff G < M, else harder
struct FocusCell {
    bool rated = false, clipped = false, changed = false, softer = false;
    long long keep = 0, energy = 0;
};
FocusCell focusCell(const int32_t *rec, const int64_t *model);
// What a frame says, from its rated cells: keep_milli = rdiv(1000 sum G, sum M) and energy_milli =
// rdiv(1000 sum (gxx + gyy), sum M) pooled over them, the range of their keep, and the kind: blind (no rated cell), steady
// (none of them changed), soft (all of them changed, every one softer), uneven (the rest)
struct FocusFrame {
    enum Kind { Blind = 0, Steady = 1, Soft = 2, Uneven = 3 };
    int rated = 0, clipped = 0, changed = 0, softer = 0, harder = 0, kind = Blind;
    long long keepMilli = 0, keepMin = 0, keepMax = 0, energyMilli = 0;
};
FocusFrame focusFrame(const int32_t *rec, const int64_t *model, size_t cells);

// The definition of abub_frame_noise_cells_dev ("Surveying a run for noise changes"): per cell of 128 x 128
// pixels of the grid (ncx x ncy whole cells, the first at (x0, y0); the survey's is abub_frame_cells_grid's) six i32 over the
// cell's pixels p of the frame, r of its reference frame (the frame two before) and s of sigma6, with d = p - r:
// rec[(cy * ncx + cx) * 6 + 0 .. 5] = n_over (pixels with |d| > s), n_clip (pixels where p or r is 0 or 255), s1_in = sum d
// and s2_in = sum d^2 over the pixels with |d| <= s (the inside ones; with s = 0 only d = 0 is inside), sad = sum |d| and
// s2_all = sum d^2 over all.  mu is not read.  Plain loops; a magnitude of at most 16384 * 255^2 < 2^31.
enum { NoiseRecordWords = 6, NoiseModelWords = 5, NoiseCellPixels = 128 * 128 /* ABUB_FIELD_CELL^2 */ };
void noiseCellsHost(const unsigned char *p, const unsigned char *r, const unsigned char *sigma6, int W, int H, int x0, int y0, int ncx,
                    int ncy, int32_t *rec);
// The rule's constants.  A cell is clipped if more than 1 / NoiseClipShare of its pixels are, busy if more than
// 1 / NoiseBusyShare of them lie outside 6 sigma; a rated cell is noisy above NoiseNoisyMilli, quiet below NoiseQuietMilli.
// The two ratios are the rule, not measurements: the sampling spread of a variance over 16384 pixels is sqrt(2 / N), about
// 1.1 %, and a factor 1.5 in variance (1.22 in sigma) is far outside it and well inside a doubling.
enum { NoiseClipShare = 8, NoiseBusyShare = 4, NoiseNoisyMilli = 1500, NoiseQuietMilli = 667 };
// Of a record with N = 16384: n_in = N - n_over and E = s2_in - floor(s1_in^2 / n_in) (0 where n_in = 0), the inside sum of
// squares about the inside mean: a level step between the two frames does not count as noise
inline long long noiseNIn(const int32_t *rec) { return (long long)NoiseCellPixels - rec[0]; }
inline long long noiseE(const int32_t *rec)
{
    const long long n = noiseNIn(rec), s1 = rec[2];
    return n > 0 ? (long long)rec[3] - s1 * s1 / n : 0; // (s1^2 >= 0: the division floors)
}
inline bool noiseClipped(const int32_t *rec) { return (long long)rec[1] * NoiseClipShare > (long long)NoiseCellPixels; }
inline bool noiseBusy(const int32_t *rec) { return (long long)rec[0] * NoiseBusyShare > (long long)NoiseCellPixels; }
// The camera's share, measured from the run itself: rec[(cy * ncx + cx) * 5 + 0 .. 4] = BE, BN, B, sum s^2 over the cell, the
// cell's pixels with s = 0.  recs[0 .. nrecs): the records ([ncy][ncx][6]) of the camera's rows at stack position 1 that have
// one (their reference is frame 0: the two frames the Trainer reads); per cell, over those of them that are neither clipped
// nor busy in that cell, BE = sum E, BN = sum n_in and B their number.  The u8 sigma is truncated, so a rule against sigma
// itself would call every steady run noisy: the baseline is the run's own.
void noiseModelHost(const unsigned char *sigma6, int W, int H, int x0, int y0, int ncx, int ncy, const int32_t *const *recs, size_t nrecs,
                    int64_t *rec);
// What a cell says, from its frame record and its model record (one function for both routes; integers only, unsigned
// __int128).  The states in this order: clipped; busy (too much of the cell lies outside 6 sigma for the inside sums to mean
// noise; all_milli says which); nobase (BE = 0 or B = 0); else rated by q_milli = floor(1000 E BN / (n_in BE)): noisy above
// 1500, quiet below 667, else same.  all_milli = floor(1000 s2_all BN / (N BE)), 0 without a baseline, whatever the state.
// model_milli = floor(1000 * 18 BE N / (BN sum s^2)) (0 where BN or sum s^2 is 0): how far the u8 sigma plane is from the
// noise it was trained on (E[d^2] = 2 sigma^2 and s = 6 sigma give the 18); reported, never used to rate.
struct NoiseCell {
    enum State { Clipped = 0, Busy = 1, NoBase = 2, Noisy = 3, Quiet = 4, Same = 5 };
    int state = NoBase;
    bool rated() const { return state >= Noisy; }
    long long qMilli = 0, allMilli = 0; // qMilli: of a rated cell
};
NoiseCell noiseCell(const int32_t *rec, const int64_t *model);
long long noiseModelMilli(const int64_t *model);
// What a frame says, from its cells.  Pooled over the rated cells q_milli = floor(1000 sum(E BN) / sum(n_in BE)) and the range
// of their q_milli; pooled over the cells with a baseline that are not clipped all_milli = floor(1000 sum(s2_all BN) /
// sum(N BE)) (0 where there is none).  kind, with U the cells that are not clipped: blind (rated + busy < a quarter of all
// cells), else busy (busy * 2 > U), else steady (no noisy and no quiet cell), else noisy (no quiet cell and noisy * 2 >=
// rated), else quiet (no noisy cell and quiet * 2 >= rated), else uneven
struct NoiseFrame {
    enum Kind { Blind = 0, Busy = 1, Steady = 2, Noisy = 3, Quiet = 4, Uneven = 5 };
    int rated = 0, clipped = 0, busy = 0, noisy = 0, quiet = 0, kind = Blind;
    long long qMilli = 0, qMin = 0, qMax = 0, allMilli = 0;
};
NoiseFrame noiseFrame(const int32_t *rec, const int64_t *model, size_t cells);

// The definition of abub_frame_lines_dev ("Surveying a run for torn, repeated and banded frames"): per image
// row y of the W x H frame p five u32 over the row's W pixels, against m of mu and r of the reference frame (the frame two
// before; null: none, words 3 and 4 are 0): rows[y * 5 + 0 .. 4] = sum p, sum |p - m|, n_clip (pixels with p == 0 or
// p == 255), sum |p - r|, n_same (pixels with p == r); per image column x the first three over the column's H pixels:
// cols[x * 3 + 0 .. 2].  Plain loops; with W, H <= 65535 a value of at most 65535 * 255 < 2^24.
enum { LinesRowWords = 5, LinesColWords = 3, LinesModelWords = 3 };
void linesHost(const unsigned char *p, const unsigned char *r, const unsigned char *mu, int W, int H, uint32_t *rows, uint32_t *cols);
// The camera's share, once per camera: per row (rows[y * 3 + 0 .. 2]) and per column (cols[x * 3 + 0 .. 2]) sum m, T = the
// sum of sigma6 (min(6 sigma, 255)) and n_s0, the pixels with sigma6 == 0
void linesModelHost(const unsigned char *mu, const unsigned char *sigma6, int W, int H, uint32_t *rows, uint32_t *cols);
// The rule's constants.  A line of N pixels is unrated if more than 1 / LinesShare of them are clipped or have sigma6 == 0.
// A rated line is off when e^2 N > LinesFactor (n T)^2, with n the frame's rated lines of its direction, D = word 0 - sum m,
// S the sum of D over them and e = n D - S: n times the line's excess over the frame's own level, against two times T in
// amplitude (the line's noise is about T / (6 sqrt N); DESIGN has the simulation the factor comes from and the measured
// margin).  A frame is torn from LinesTornRun consecutive stale rows on, banded or striped from LinesOffLines off lines on.
enum { LinesShare = 4, LinesFactor = 4, LinesTornRun = 8, LinesOffLines = 4 };
// What one line says (one function for rows and columns and for both routes; integers only, the products in unsigned
// __int128: e^2 N reaches 10^29): rec, its record (the first three words are read); model, its model record; N, its pixels;
// n and S as above, over the rated lines of the frame -> LineUnrated, LineRated (and not off) or LineOff.  *num and *den (may
// be null) get e^2 N and (n T)^2 of a rated line
enum LineState { LineUnrated = 0, LineRated = 1, LineOff = 2, LineStale = 3 }; // (stale: of a row, in linesFrame's states only)
bool lineRated(const uint32_t *rec, const uint32_t *model, long long N);
int lineRate(const uint32_t *rec, const uint32_t *model, long long N, long long n, long long S, unsigned __int128 *num = nullptr,
             unsigned __int128 *den = nullptr);
// What a frame says, from its records and its camera's model.  A rated row is stale when the frame has a reference and its
// n_same == W.  kind, the first that applies: blind (the rated rows are fewer than a quarter of H), repeated (a reference,
// and every rated row is stale), torn (a run of at least 8 consecutive stale rows), banded (at least 4 off rows), striped (at
// least 4 off columns), steady.  levelMilli = floor(1000 S / (n W)) over the rated rows (0 without one): the frame's level
// above the model's; first / last: -1 where there is none
struct LinesFrame {
    enum Kind { Blind = 0, Repeated = 1, Torn = 2, Banded = 3, Striped = 4, Steady = 5 };
    int ratedRows = 0, offRows = 0, staleRows = 0, firstStale = -1, lastStale = -1, ratedCols = 0, offCols = 0;
    int firstOffRow = -1, lastOffRow = -1, firstOffCol = -1, lastOffCol = -1, kind = Blind;
    long long levelMilli = 0;
};
// rowState[H] and colState[W] (may be null): per line its LineState (a row that is off and stale: LineStale)
LinesFrame linesFrame(const uint32_t *rows, const uint32_t *cols, const uint32_t *modelRows, const uint32_t *modelCols, int W, int H,
                      bool hasRef, uint8_t *rowState = nullptr, uint8_t *colState = nullptr);

// What a survey makes of every ok row of a camera with a model, beyond its record: the index of the row's state, of the
// product's counters and of the host threads' clocks
enum SurveyProduct { SurveyShiftProduct = 0, SurveyFieldProduct = 1, SurveyLightProduct = 2, SurveyFocusProduct = 3, SurveyNoiseProduct = 4,
                     SurveyLinesProduct = 5, SurveyProducts = 6 };
// One row of a survey: a frame the run lists, or one it should list (missing)
struct SurveyRow {
    enum State { Ok = 0, Undecodable = 1, Missing = 2, OtherSize = 3 };
    enum Made { None = 0, Host = 1, Kernel = 2 }; // who made a product of the row: nobody, a host thread, the product's kernel
    size_t ev = 0;           // index into the run's sorted event list
    std::string event, name;
    int cam = 0, frame = 0;  // frame: its place in its (event, camera) stack, missing frames counted
    int state = Ok, w = 0, h = 0; // w, h: of Ok and OtherSize rows
    FrameStats s;            // Ok: all of it, as far as its flags say; OtherSize: the raw columns
    bool onKernel = false;
    uint16_t made = 0;       // two bits per SurveyProduct: an ok row of a camera with a model has every product that was asked for
                             // (the noise only where its reference row is another row, ok and of the run's size)
    Made has(SurveyProduct p) const { return (Made)(made >> (2 * p) & 3); }
    void set(SurveyProduct p, Made m) { made = (uint16_t)((made & ~(3 << (2 * p))) | (m << (2 * p))); }
    ShiftBest shift;             // with a shift file: its surface's answer
    std::vector<int32_t> field;  // with a field directory: its cells' records, [ncy][ncx][5]
    std::vector<uint32_t> light; // with a light directory: its cells' light records, [ncy][ncx][6]
    std::vector<int32_t> focus;  // with a focus directory: its cells' focus records, [ncy][ncx][5]
    std::vector<int32_t> noise;  // with a noise directory: its cells' noise records, [ncy][ncx][6]
    std::vector<uint32_t> linesRows, linesCols; // with a lines directory: linesHost's [H][5] and [W][3]
    bool linesRef = false;       // those were made against a reference frame (another row, ok and of the run's size)
    const char *stateName() const; // "ok", "undecodable", "missing", "other_size"
};
// What the report says of one camera's model
struct SurveyModel {
    bool trained = false;
    int trainingSetSize = 0, sigmaMax = 0;
    long long pixels = 0, sigmaZero = 0, sigma6Sat = 0; // pixels with sigma == 0; with 6 sigma >= 255
    double muMean = 0;
    std::vector<uint32_t> light; // with a light directory, of a trained camera: lightModelHost's [ncy][ncx][3]
    std::vector<int64_t> focus;  // with a focus directory, of a trained camera: focusModelHost's [ncy][ncx][3]
    std::vector<int64_t> noise;  // with a noise directory, of a trained camera: noiseModelHost's [ncy][ncx][5]
    std::vector<uint32_t> linesRows, linesCols; // with a lines directory, of a trained camera: linesModelHost's [H][3] and [W][3]
};
// The counters of one product: the rows whose product its kernel made (abub_frame_shift_dev, abub_frame_shift_cells_dev,
// abub_frame_light_cells_dev, abub_frame_focus_cells_dev, abub_frame_noise_cells_dev, abub_frame_lines_dev) and those a host thread made from the definition, the kernel's
// calls, the seconds of the device route's leg (launches, copy back) and the seconds the host threads spent in the
// definition, summed over the threads
struct ProductStats {
    long long framesKernel = 0, framesHost = 0;
    int launches = 0;
    double leg_s = 0, host_s = 0;
};
struct SurveyStats {
    int events = 0;
    long long frames = 0; // rows: ok + undecodable + missing + otherSize
    long long ok = 0, undecodable = 0, missing = 0, otherSize = 0;
    // Of `frames`: framesKernel got their record from abub_frame_stats_dev, framesHostRoute from a host thread (or have
    // none).  Of the device route (device -1: it was not taken): the frames each decoder lane decoded, those a host thread
    // decoded for the slab, reference frames read again because their batch was over, archive entries inflated on the GPU
    long long framesKernel = 0, framesHostRoute = 0;
    long long gpuPngDecoded = 0, gpuUnpacked = 0, gpuBmpDecoded = 0, hostDecoded = 0, reread = 0, gpuUnzipped = 0;
    int device = -1, W = 0, H = 0, batches = 0, modelCams = 0;
    double read_s = 0, decode_s = 0, stats_s = 0, total_s = 0;
    // With a planes directory: the rows abub_pixel_activity_dev added to the planes and those a host thread added (on the
    // device route: the rows whose file no GPU decoder reads, decoded by a reading thread, and the rows not in place); the
    // seconds of the activity launches, of the planes' copy back and of writing the files
    long long planeRowsKernel = 0, planeRowsHost = 0;
    double activity_s = 0, planes_copy_s = 0, planes_write_s = 0;
    ProductStats product[SurveyProducts]; // of the products that were asked for
};
// What a survey writes and where (abub3hs --survey and its --survey-* flags); an empty path: that product is not made.
// srcRunDir (empty: an archive) is the directory the run is read from; it is refused as any of the directories below: a run
// directory is not the place for what was derived from it.
struct SurveyRequest {
    std::string reportPath, srcRunDir;
    // DESIGN section 3, "Surveying a run per pixel": planesDir (the CLI's DIR/<run_ID>) gets cam<c>_activity.npy (u32
    // [6, H, W]) for every camera with a listed row, cam<c>_moved.png for those with a model, and activity.txt
    std::string planesDir;
    // "Surveying a run for movement": per ok row of a camera with a model the best displacement of the frame against mu within
    // shiftRadius.  A run narrower or lower than 2 shiftRadius + 1 is refused before its frames are measured
    std::string shiftPath;
    int shiftRadius = 4;
    // The per-cell products, each into its directory (the CLI's DIR/<run_ID>), for every camera with a model, of its rows
    // that have the product, in survey order.  All three share one grid: abub_frame_cells_grid at cellRadius; a run narrower or
    // lower than 128 + 2 cellRadius has no whole cell and is refused before its frames are measured.
    // "... for local movement": cam<c>_field.npy (i32 [N_c, ncy, ncx, 5]) and field.txt;
    // "... for lighting changes": cam<c>_light.npy (i32 [N_c, ncy, ncx, 6]), cam<c>_light_model.npy (i32 [ncy, ncx, 3]), light.txt;
    // "... for lost focus": cam<c>_focus.npy (i32 [N_c, ncy, ncx, 5]), cam<c>_focus_model.npy (i64 [ncy, ncx, 3]), focus.txt;
    // "... for noise changes": cam<c>_noise.npy (i32 [N_c, ncy, ncx, 6]), cam<c>_noise_model.npy (i64 [ncy, ncx, 5]), noise.txt
    std::string fieldDir;
    int cellRadius = 4;
    std::string lightDir, focusDir, noiseDir;
    // "Surveying a run for torn, repeated and banded frames": linesDir (the CLI's DIR/<run_ID>) gets, for every camera with a
    // model, of its ok rows cam<c>_lines_rows.npy (i32 [N_c, H, 5]) and cam<c>_lines_cols.npy (i32 [N_c, W, 3]), the model's
    // cam<c>_lines_model_rows.npy (i32 [H, 3]) and cam<c>_lines_model_cols.npy (i32 [W, 3]), and lines.txt.  No grid: any size
    std::string linesDir;
};
// The texts of field.txt, light.txt, focus.txt and noise.txt: "# abub3hs <tag> 1", the grid's line, the table's header and one
// tab-separated row per survey row, one `<tag> cam` line per camera, the `moved` (field) or `changed` lines of every camera
// with a model, the `run` line.  Both routes write them through these functions; W, H: the run's size; models[c].light,
// models[c].focus and models[c].noise: the camera's model record.  A `noise cam` line ends with the cells' model_milli.
std::string FieldReport(int radius, int W, int H, const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows);
std::string LightReport(int radius, int W, int H, const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows);
std::string FocusReport(int radius, int W, int H, const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows);
std::string NoiseReport(int radius, int W, int H, const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows);
// The text of lines.txt: "# abub3hs lines 1", `size W H`, the table's header and one tab-separated row per survey row (the
// rated, off and stale rows, the first and last stale row, the rated and off columns, the first and last off row and off
// column, the level in thousandths, the kind), one `lines cam` line per camera, per camera with a model one `changed` line
// for every row and every column that was off or stale in a frame, with the number of such frames, the `run` line
std::string LinesReport(int W, int H, const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows);
// The shift file's text: "# abub3hs shift 1", `radius R`, the table's header and one tab-separated row per survey row, one
// `shift cam` line per camera, the `run` line.  Both routes write it through this one function.
std::string ShiftReport(int radius, const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows);
// The report's text ("Surveying a run"): "# abub3hs survey 1", one `model` line per camera, the table's
// header and one tab-separated row per frame, the `run` line.  Both routes write it through this one function.
std::string SurveyReport(const std::vector<SurveyModel> &models, const std::vector<SurveyRow> &rows);
// abub3hs --survey FILE: every frame that `parser` lists for cameras 0 .. numCams-1 measured, no analysis: one row per
// frame in event, camera and frame order.  A frame number (read from the name through imageFormat) that some stack of the
// run has and a stack with frames lacks is a `missing` row of that stack.  Frame i of a stack is measured against frame
// max(i - 2, 0) of it (the trigger search's pairing) and against the model of its camera: trainers[cam] where it is there,
// trained (StatusCode 0) and of the run's size (that of the first frame that decodes); without it the model columns are
// invalid, and the moved columns also where the reference frame is not ok.  The report goes to request.reportPath (empty: it
// is not written), every other product of `request` to its place; a product changes nothing in the others.  Returns 0, or 1
// if any frame is not ok; throws where a file cannot be written.
// device < 0, the host route: cv::imdecode and the definitions (frameStatsHost, activityAddHost, frameShiftHost,
// fieldCellsHost, lightCellsHost, focusCellsHost, noiseCellsHost, linesHost) on `nthreads` threads.  No GPU.
// device >= 0 (--survey-gpu): the same rows and the same files, byte for byte.  The frames are read through the FileBatch
// protocol (framefiles.hpp) in batches of at most 4 frames per CU (ABUB_SURVEY_BATCH=n: of n), decoded into the batch's
// slab, and measured by one abub_frame_stats_dev launch per batch, with the products' kernels behind it.  A batch that
// begins inside a stack reads again the at most two frames of the batch before that its first jobs refer to (they take
// slots of their own: the number of batches is ceil(rows / batch size) exactly).  A frame that is not in place in the slab
// (no decoder reads it, another size) gets its row from the host route's per-frame function.  A run whose width the
// decoders do not take, or without a frame that decodes, goes the host route whole.  Throws, before anything else, when
// there is no such device.
int SurveyRun(Parser *parser, const std::vector<Trainer *> &trainers, int numCams, const std::string &imageFormat,
              const SurveyRequest &request, int nthreads, int device, SurveyStats *stats, std::vector<SurveyRow> *rows = nullptr,
              std::vector<SurveyModel> *models = nullptr);

// A run listed and trained, ready for detect; rc = -5 (the run cannot be read) or -7 (a camera did not train)
struct PreparedRun {
    std::unique_ptr<Parser> parser;
    std::vector<std::string> events;
    std::vector<std::unique_ptr<Trainer>> owned;
    std::vector<Trainer *> trainers;
    int rc = 0;
    double train_s = 0;
    bool hostTrained = false;
    long long trainGpuUnzipped = 0; // ABUB_GPU_UNZIP=1: archive entries abub_unzip_dev inflated for the device training
    std::string log; // stdout lines held back (buffered)
    PreparedRun();
    PreparedRun(PreparedRun &&);
    PreparedRun &operator=(PreparedRun &&);
    ~PreparedRun();
};

// The CLI's flow up to detect (AutoBubStart3.cpp:250-307) without writing anything: the event list, then training (the
// host Trainer, or TrainOnDevice where opt.trainOnGpu; trainerDebug: the Trainers' debug flag).  buffered: the lines for
// stdout are held in pr.log (the host Trainer's own lines are printed as they come); buffers: kept from run to run.
PreparedRun PrepareRun(const RunSpec &r, const BatchedRunOptions &opt, int trainerDebug, DeviceTrainBuffers *buffers,
                       bool buffered);
// Prints the held-back lines, then writes the run's header into opt.outDir, and its -5 / -7 rows when it failed
void CommitRun(const RunSpec &r, const BatchedRunOptions &opt, PreparedRun &pr);

struct CampaignStats {
    int runs = 0;                  // runs that were started (listed, trained, detected or failed)
    long long frames = 0;          // frames of the batched runs (decoded or not)
    double total_s = 0;
    double train_s = 0;            // training, summed over runs
    double trainExposed_s = 0;     // ... of which the detect loop waited for
    int pipelinesBuilt = 0;
    long long framesGpuUnzipped = 0, trainGpuUnzipped = 0; // ABUB_GPU_UNZIP=1: archive entries inflated by abub_unzip_dev, detect / training
    int trainedOnHost = 0;         // runs trained by the host Trainer (ABUB_TRAIN_ON_GPU=0, or TrainOnDevice declined)
    std::vector<int> status;       // per run: 0, -5, -6, -7 (what a single-run invocation returns)
    std::vector<std::string> notRun; // runs never started after a GPU failure
};

// Every run of `runs` in one process, each written to its own abub3hs_<run>.txt in opt.outDir with the bytes a single-run
// invocation writes.  The workers (one per GPU) keep their buffers, streams and pipelines from one run to the next; while
// a run is detected, the next one lists its events and trains (on the device, its own stream).  A HIP or IO failure ends
// the campaign at that run (-6).  Returns the first nonzero status in list order, else 0.
int RunCampaign(const std::vector<RunSpec> &runs, const BatchedRunOptions &opt, CampaignStats *stats);

} // namespace abub
#endif
