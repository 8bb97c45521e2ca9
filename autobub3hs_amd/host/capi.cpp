// capi.cpp -- small C surface over the C++ API mirror so that the Python test-suite and bench.py can
// drive Trainer / L3Localizer exactly the way the reference's main() does (AutoBubStart3.cpp:294-307,
// :363-364 and AnyCamAnalysis :67-125).  Not part of the drop-in boundary.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <exception>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "AlgorithmTraining/Trainer.hpp"
#include "AnalyzerUnit.hpp"
#include "ImageEntropyMethods/ImageEntropyMethods.hpp"
#include "BubbleLocalizer/L3Localizer.hpp"
#include "PICOFormatWriter/PICOFormatWriterV4.hpp"
#include "ParseFolder/Parser.hpp"
#include "ParseFolder/RawParser.hpp"
#include "ParseFolder/ZipParser.hpp"
#include "devctx.hpp"
#include "devtrain.hpp"
#include "driver.hpp"
#include "hostlogic.hpp"
#include "peek.hpp"
#include "bmpwalk.hpp"
#include "pngwalk.hpp"
#include "runbatch.hpp"
#include "zipwrite.hpp"
#include "stackresult.hpp"

namespace {

struct Run {
    Parser *parser = nullptr; // MemParser (tests / synthetic), RawParser or ZipParser
    int kind = -1;            // of abh_run_open
    std::string runFolder, imageFolder, imageFormat;
    MemParser *mem = nullptr;
    std::string frames_of_last_query;
    std::map<int, Trainer *> trainers;
    abub::StackResult last; // last analysis; last.error also carries the text of any other failed call on the run
};

} // namespace

// test hook for the per-frame statistics that are private in AnalyzerUnit and dead upstream (128-bin entropy and its
// z-score, AnalyzerUnit.cpp:386-433; the image overload of calculateSignificanceFrame :435-504)
namespace abub {
struct AnalyzerProbe {
    static float entropy(AnalyzerUnit &A, cv::Mat &m) { return A.calculateEntropyFrame(m, false); }
    static double entropySignificance(AnalyzerUnit &A, cv::Mat &m, bool store) { return A.calculateEntropySignificance(m, store, false); }
    static double significance(AnalyzerUnit &A, cv::Mat &m, bool store) { return A.calculateSignificanceFrame(m, store, false); }
};
} // namespace abub

extern "C" {

// feeds `n` images [n][H][W] through an analyzer of (ev, cam): out[3*k] = 128-bin entropy of image k, out[3*k+1] =
// its z-score over the history so far (stored), out[3*k+2] = the 256-bin significance (stored)
int abh_probe_frame_stats(void *r, const char *ev, int cam, const uint8_t *imgs, int n, int W, int H, double *out)
{
    Run *run = (Run *)r;
    auto it = run->trainers.find(cam);
    if (it == run->trainers.end() || !it->second)
        return -100;
    Trainer *t = it->second;
    try {
        L3Localizer A(ev, "", cam, true, &t, "", run->parser->clone());
        for (int k = 0; k < n; ++k) {
            cv::Mat m(H, W, CV_8U);
            std::memcpy(m.data, imgs + (size_t)k * W * H, (size_t)W * H);
            out[3 * k] = abub::AnalyzerProbe::entropy(A, m);
            out[3 * k + 1] = abub::AnalyzerProbe::entropySignificance(A, m, true);
            out[3 * k + 2] = abub::AnalyzerProbe::significance(A, m, true);
        }
    } catch (std::exception &e) {
        run->last.error = e.what();
        return -1;
    }
    abub::DeviceContext::releaseThread();
    return 0;
}

void *abh_run_new()
{
    Run *r = new Run();
    r->mem = new MemParser();
    r->parser = r->mem;
    return r;
}

// kind 0: directory tree (RawParser), 1: zip archive (ZipParser); NULL if the source cannot be opened
void *abh_run_open(int kind, const char *runFolder, const char *imageFolder, const char *imageFormat)
{
    try {
        Run *r = new Run();
        if (kind == 0)
            r->parser = new RawParser(runFolder, imageFolder, imageFormat);
        else
            r->parser = new ZipParser(runFolder, imageFolder, imageFormat);
        r->kind = kind;
        r->runFolder = runFolder;
        r->imageFolder = imageFolder;
        r->imageFormat = imageFormat;
        return r;
    } catch (int code) {
        return nullptr;
    } catch (std::exception &) {
        return nullptr;
    }
}

// '\n'-joined list into the run's scratch string; returns its c_str (valid until the next query)
const char *abh_run_events(void *r)
{
    Run *run = (Run *)r;
    run->frames_of_last_query.clear();
    for (auto &e : abub::sortedEvents(*run->parser))
        run->frames_of_last_query += e + "\n";
    return run->frames_of_last_query.c_str();
}
const char *abh_run_frames(void *r, const char *ev, int cam)
{
    Run *run = (Run *)r;
    std::vector<std::string> fr;
    run->parser->ParseAndSortFramesInFolder(ev, cam, fr);
    run->frames_of_last_query.clear();
    for (auto &f : fr)
        run->frames_of_last_query += f + "\n";
    return run->frames_of_last_query.c_str();
}
// decode one frame through the parser: returns GetImage's code, fills w/h and (if cap suffices) the pixels
int abh_run_image(void *r, const char *ev, const char *frame, uint8_t *out, int cap, int *w, int *h)
{
    Run *run = (Run *)r;
    cv::Mat m;
    int rc = run->parser->GetImage(ev, frame, m);
    *w = m.cols;
    *h = m.rows;
    if (!m.empty() && (int)m.total() <= cap)
        std::memcpy(out, m.data, m.total());
    return rc;
}
// the archive entry behind a frame (Parser::GetImageEntryInfo / ReadImageEntryRaw): info_out = [method, compressed size,
// uncompressed size, CRC-32], returns 1, or 0 where the parser has no entry to describe; abh_run_entry_raw: the entry's
// compressed bytes as they lie in the archive, returns their count or -1
int abh_run_entry_info(void *r, const char *ev, const char *frame, double *info_out)
{
    Parser::EntryInfo e;
    try {
        if (!((Run *)r)->parser->GetImageEntryInfo(ev, frame, e))
            return 0;
    } catch (...) {
        return 0;
    }
    info_out[0] = e.method;
    info_out[1] = (double)e.compressedSize;
    info_out[2] = (double)e.uncompressedSize;
    info_out[3] = (double)e.crc32;
    return 1;
}
long long abh_run_entry_raw(void *r, const char *ev, const char *frame, uint8_t *out, long long cap)
{
    try {
        return ((Run *)r)->parser->ReadImageEntryRaw(ev, frame, out, (size_t)std::max(0LL, cap));
    } catch (...) {
        return -1;
    }
}
int abh_imdecode(const uint8_t *data, int n, uint8_t *out, int cap, int *w, int *h)
{
    cv::Mat m = cv::imdecode(data, (size_t)n, 0);
    *w = m.cols;
    *h = m.rows;
    if (m.empty())
        return -1;
    if ((int)m.total() <= cap)
        std::memcpy(out, m.data, m.total());
    return 0;
}

// the packed frame format (host/abf.cpp): abh_abf_encode returns the file's size (written when cap suffices), -1 on errors;
// abh_abf_decode the code of cv::abfDecodeStatus (0 = decoded into out, W * H bytes)
long long abh_abf_encode(const uint8_t *img, int W, int H, uint8_t *out, long long cap)
{
    std::vector<uchar> v;
    if (!cv::abfEncode(img, W, H, v))
        return -1;
    if ((long long)v.size() <= cap)
        std::memcpy(out, v.data(), v.size());
    return (long long)v.size();
}
int abh_abf_decode(const uint8_t *data, long long n, uint8_t *out, int W, int H)
{
    return cv::abfDecodeStatus(data, (size_t)n, out, W, H);
}
// the canonical Huffman-only PNG (host/pnghuff.cpp): abh_png_huff_encode returns the file's size (written when cap suffices),
// -1 on errors; abh_png_huff_bound cv::pngHuffFileBound; abh_png_huff_lengths cv::pngHuffLengths (the depth of the
// unlimited tree, -1 on bad arguments)
long long abh_png_huff_encode(const uint8_t *img, int W, int H, uint8_t *out, long long cap)
{
    std::vector<uchar> v;
    if (!cv::pngHuffEncode(img, W, H, v))
        return -1;
    if ((long long)v.size() <= cap)
        std::memcpy(out, v.data(), v.size());
    return (long long)v.size();
}
long long abh_png_huff_bound(int W, int H) { return (long long)cv::pngHuffFileBound(W, H); }
int abh_png_huff_lengths(const uint64_t *counts, int n, int limit, uint8_t *lengths)
{
    return cv::pngHuffLengths(counts, n, limit, lengths);
}
// abub::RepackRun of a run opened with abh_run_open into the directory `dstRunDir` (its last component is the new run ID);
// stats (may be NULL): [frames packed, copied as they are, not written, bytes of the packed frames' sources, of the packed
// files, seconds].  Returns RepackRun's code, -1 on errors.  abh_run_repack_dev: abub::RepackRunDevice on `device`, no
// fall-back when there is no such device; its stats go on with [frames encoded on the GPU, of them decoded by the PNG
// kernel, by the packed kernel, by a host thread, frames that took the host route, batches, seconds of the legs read,
// upload + decode, encode, copy back, write, the device (-1: the whole run took the host route), of the encoded frames
// those decoded by the BMP kernel, archive entries inflated by abub_unzip_dev (ABUB_GPU_UNZIP=1)] (20 values).
// abh_run_unpack / abh_run_unpack_dev: abub::UnpackRun / abub::UnpackRunDevice, the same arguments and stats (packed: frames
// written as canonical Huffman-only PNG files).
// the event file of a directory run: <run>/<runID>.txt; empty for an archive
static std::string eventFileOf(const Run &run)
{
    if (run.kind != 0)
        return std::string();
    std::string folder = run.runFolder;
    while (folder.size() > 1 && folder.back() == '/')
        folder.pop_back();
    const size_t slash = folder.find_last_of('/');
    return folder + "/" + (slash == std::string::npos ? folder : folder.substr(slash + 1)) + ".txt";
}
static int runRepack(void *r, const char *dstRunDir, int ncams, int nthreads, int device, bool onDevice, double *stats,
                     bool unpack = false, bool archive = false)
{
    Run *run = (Run *)r;
    try {
        if (run->kind < 0) {
            run->last.error = std::string(unpack ? "unpack" : "repack") + ": not a run opened from a directory or an archive";
            return -1;
        }
        const std::string src = eventFileOf(*run);
        abub::RepackStats st;
        const std::string srcDir = run->kind == 0 ? run->runFolder : std::string();
        const int threads = std::max(1, nthreads);
        const abub::ArchiveTarget target{archive, run->kind == 0 ? std::string() : abub::zipPathOf(run->runFolder)};
        const int rc = onDevice ? (unpack ? abub::UnpackRunDevice : abub::RepackRunDevice)(run->parser, srcDir, src, dstRunDir,
                                                                                         run->imageFolder, ncams, threads, device, &st,
                                                                                         target)
                                : (unpack ? abub::UnpackRun : abub::RepackRun)(run->parser, srcDir, src, dstRunDir, run->imageFolder,
                                                                               ncams, threads, &st, target);
        if (stats) {
            const double v[20] = {(double)st.packed, (double)st.copied, (double)st.failed, (double)st.bytesIn, (double)st.bytesOut,
                                  st.total_s, (double)st.framesGpuEncoded, (double)st.framesGpuPngDecoded,
                                  (double)st.framesGpuUnpacked, (double)st.framesHostDecoded, (double)st.framesHostRoute,
                                  (double)st.batches, st.read_s, st.decode_s, st.encode_s, st.copy_s, st.write_s, (double)st.device,
                                  (double)st.framesGpuBmpDecoded, (double)st.framesGpuUnzipped};
            std::memcpy(stats, v, (onDevice || archive ? 20 : 6) * sizeof(double));
            if (archive) {
                stats[20] = (double)st.archiveBytes;
                stats[21] = (double)st.archiveEntries;
                stats[22] = st.pack_s;
            }
        }
        return rc;
    } catch (std::exception &e) {
        run->last.error = e.what();
        return -1;
    }
}
int abh_run_repack(void *r, const char *dstRunDir, int ncams, int nthreads, double *stats)
{
    return runRepack(r, dstRunDir, ncams, nthreads, -1, false, stats);
}
int abh_run_repack_dev(void *r, const char *dstRunDir, int ncams, int nthreads, int device, double *stats)
{
    return runRepack(r, dstRunDir, ncams, nthreads, device, true, stats);
}
int abh_run_unpack(void *r, const char *dstRunDir, int ncams, int nthreads, double *stats)
{
    return runRepack(r, dstRunDir, ncams, nthreads, -1, false, stats, true);
}
int abh_run_unpack_dev(void *r, const char *dstRunDir, int ncams, int nthreads, int device, double *stats)
{
    return runRepack(r, dstRunDir, ncams, nthreads, device, true, stats, true);
}
// --archive: the four entries above with the copy written as the one archive <dstRunDir>.zip (host/zipwrite.hpp).  device < 0:
// the host route; unpack != 0: abh_run_unpack's codec.  stats (may be NULL): the 20 values of abh_run_repack_dev (those of
// the device route 0 on the host route, the device -1), then [the archive's bytes, its entries, seconds of abub_zip_pack_dev]
// (23 values).
int abh_run_repack_archive(void *r, const char *dstRunDir, int ncams, int nthreads, int device, int unpack, double *stats)
{
    return runRepack(r, dstRunDir, ncams, nthreads, device, device >= 0, stats, unpack != 0, true);
}
// The host writer of the canonical archive alone: n entries (entry i: name_len[i] bytes of `names`, len[i] bytes of `data`,
// both laid end to end) written to `path` through <path>.part.  Returns 0, or -1 (abh_zip_error() says why; no file is left)
static thread_local std::string zipError;
int abh_zip_write(const char *path, int n, const uint8_t *names, const uint32_t *name_len, const uint8_t *data, const uint64_t *len)
{
    try {
        abub::ZipWriter zw(path);
        for (int i = 0; i < n; ++i) {
            zw.add(std::string((const char *)names, name_len[i]), data, (size_t)len[i]);
            names += name_len[i];
            data += len[i];
        }
        zw.finish();
        return 0;
    } catch (std::exception &e) {
        zipError = e.what();
        return -1;
    }
}
const char *abh_zip_error() { return zipError.c_str(); }

// abub::VerifyRun of two runs opened with abh_run_open: is `other` pixel for pixel the run `src`?  stats (may be NULL, 29
// values; the last two: the source's and the other run's archive entries inflated by abub_unzip_dev, ABUB_GPU_UNZIP=1): [events, frames, same, same but not packed, copied, differ, missing, undecodable, extra, the event file (0 same,
// 1 differs, 2 missing, 3 not compared), seconds, the report's length; of the device route: frames compared by the kernel,
// frames that took the host route, the source's frames decoded by the PNG kernel, by the packed kernel, by a host thread,
// the other run's likewise, batches, seconds of the legs read, upload + decode, compare, the device (-1: it was not
// taken), the source's and the other run's frames decoded by the BMP kernel].  report (may be NULL): one line per finding, "event\tname\tverdict\tndiff\tx\ty\tmax_abs\tw\th\tother_w\tother_h\n",
// cut at report_cap - 1 characters; the whole text stays with `src` for abh_run_verify_report.  Returns VerifyRun's code, -1
// on errors.  abh_run_verify_dev: abub::VerifyRunDevice on `device`, no fall-back when there is no such device.
static int runVerify(void *a, void *b, int ncams, int nthreads, int device, bool onDevice, double *stats, char *report, int report_cap,
                     bool otherIsArchive = false)
{
    Run *run = (Run *)a, *other = (Run *)b;
    try {
        if (!other || run->kind < 0 || other->kind < 0) {
            run->last.error = "verify: not two runs opened from a directory or an archive";
            return -1;
        }
        abub::VerifyStats st;
        std::vector<abub::VerifyFinding> findings;
        const int rc = onDevice ? abub::VerifyRunDevice(run->parser, other->parser, eventFileOf(*run), eventFileOf(*other), ncams,
                                                        std::max(1, nthreads), device, &st, &findings, otherIsArchive)
                                : abub::VerifyRun(run->parser, other->parser, eventFileOf(*run), eventFileOf(*other), ncams,
                                                  std::max(1, nthreads), &st, &findings, otherIsArchive);
        std::string &text = run->frames_of_last_query;
        text.clear();
        for (const abub::VerifyFinding &f : findings)
            text += f.event + "\t" + f.name + "\t" + f.verdictName() + "\t" + std::to_string(f.ndiff) + "\t" + std::to_string(f.x) + "\t" +
                    std::to_string(f.y) + "\t" + std::to_string(f.maxAbs) + "\t" + std::to_string(f.w) + "\t" + std::to_string(f.h) + "\t" +
                    std::to_string(f.otherW) + "\t" + std::to_string(f.otherH) + "\n";
        if (report && report_cap > 0) {
            const size_t n = std::min(text.size(), (size_t)report_cap - 1);
            std::memcpy(report, text.data(), n);
            report[n] = 0;
        }
        if (stats) {
            const double v[29] = {(double)st.events, (double)st.frames, (double)st.same, (double)st.sameNotPacked, (double)st.copied,
                                  (double)st.differ, (double)st.missing, (double)st.undecodable, (double)st.extra, (double)st.eventFile,
                                  st.total_s, (double)text.size(), (double)st.framesKernel, (double)st.framesHostRoute,
                                  (double)st.srcGpuPngDecoded, (double)st.srcGpuUnpacked, (double)st.srcHostDecoded,
                                  (double)st.otherGpuPngDecoded, (double)st.otherGpuUnpacked, (double)st.otherHostDecoded,
                                  (double)st.batches, st.read_s, st.decode_s, st.compare_s, (double)st.device,
                                  (double)st.srcGpuBmpDecoded, (double)st.otherGpuBmpDecoded, (double)st.srcGpuUnzipped,
                                  (double)st.otherGpuUnzipped};
            std::memcpy(stats, v, sizeof v);
        }
        return rc;
    } catch (std::exception &e) {
        run->last.error = e.what();
        return -1;
    } catch (...) { // (the parsers throw their status codes)
        run->last.error = "verify: a run could not be read";
        return -1;
    }
}
int abh_run_verify(void *src, void *other, int ncams, int nthreads, double *stats, char *report, int report_cap)
{
    return runVerify(src, other, ncams, nthreads, -1, false, stats, report, report_cap);
}
int abh_run_verify_dev(void *src, void *other, int ncams, int nthreads, int device, double *stats, char *report, int report_cap)
{
    return runVerify(src, other, ncams, nthreads, device, true, stats, report, report_cap);
}
// --archive: `other` is a run opened from the archive that --repack --archive wrote; the event file is compared as bytes (the
// archive's <run>.txt entry against the source's file or entry).  device < 0: the host route
int abh_run_verify_archive(void *src, void *other, int ncams, int nthreads, int device, double *stats, char *report, int report_cap)
{
    return runVerify(src, other, ncams, nthreads, device, device >= 0, stats, report, report_cap, true);
}
// the whole report of the last abh_run_verify[_dev] on `src` (valid until the next query on it)
const char *abh_run_verify_report(void *src)
{
    return ((Run *)src)->frames_of_last_query.c_str();
}

// abub::SurveyRun of a run opened with abh_run_open (abub3hs --survey): the run is listed and trained the way the CLI does it
// (abub::PrepareRun, the host Trainer; a camera that does not train has no model), then every frame is measured.  path (may
// be NULL or empty): where the report is written.  stats (may be NULL, 24 values): [events, frames, ok, undecodable, missing,
// other size, frames measured by the kernel, frames that took the host route, frames decoded by the PNG kernel, by the
// packed kernel, by the BMP kernel, by a host thread for the slab, reference frames read again, archive entries inflated on
// the GPU, the device (-1: its route was not taken), W, H, batches, cameras with a model, seconds of the legs read, upload +
// decode, measure, seconds in all, the report's length].  report (may be NULL): the report's text, cut at report_cap - 1
// characters; the whole text stays with the run for abh_run_survey_report.  Returns SurveyRun's code (0, or 1 if a frame is
// not ok), -5 if the run cannot be read, -1 on errors.  abh_run_survey_dev: the device route on `device`, no fall-back
// when there is no such device.
// abh_run_survey_planes[_dev]: the same with the per-pixel planes written to planes_dir (abub::SurveyRequest::planesDir, the CLI's
// DIR/<run_ID>; NULL or empty: none) and plane_stats (may be NULL, 5 values): [rows added to the planes by
// abub_pixel_activity_dev, rows added by a host thread, seconds of the activity launches, of the copy back, of the files].
// abh_run_survey_shift[_dev]: the same with the shift search (SurveyRequest::shiftPath; DESIGN section 3, "Surveying a run for
// movement") written to shift_path (NULL or empty: none) at radius shift_radius (1 to 8), and shift_stats (may be NULL, 5
// values): [frames searched by abub_frame_shift_dev, by a host thread, the kernel's calls, seconds of the device route's shift
// leg, seconds the host threads spent in frameShiftHost].
// abh_run_survey_field[_dev]: the same with the per-cell shift field (SurveyRequest::fieldDir; DESIGN section 3, "Surveying a run
// for local movement") written to field_dir (the CLI's DIR/<run_ID>; NULL or empty: none) at radius field_radius (1 to 8),
// and field_stats (may be NULL, 5 values): the shift's five for abub_frame_shift_cells_dev and fieldCellsHost.
// abh_run_survey_light[_dev]: the same with the per-cell light records (SurveyRequest::lightDir; DESIGN section 3, "Surveying a run
// for lighting changes") written to light_dir (the CLI's DIR/<run_ID>; NULL or empty: none) on the grid of field_radius,
// whether or not field_dir is given, and light_stats (may be NULL, 5 values): the same five for abub_frame_light_cells_dev
// and lightCellsHost.
// abh_run_survey_focus[_dev]: the same with the per-cell focus records (SurveyRequest::focusDir; DESIGN section 3, "Surveying a run
// for lost focus") written to focus_dir (the CLI's DIR/<run_ID>; NULL or empty: none) on the grid of field_radius, whether
// or not field_dir or light_dir is given, and focus_stats (may be NULL, 5 values): the same five for
// abub_frame_focus_cells_dev and focusCellsHost.
// abh_run_survey_noise[_dev]: the same with the per-cell noise records (SurveyRequest::noiseDir; DESIGN section 3, "Surveying a run
// for noise changes") written to noise_dir (the CLI's DIR/<run_ID>; NULL or empty: none) on the grid of field_radius, whether
// or not any of the other three is given, and noise_stats (may be NULL, 5 values): the same five for
// abub_frame_noise_cells_dev and noiseCellsHost.
// abh_run_survey_lines[_dev]: the same with the per-line records (SurveyRequest::linesDir; DESIGN section 3, "Surveying a run
// for torn, repeated and banded frames") written to lines_dir (the CLI's DIR/<run_ID>; NULL or empty: none), whatever else is
// given, and lines_stats (may be NULL, 5 values): the same five for abub_frame_lines_dev and linesHost.
// what an entry's arguments ask for (a NULL path: none; the directory the run is read from is runSurvey's to fill in)
static abub::SurveyRequest surveyRequest(const char *path, const char *planes_dir = nullptr, const char *shift_path = nullptr,
                                         int shift_radius = 4, const char *field_dir = nullptr, int field_radius = 4,
                                         const char *light_dir = nullptr, const char *focus_dir = nullptr, const char *noise_dir = nullptr,
                                         const char *lines_dir = nullptr)
{
    const auto str = [](const char *s) { return std::string(s ? s : ""); };
    abub::SurveyRequest rq;
    rq.reportPath = str(path);
    rq.planesDir = str(planes_dir);
    rq.shiftPath = str(shift_path);
    rq.shiftRadius = shift_radius;
    rq.fieldDir = str(field_dir);
    rq.cellRadius = field_radius;
    rq.lightDir = str(light_dir);
    rq.focusDir = str(focus_dir);
    rq.noiseDir = str(noise_dir);
    rq.linesDir = str(lines_dir);
    return rq;
}
static int runSurvey(void *r, abub::SurveyRequest rq, int ncams, int nthreads, int device, bool onDevice, char *report, int report_cap,
                     double *stats, double *plane_stats = nullptr, double *shift_stats = nullptr, double *field_stats = nullptr,
                     double *light_stats = nullptr, double *focus_stats = nullptr, double *noise_stats = nullptr,
                     double *lines_stats = nullptr)
{
    Run *run = (Run *)r;
    try {
        if (run->kind < 0) {
            run->last.error = "survey: not a run opened from a directory or an archive";
            return -1;
        }
        abub::RunSpec sp;
        sp.eventDir = run->runFolder;
        sp.imageFolder = run->imageFolder;
        sp.imageFormat = run->imageFormat;
        sp.numCams = ncams;
        sp.zipped = run->kind == 1;
        abub::BatchedRunOptions bo;
        bo.trainOnGpu = 0;
        abub::PreparedRun pr = abub::PrepareRun(sp, bo, 0, nullptr, true);
        if (pr.rc == -5)
            return -5;
        abub::SurveyStats st;
        std::vector<abub::SurveyRow> rows;
        std::vector<abub::SurveyModel> models;
        rq.srcRunDir = run->kind == 0 ? run->runFolder : std::string();
        if (onDevice && device < 0) // (a _dev entry chose the device route: there is no falling back to the host's)
            throw std::runtime_error("survey: no such HIP device: " + std::to_string(device));
        const int rc = abub::SurveyRun(pr.parser.get(), pr.trainers, ncams, sp.imageFormat, rq, std::max(1, nthreads), onDevice ? device : -1,
                                       &st, &rows, &models);
        double *const product_stats[abub::SurveyProducts] = {shift_stats, field_stats, light_stats, focus_stats, noise_stats, lines_stats};
        for (int p = 0; p < abub::SurveyProducts; ++p)
            if (product_stats[p]) {
                const abub::ProductStats &ps = st.product[p];
                const double v[5] = {(double)ps.framesKernel, (double)ps.framesHost, (double)ps.launches, ps.leg_s, ps.host_s};
                std::memcpy(product_stats[p], v, sizeof v);
            }
        if (plane_stats) {
            const double v[5] = {(double)st.planeRowsKernel, (double)st.planeRowsHost, st.activity_s, st.planes_copy_s, st.planes_write_s};
            std::memcpy(plane_stats, v, sizeof v);
        }
        std::string &text = run->frames_of_last_query;
        text = abub::SurveyReport(models, rows);
        if (report && report_cap > 0) {
            const size_t n = std::min(text.size(), (size_t)report_cap - 1);
            std::memcpy(report, text.data(), n);
            report[n] = 0;
        }
        if (stats) {
            const double v[24] = {(double)st.events, (double)st.frames, (double)st.ok, (double)st.undecodable, (double)st.missing,
                                  (double)st.otherSize, (double)st.framesKernel, (double)st.framesHostRoute, (double)st.gpuPngDecoded,
                                  (double)st.gpuUnpacked, (double)st.gpuBmpDecoded, (double)st.hostDecoded, (double)st.reread,
                                  (double)st.gpuUnzipped, (double)st.device, (double)st.W, (double)st.H, (double)st.batches,
                                  (double)st.modelCams, st.read_s, st.decode_s, st.stats_s, st.total_s, (double)text.size()};
            std::memcpy(stats, v, sizeof v);
        }
        return rc;
    } catch (std::exception &e) {
        run->last.error = e.what();
        return -1;
    } catch (...) { // (the parsers throw their status codes)
        run->last.error = "survey: the run could not be read";
        return -1;
    }
}
int abh_run_survey(void *r, const char *path, int ncams, int nthreads, double *stats, char *report, int report_cap)
{
    return runSurvey(r, surveyRequest(path), ncams, nthreads, -1, false, report, report_cap, stats);
}
int abh_run_survey_dev(void *r, const char *path, int ncams, int nthreads, int device, double *stats, char *report, int report_cap)
{
    return runSurvey(r, surveyRequest(path), ncams, nthreads, device, true, report, report_cap, stats);
}
int abh_run_survey_planes(void *r, const char *path, const char *planes_dir, int ncams, int nthreads, double *stats, double *plane_stats,
                          char *report, int report_cap)
{
    return runSurvey(r, surveyRequest(path, planes_dir), ncams, nthreads, -1, false, report, report_cap, stats, plane_stats);
}
int abh_run_survey_planes_dev(void *r, const char *path, const char *planes_dir, int ncams, int nthreads, int device, double *stats,
                              double *plane_stats, char *report, int report_cap)
{
    return runSurvey(r, surveyRequest(path, planes_dir), ncams, nthreads, device, true, report, report_cap, stats, plane_stats);
}
int abh_run_survey_shift(void *r, const char *path, const char *planes_dir, const char *shift_path, int shift_radius, int ncams,
                         int nthreads, double *stats, double *plane_stats, double *shift_stats, char *report, int report_cap)
{
    return runSurvey(r, surveyRequest(path, planes_dir, shift_path, shift_radius), ncams, nthreads, -1, false, report, report_cap, stats,
                     plane_stats, shift_stats);
}
int abh_run_survey_shift_dev(void *r, const char *path, const char *planes_dir, const char *shift_path, int shift_radius, int ncams,
                             int nthreads, int device, double *stats, double *plane_stats, double *shift_stats, char *report,
                             int report_cap)
{
    return runSurvey(r, surveyRequest(path, planes_dir, shift_path, shift_radius), ncams, nthreads, device, true, report, report_cap, stats,
                     plane_stats, shift_stats);
}
int abh_run_survey_field(void *r, const char *path, const char *planes_dir, const char *shift_path, int shift_radius, const char *field_dir,
                         int field_radius, int ncams, int nthreads, double *stats, double *plane_stats, double *shift_stats,
                         double *field_stats, char *report, int report_cap)
{
    return runSurvey(r, surveyRequest(path, planes_dir, shift_path, shift_radius, field_dir, field_radius), ncams, nthreads, -1, false,
                     report, report_cap, stats, plane_stats, shift_stats, field_stats);
}
int abh_run_survey_field_dev(void *r, const char *path, const char *planes_dir, const char *shift_path, int shift_radius,
                             const char *field_dir, int field_radius, int ncams, int nthreads, int device, double *stats,
                             double *plane_stats, double *shift_stats, double *field_stats, char *report, int report_cap)
{
    return runSurvey(r, surveyRequest(path, planes_dir, shift_path, shift_radius, field_dir, field_radius), ncams, nthreads, device, true,
                     report, report_cap, stats, plane_stats, shift_stats, field_stats);
}
int abh_run_survey_light(void *r, const char *path, const char *planes_dir, const char *shift_path, int shift_radius, const char *field_dir,
                         int field_radius, const char *light_dir, int ncams, int nthreads, double *stats, double *plane_stats,
                         double *shift_stats, double *field_stats, double *light_stats, char *report, int report_cap)
{
    return runSurvey(r, surveyRequest(path, planes_dir, shift_path, shift_radius, field_dir, field_radius, light_dir), ncams, nthreads, -1,
                     false, report, report_cap, stats, plane_stats, shift_stats, field_stats, light_stats);
}
int abh_run_survey_light_dev(void *r, const char *path, const char *planes_dir, const char *shift_path, int shift_radius,
                             const char *field_dir, int field_radius, const char *light_dir, int ncams, int nthreads, int device,
                             double *stats, double *plane_stats, double *shift_stats, double *field_stats, double *light_stats,
                             char *report, int report_cap)
{
    return runSurvey(r, surveyRequest(path, planes_dir, shift_path, shift_radius, field_dir, field_radius, light_dir), ncams, nthreads,
                     device, true, report, report_cap, stats, plane_stats, shift_stats, field_stats, light_stats);
}
int abh_run_survey_focus(void *r, const char *path, const char *planes_dir, const char *shift_path, int shift_radius, const char *field_dir,
                         int field_radius, const char *light_dir, const char *focus_dir, int ncams, int nthreads, double *stats,
                         double *plane_stats, double *shift_stats, double *field_stats, double *light_stats, double *focus_stats,
                         char *report, int report_cap)
{
    return runSurvey(r, surveyRequest(path, planes_dir, shift_path, shift_radius, field_dir, field_radius, light_dir, focus_dir), ncams,
                     nthreads, -1, false, report, report_cap, stats, plane_stats, shift_stats, field_stats, light_stats, focus_stats);
}
int abh_run_survey_focus_dev(void *r, const char *path, const char *planes_dir, const char *shift_path, int shift_radius,
                             const char *field_dir, int field_radius, const char *light_dir, const char *focus_dir, int ncams,
                             int nthreads, int device, double *stats, double *plane_stats, double *shift_stats, double *field_stats,
                             double *light_stats, double *focus_stats, char *report, int report_cap)
{
    return runSurvey(r, surveyRequest(path, planes_dir, shift_path, shift_radius, field_dir, field_radius, light_dir, focus_dir), ncams,
                     nthreads, device, true, report, report_cap, stats, plane_stats, shift_stats, field_stats, light_stats, focus_stats);
}
int abh_run_survey_noise(void *r, const char *path, const char *planes_dir, const char *shift_path, int shift_radius, const char *field_dir,
                         int field_radius, const char *light_dir, const char *focus_dir, const char *noise_dir, int ncams, int nthreads,
                         double *stats, double *plane_stats, double *shift_stats, double *field_stats, double *light_stats,
                         double *focus_stats, double *noise_stats, char *report, int report_cap)
{
    return runSurvey(r, surveyRequest(path, planes_dir, shift_path, shift_radius, field_dir, field_radius, light_dir, focus_dir, noise_dir),
                     ncams, nthreads, -1, false, report, report_cap, stats, plane_stats, shift_stats, field_stats, light_stats, focus_stats,
                     noise_stats);
}
int abh_run_survey_noise_dev(void *r, const char *path, const char *planes_dir, const char *shift_path, int shift_radius,
                             const char *field_dir, int field_radius, const char *light_dir, const char *focus_dir, const char *noise_dir,
                             int ncams, int nthreads, int device, double *stats, double *plane_stats, double *shift_stats,
                             double *field_stats, double *light_stats, double *focus_stats, double *noise_stats, char *report,
                             int report_cap)
{
    return runSurvey(r, surveyRequest(path, planes_dir, shift_path, shift_radius, field_dir, field_radius, light_dir, focus_dir, noise_dir),
                     ncams, nthreads, device, true, report, report_cap, stats, plane_stats, shift_stats, field_stats, light_stats,
                     focus_stats, noise_stats);
}
int abh_run_survey_lines(void *r, const char *path, const char *planes_dir, const char *shift_path, int shift_radius, const char *field_dir,
                         int field_radius, const char *light_dir, const char *focus_dir, const char *noise_dir, const char *lines_dir,
                         int ncams, int nthreads, double *stats, double *plane_stats, double *shift_stats, double *field_stats,
                         double *light_stats, double *focus_stats, double *noise_stats, double *lines_stats, char *report, int report_cap)
{
    return runSurvey(r, surveyRequest(path, planes_dir, shift_path, shift_radius, field_dir, field_radius, light_dir, focus_dir, noise_dir,
                                      lines_dir),
                     ncams, nthreads, -1, false, report, report_cap, stats, plane_stats, shift_stats, field_stats, light_stats, focus_stats,
                     noise_stats, lines_stats);
}
int abh_run_survey_lines_dev(void *r, const char *path, const char *planes_dir, const char *shift_path, int shift_radius,
                             const char *field_dir, int field_radius, const char *light_dir, const char *focus_dir, const char *noise_dir,
                             const char *lines_dir, int ncams, int nthreads, int device, double *stats, double *plane_stats,
                             double *shift_stats, double *field_stats, double *light_stats, double *focus_stats, double *noise_stats,
                             double *lines_stats, char *report, int report_cap)
{
    return runSurvey(r, surveyRequest(path, planes_dir, shift_path, shift_radius, field_dir, field_radius, light_dir, focus_dir, noise_dir,
                                      lines_dir),
                     ncams, nthreads, device, true, report, report_cap, stats, plane_stats, shift_stats, field_stats, light_stats,
                     focus_stats, noise_stats, lines_stats);
}
// the whole report of the last abh_run_survey[_dev] on the run (valid until the next query on it)
const char *abh_run_survey_report(void *r)
{
    return ((Run *)r)->frames_of_last_query.c_str();
}
// abub::frameStatsHost on raw buffers of n bytes (ref, mu may be NULL; sigma6 = min(6 sigma, 255) goes with mu): out[11] =
// [min, max, n_zero, n_sat, n_out, n_moved, flags, sum, sumsq, sum_out, sum_moved]
void abh_frame_stats_host(const uint8_t *cur, const uint8_t *ref, const uint8_t *mu, const uint8_t *sigma6, uint64_t n, uint64_t *out)
{
    const abub::FrameStats s = abub::frameStatsHost(cur, ref, mu, sigma6, (size_t)n);
    const uint64_t v[11] = {s.min, s.max, s.nZero, s.nSat, s.nOut, s.nMoved, s.flags, s.sum, s.sumsq, s.sumOut, s.sumMoved};
    std::memcpy(out, v, sizeof v);
}

// abub::activityAddHost on raw buffers: one frame of n bytes ADDED to planes[6 * n] (ref, mu may be NULL; sigma6 goes with mu)
void abh_activity_add_host(uint32_t *planes, const uint8_t *cur, const uint8_t *ref, const uint8_t *mu, const uint8_t *sigma6, uint64_t n)
{
    abub::activityAddHost(planes, cur, ref, mu, sigma6, (size_t)n);
}

// abub::frameShiftHost on raw buffers: the W x H frame p against the model plane m at radius R -> sad[(2 R + 1)^2]; returns 0,
// or -1 (nothing written) for a null pointer, R outside [1, 8] or a side below 2 R + 1
int abh_frame_shift_host(const uint8_t *p, const uint8_t *m, int W, int H, int R, uint64_t *sad)
{
    if (!p || !m || !sad || R < 1 || R > 8 || W < 2 * R + 1 || H < 2 * R + 1)
        return -1;
    abub::frameShiftHost(p, m, W, H, R, sad);
    return 0;
}
// abub::shiftBest of a surface of radius R: out[3] = [dx, dy, at_edge]
void abh_shift_best(const uint64_t *sad, int R, int *out)
{
    const abub::ShiftBest b = abub::shiftBest(sad, R);
    out[0] = b.dx;
    out[1] = b.dy;
    out[2] = b.atEdge ? 1 : 0;
}

// abub_frame_cells_grid (the GPU library's, the one copy of the rule): out[4] = [ncx, ncy, x0, y0]; returns 0, or -1 (nothing
// written) for a null pointer, R outside [1, 8] or a negative side
int abh_field_grid(int W, int H, int R, int *out)
{
    if (!out)
        return -1;
    int v[4];
    if (abub_frame_cells_grid(W, H, R, &v[0], &v[1], &v[2], &v[3]) != ABUB_OK)
        return -1;
    std::memcpy(out, v, sizeof v);
    return 0;
}
// abub::fieldCellsHost and abub::fieldCell on raw buffers: the W x H frame p against the model plane m at radius R ->
// sad[ncy * ncx * (2 R + 1)^2] and rec[ncy * ncx * 5]; returns the number of cells, or -1 (nothing written) for a null
// pointer, R outside [1, 8] or a frame without a whole cell
int abh_field_cells_host(const uint8_t *p, const uint8_t *m, int W, int H, int R, uint32_t *sad, int32_t *rec)
{
    int g[4];
    if (!p || !m || !sad || !rec || abh_field_grid(W, H, R, g) || g[0] * g[1] == 0)
        return -1;
    const size_t cells = abub::fieldCellsHost(p, m, W, H, R, sad), N = (size_t)(2 * R + 1) * (2 * R + 1);
    for (size_t k = 0; k < cells; ++k)
        abub::fieldCell(sad + k * N, R, rec + k * abub::FieldRecordWords);
    return (int)cells;
}

// do ncx x ncy whole cells of 128 x 128 pixels from (x0, y0) lie inside a W x H frame?
static bool lightGridInside(int W, int H, int x0, int y0, int ncx, int ncy)
{
    const int C = ABUB_FIELD_CELL;
    return W >= C && H >= C && ncx >= 1 && ncy >= 1 && ncx <= W / C && ncy <= H / C && x0 >= 0 && y0 >= 0 && x0 <= W - C * ncx &&
           y0 <= H - C * ncy;
}
// abub::lightCellsHost / abub::lightModelHost on raw buffers: the W x H frame p against the model plane m (mu, sigma6) on
// the grid of ncx x ncy cells of 128 x 128 pixels from (x0, y0) -> rec[ncy * ncx * 6] / rec[ncy * ncx * 3]; returns the
// number of cells, or -1 (nothing written) for a null pointer or a grid that does not lie inside the frame
int abh_light_cells_host(const uint8_t *p, const uint8_t *m, int W, int H, int x0, int y0, int ncx, int ncy, uint32_t *rec)
{
    if (!p || !m || !rec || !lightGridInside(W, H, x0, y0, ncx, ncy))
        return -1;
    abub::lightCellsHost(p, m, W, H, x0, y0, ncx, ncy, rec);
    return ncx * ncy;
}
int abh_light_model_host(const uint8_t *mu, const uint8_t *sigma6, int W, int H, int x0, int y0, int ncx, int ncy, uint32_t *rec)
{
    if (!mu || !sigma6 || !rec || !lightGridInside(W, H, x0, y0, ncx, ncy))
        return -1;
    abub::lightModelHost(mu, sigma6, W, H, x0, y0, ncx, ncy, rec);
    return ncx * ncy;
}
// abub::lightFrame on raw buffers, what a frame's records say against the model's: out[12] = rated, clipped, changed, up,
// down, kind (0 blind, 1 steady, 2 level, 3 uneven), has_gain, level_milli, ratio_min, ratio_max, gain_milli, offset_milli
void abh_light_frame(const uint32_t *rec, const uint32_t *model, int cells, long long *out)
{
    const abub::LightFrame f = abub::lightFrame(rec, model, (size_t)std::max(cells, 0));
    const long long v[12] = {f.rated, f.clipped, f.changed, f.up, f.down, f.kind, f.hasGain ? 1 : 0, f.levelMilli, f.ratioMin, f.ratioMax,
                             f.gainMilli, f.offsetMilli};
    std::memcpy(out, v, sizeof v);
}

// do ncx x ncy whole cells of 128 x 128 pixels from (x0, y0) and a ring of one pixel around them lie inside a W x H frame?
static bool focusGridInside(int W, int H, int x0, int y0, int ncx, int ncy)
{
    const int C = ABUB_FIELD_CELL;
    return W >= C + 2 && H >= C + 2 && ncx >= 1 && ncy >= 1 && ncx <= (W - 2) / C && ncy <= (H - 2) / C && x0 >= 1 && y0 >= 1 &&
           x0 <= W - 1 - C * ncx && y0 <= H - 1 - C * ncy;
}
// abub::focusCellsHost / abub::focusModelHost on raw buffers: the W x H frame p against the model plane m / the planes mu and
// sigma6 on the grid of ncx x ncy cells of 128 x 128 pixels from (x0, y0) -> rec[ncy * ncx * 5] (i32) / rec[ncy * ncx * 3]
// (i64); returns the number of cells, or -1 (nothing written) for a null pointer or a grid that does not lie inside the
// frame with its ring
int abh_focus_cells_host(const uint8_t *p, const uint8_t *m, int W, int H, int x0, int y0, int ncx, int ncy, int32_t *rec)
{
    if (!p || !m || !rec || !focusGridInside(W, H, x0, y0, ncx, ncy))
        return -1;
    abub::focusCellsHost(p, m, W, H, x0, y0, ncx, ncy, rec);
    return ncx * ncy;
}
int abh_focus_model_host(const uint8_t *mu, const uint8_t *sigma6, int W, int H, int x0, int y0, int ncx, int ncy, int64_t *rec)
{
    if (!mu || !sigma6 || !rec || !focusGridInside(W, H, x0, y0, ncx, ncy))
        return -1;
    abub::focusModelHost(mu, sigma6, W, H, x0, y0, ncx, ncy, rec);
    return ncx * ncy;
}
// abub::focusCell on raw buffers, what a cell's record says against its model's: out[6] = rated, clipped, changed, softer,
// keep, energy
void abh_focus_cell(const int32_t *rec, const int64_t *model, long long *out)
{
    const abub::FocusCell c = abub::focusCell(rec, model);
    const long long v[6] = {c.rated, c.clipped, c.changed, c.softer, c.keep, c.energy};
    std::memcpy(out, v, sizeof v);
}
// abub::focusFrame on raw buffers, what a frame's records say against the model's: out[10] = rated, clipped, changed, softer,
// harder, kind (0 blind, 1 steady, 2 soft, 3 uneven), keep_milli, keep_min, keep_max, energy_milli
void abh_focus_frame(const int32_t *rec, const int64_t *model, int cells, long long *out)
{
    const abub::FocusFrame f = abub::focusFrame(rec, model, (size_t)std::max(cells, 0));
    const long long v[10] = {f.rated, f.clipped, f.changed, f.softer, f.harder, f.kind, f.keepMilli, f.keepMin, f.keepMax, f.energyMilli};
    std::memcpy(out, v, sizeof v);
}

// abub::noiseCellsHost on raw buffers: the W x H frame p against its reference frame r and the plane sigma6 on the grid of
// ncx x ncy cells of 128 x 128 pixels from (x0, y0) -> rec[ncy * ncx * 6] (i32); returns the number of cells, or -1 (nothing
// written) for a null pointer or a grid that does not lie inside the frame
int abh_noise_cells_host(const uint8_t *p, const uint8_t *r, const uint8_t *sigma6, int W, int H, int x0, int y0, int ncx, int ncy,
                         int32_t *rec)
{
    if (!p || !r || !sigma6 || !rec || !lightGridInside(W, H, x0, y0, ncx, ncy))
        return -1;
    abub::noiseCellsHost(p, r, sigma6, W, H, x0, y0, ncx, ncy, rec);
    return ncx * ncy;
}
// abub::noiseModelHost on raw buffers: recs[nrecs * ncy * ncx * 6], the records of the camera's rows at stack position 1, one
// after another (nrecs may be 0, recs then NULL) -> rec[ncy * ncx * 5] (i64); returns as above
int abh_noise_model_host(const uint8_t *sigma6, int W, int H, int x0, int y0, int ncx, int ncy, const int32_t *recs, int nrecs, int64_t *rec)
{
    if (!sigma6 || !rec || nrecs < 0 || (nrecs > 0 && !recs) || !lightGridInside(W, H, x0, y0, ncx, ncy))
        return -1;
    std::vector<const int32_t *> each((size_t)nrecs);
    for (int q = 0; q < nrecs; ++q)
        each[(size_t)q] = recs + (size_t)q * ncx * ncy * abub::NoiseRecordWords;
    abub::noiseModelHost(sigma6, W, H, x0, y0, ncx, ncy, each.data(), each.size(), rec);
    return ncx * ncy;
}
// abub::noiseCell on raw buffers, what a cell's record says against its model's: out[4] = state (0 clipped, 1 busy, 2 nobase,
// 3 noisy, 4 quiet, 5 same), q_milli, all_milli, model_milli
void abh_noise_cell(const int32_t *rec, const int64_t *model, long long *out)
{
    const abub::NoiseCell c = abub::noiseCell(rec, model);
    const long long v[4] = {c.state, c.qMilli, c.allMilli, abub::noiseModelMilli(model)};
    std::memcpy(out, v, sizeof v);
}
// abub::noiseFrame on raw buffers, what a frame's records say against the model's: out[10] = rated, clipped, busy, noisy,
// quiet, kind (0 blind, 1 busy, 2 steady, 3 noisy, 4 quiet, 5 uneven), q_milli, q_min, q_max, all_milli
void abh_noise_frame(const int32_t *rec, const int64_t *model, int cells, long long *out)
{
    const abub::NoiseFrame f = abub::noiseFrame(rec, model, (size_t)std::max(cells, 0));
    const long long v[10] = {f.rated, f.clipped, f.busy, f.noisy, f.quiet, f.kind, f.qMilli, f.qMin, f.qMax, f.allMilli};
    std::memcpy(out, v, sizeof v);
}

// abub::linesHost on raw buffers: the W x H frame p against the plane mu and the reference frame r (NULL: none) -> rows[H * 5]
// and cols[W * 3] (u32); returns H, or -1 (nothing written) for a null pointer or a side outside [1, 65535]
int abh_lines_host(const uint8_t *p, const uint8_t *r, const uint8_t *mu, int W, int H, uint32_t *rows, uint32_t *cols)
{
    if (!p || !mu || !rows || !cols || W < 1 || W > 65535 || H < 1 || H > 65535)
        return -1;
    abub::linesHost(p, r, mu, W, H, rows, cols);
    return H;
}
// abub::linesModelHost on raw buffers -> rows[H * 3] and cols[W * 3] (u32): sum mu, sum sigma6, pixels with sigma6 == 0;
// returns as above
int abh_lines_model_host(const uint8_t *mu, const uint8_t *sigma6, int W, int H, uint32_t *rows, uint32_t *cols)
{
    if (!mu || !sigma6 || !rows || !cols || W < 1 || W > 65535 || H < 1 || H > 65535)
        return -1;
    abub::linesModelHost(mu, sigma6, W, H, rows, cols);
    return H;
}
// abub::lineRate on raw buffers, what a line of N pixels says: rec[3] and model[3], n the frame's rated lines and S their sum
// of D; returns 0 unrated, 1 rated and not off, 2 off; out[4] (may be NULL) = e^2 N and (n T)^2 of a rated line, each as its
// low and its high 64 bits
int abh_lines_rate(const uint32_t *rec, const uint32_t *model, long long N, long long n, long long S, unsigned long long *out)
{
    unsigned __int128 num = 0, den = 0;
    const int state = abub::lineRate(rec, model, N, n, S, &num, &den);
    if (out) {
        const unsigned long long v[4] = {(unsigned long long)num, (unsigned long long)(num >> 64), (unsigned long long)den,
                                         (unsigned long long)(den >> 64)};
        std::memcpy(out, v, sizeof v);
    }
    return state;
}
// abub::linesFrame on raw buffers, what a frame's records say against the model's: out[13] = rated_rows, off_rows, stale_rows,
// first_stale, last_stale, rated_cols, off_cols, first_off_row, last_off_row, first_off_col, last_off_col (-1: none),
// level_milli, kind (0 blind, 1 repeated, 2 torn, 3 banded, 4 striped, 5 steady); row_state[H] and col_state[W] (may be NULL):
// per line 0 unrated, 1 rated, 2 off, 3 stale
void abh_lines_frame(const uint32_t *rows, const uint32_t *cols, const uint32_t *model_rows, const uint32_t *model_cols, int W, int H,
                     int has_ref, long long *out, uint8_t *row_state, uint8_t *col_state)
{
    const abub::LinesFrame f = abub::linesFrame(rows, cols, model_rows, model_cols, W, H, has_ref != 0, row_state, col_state);
    const long long v[13] = {f.ratedRows, f.offRows, f.staleRows, f.firstStale, f.lastStale, f.ratedCols, f.offCols, f.firstOffRow,
                             f.lastOffRow, f.firstOffCol, f.lastOffCol, f.levelMilli, f.kind};
    std::memcpy(out, v, sizeof v);
}

// bmpWalk (host/bmpwalk.hpp: what the reading threads learn about a BMP before the GPU decodes it): 1 = a file decodeBMP
// reads as a W x H image (fields_out: data_off, stride, bpp, top-down, the table is the identity; lut_out[256]), 0 = not
int abh_bmp_walk(const uint8_t *data, int n, int W, int H, uint32_t *fields_out, uint8_t *lut_out)
{
    abub::BmpInfo info;
    if (n < 0 || !abub::bmpWalk(data, (size_t)n, W, H, info))
        return 0;
    fields_out[0] = info.dataOff;
    fields_out[1] = info.stride;
    fields_out[2] = (uint32_t)info.bpp;
    fields_out[3] = info.topDown ? 1 : 0;
    fields_out[4] = info.identity ? 1 : 0;
    std::memcpy(lut_out, info.lut, 256);
    return 1;
}

// cv::imwrite of the debug write-out (PNG, or BMP by extension)
// pngWalk (host/pngwalk.hpp: what RunBatched learns about a file before the GPU decodes it): 1 = a W x H 8-bit grey / palette PNG
// (segs_out: up to cap (offset, length) pairs of its IDAT chunks, *nsegs their number, *palette, lut_out[256]), 0 = a file
// for the host decoder
int abh_png_walk(const uint8_t *data, int n, int W, int H, uint32_t *segs_out, int cap, int *nsegs, int *palette, uint8_t *lut_out)
{
    abub::PngInfo info;
    if (!abub::pngWalk(data, (size_t)n, W, H, info))
        return 0;
    *nsegs = (int)info.segs.size();
    for (int i = 0; i < (int)info.segs.size() && i < cap; ++i) {
        segs_out[2 * i] = info.segs[i].off;
        segs_out[2 * i + 1] = info.segs[i].len;
    }
    *palette = info.palette ? 1 : 0;
    if (info.palette)
        std::memcpy(lut_out, info.lut, 256);
    return 1;
}

static int pngWalkOut(const uint8_t *data, int n, int W, int H, bool typed, bool adam7, uint32_t *segs_out, int cap, int *nsegs,
                      int *palette, uint8_t *lut_out, uint32_t *kind);
// pngWalk with typed = true (ABUB_GPU_PNG_TYPES=1): also the other PNG types the host decoder reads; *kind = 0 for an 8-bit
// grey / palette file, else colour type | bit depth << 8; the table also for a palette below 8 bits
int abh_png_walk_typed(const uint8_t *data, int n, int W, int H, uint32_t *segs_out, int cap, int *nsegs, int *palette, uint8_t *lut_out,
                       uint32_t *kind)
{
    return pngWalkOut(data, n, W, H, true, false, segs_out, cap, nsegs, palette, lut_out, kind);
}
// pngWalk with adam7 = true (ABUB_GPU_PNG_ADAM7=1) and typed as given: also Adam7-interlaced files of the kinds the walk takes
// anyway; *kind has ABUB_PNG_KIND_ADAM7 set for such a file
int abh_png_walk_adam7(const uint8_t *data, int n, int W, int H, int typed, uint32_t *segs_out, int cap, int *nsegs, int *palette,
                       uint8_t *lut_out, uint32_t *kind)
{
    return pngWalkOut(data, n, W, H, typed != 0, true, segs_out, cap, nsegs, palette, lut_out, kind);
}
static int pngWalkOut(const uint8_t *data, int n, int W, int H, bool typed, bool adam7, uint32_t *segs_out, int cap, int *nsegs,
                      int *palette, uint8_t *lut_out, uint32_t *kind)
{
    abub::PngInfo info;
    if (!abub::pngWalk(data, (size_t)n, W, H, info, typed, adam7))
        return 0;
    *nsegs = (int)info.segs.size();
    for (int i = 0; i < (int)info.segs.size() && i < cap; ++i) {
        segs_out[2 * i] = info.segs[i].off;
        segs_out[2 * i + 1] = info.segs[i].len;
    }
    *palette = info.palette ? 1 : 0;
    if (info.palette)
        std::memcpy(lut_out, info.lut, 256);
    *kind = info.kind;
    return 1;
}

int abh_imwrite(const char *path, const uint8_t *img, int W, int H)
{
    cv::Mat m(H, W, CV_8U);
    std::memcpy(m.data, img, (size_t)W * H);
    return cv::imwrite(path, m) ? 0 : -1;
}

void abh_run_free(void *r)
{
    Run *run = (Run *)r;
    for (auto &kv : run->trainers)
        delete kv.second;
    delete run->parser;
    delete run;
    abub::DeviceContext::releaseThread();
}

// frames: [F][H][W]; ok: F flags or NULL
int abh_run_add_event(void *r, const char *ev, int cam, const uint8_t *frames, int F, int W, int H, const uint8_t *ok)
{
    Run *run = (Run *)r;
    std::vector<cv::Mat> v;
    for (int k = 0; k < F; ++k) {
        cv::Mat m;
        if (!ok || ok[k]) {
            m.create(H, W, CV_8U);
            std::memcpy(m.data, frames + (size_t)k * W * H, (size_t)W * H);
        }
        v.push_back(m);
    }
    if (!run->mem)
        return -1;
    run->mem->AddFrames(ev, cam, v);
    return 0;
}

// Trainer over every event of the run (numeric order like AutoBubStart3.cpp:284)
int abh_train(void *r, int cam, int *status, int *tss, uint8_t *mu_out, uint8_t *sigma_out)
{
    Run *run = (Run *)r;
    try {
        const std::vector<std::string> events = abub::sortedEvents(*run->parser);
        delete run->trainers[cam];
        Trainer *t = new Trainer(cam, events, "", "cam%d_image%u.png", "", run->parser->clone(), false);
        run->trainers[cam] = t;
        t->MakeAvgSigmaImage(false);
        *status = t->StatusCode;
        *tss = t->TrainingSetSize;
        if (t->StatusCode == 0 && mu_out && sigma_out) {
            std::memcpy(mu_out, t->TrainedAvgImage.data, t->TrainedAvgImage.total());
            std::memcpy(sigma_out, t->TrainedSigmaImage.data, t->TrainedSigmaImage.total());
        }
        return 0;
    } catch (std::exception &e) {
        run->last.error = e.what();
        return -1;
    }
}

// Every camera 0..ncams-1 trained in one pass on the device (TrainOnDevice) over every event of the run; per camera c:
// status[c], tss[c] and, where it trained, its mu / sigma at mu_out + c * cap, sigma_out + c * cap (cap bytes each).  The
// Run's Trainers are replaced.  Returns 0 (trained on the device), 1 (TrainOnDevice declined the run: the host Trainer
// trained it), -1 on errors.  stats (may be NULL): [frames decoded by the GPU decoder, by host threads, decode launches,
// seconds, packed frames decoded by the GPU decoder (they count in the first, too), BMP frames likewise].
int abh_train_device(void *r, int ncams, int *status, int *tss, uint8_t *mu_out, uint8_t *sigma_out, int cap, double *stats)
{
    Run *run = (Run *)r;
    try {
        const std::vector<std::string> events = abub::sortedEvents(*run->parser);
        std::vector<Trainer *> trainers;
        for (int c = 0; c < ncams; ++c) {
            delete run->trainers[c];
            run->trainers[c] = new Trainer(c, events, "", "cam%d_image%u.png", "", run->parser->clone(), false);
            trainers.push_back(run->trainers[c]);
        }
        abub::DeviceTrainOptions to;
        std::string why;
        abub::DeviceTrainStats st;
        const int rc = abub::TrainOnDevice(run->parser, events, trainers, to, &st, &why);
        if (stats) {
            stats[0] = (double)st.framesGpuDecoded;
            stats[1] = (double)st.framesHostDecoded;
            stats[2] = (double)st.decodeLaunches;
            stats[3] = st.total_s;
            stats[4] = (double)st.framesGpuUnpacked;
            stats[5] = (double)st.framesGpuBmp;
            stats[6] = (double)st.framesGpuUnzipped;
        }
        if (rc != 0) {
            run->last.error = why;
            for (Trainer *t : trainers)
                t->MakeAvgSigmaImage(false);
        }
        for (int c = 0; c < ncams; ++c) {
            Trainer *t = trainers[c];
            status[c] = t->StatusCode;
            tss[c] = t->TrainingSetSize;
            if (t->StatusCode == 0 && mu_out && sigma_out && (int)t->TrainedAvgImage.total() <= cap) {
                std::memcpy(mu_out + (size_t)c * cap, t->TrainedAvgImage.data, t->TrainedAvgImage.total());
                std::memcpy(sigma_out + (size_t)c * cap, t->TrainedSigmaImage.data, t->TrainedSigmaImage.total());
            }
        }
        return rc != 0 ? 1 : 0;
    } catch (std::exception &e) {
        run->last.error = e.what();
        return -1;
    }
}

// install a model directly (tests that want a specific mu/sigma/TrainingSetSize)
int abh_set_model(void *r, int cam, const uint8_t *mu, const uint8_t *sigma, int W, int H, int tss)
{
    Run *run = (Run *)r;
    static unsigned long long next = 1ull << 40;
    delete run->trainers[cam];
    Trainer *t = new Trainer(cam, {}, "", "cam%d_image%u.png", "", run->parser->clone(), false);
    t->TrainedAvgImage.create(H, W, CV_8U);
    t->TrainedSigmaImage.create(H, W, CV_8U);
    std::memcpy(t->TrainedAvgImage.data, mu, (size_t)W * H);
    std::memcpy(t->TrainedSigmaImage.data, sigma, (size_t)W * H);
    t->TrainingSetSize = tss;
    t->ModelId = next++;
    run->trainers[cam] = t;
    return 0;
}

int abh_analyze(void *r, const char *ev, int cam, const char *maskdir)
{
    Run *run = (Run *)r;
    run->last.bubbles.clear();
    run->last.error.clear();
    auto it = run->trainers.find(cam);
    if (it == run->trainers.end() || !it->second) {
        run->last.error = "no trainer for camera";
        return -100;
    }
    Trainer *t = it->second;
    AnalyzerUnit *A = nullptr;
    try {
        A = new L3Localizer(ev, "", cam, true, &t, maskdir ? maskdir : "", run->parser->clone());
    } catch (std::exception &e) {
        run->last.error = e.what();
        return -100;
    }
    size_t rectsBegin = 0;
    run->last.staged = abub::analyzeUntilBubble(A, true, "", run->last.error, &rectsBegin);
    if (run->last.staged == -6)
        std::cout << run->last.error << '\n';
    run->last.capture(*A, rectsBegin);
    delete A;
    return run->last.staged;
}

// A whole run (every event of the Run's parser, cameras 0..ncams-1, the Run's trained models) through the batched
// pipeline into <outdir>abub3hs_<run>.txt; stats: [total_s, list_s, decode_s, gpu_s, write_s, frames, failed,
// batches, events_per_batch, gpus, frames decoded on the GPU, on host threads, gpudecode_s, packed frames decoded on the GPU, BMP frames decoded on the GPU].  Returns 0, 1 when the batched path declines the run, -1 on errors.
// peekDir (may be NULL): BatchedRunOptions::peekDir; peekOut (may be NULL): [stacks, files, bytes, 1 = GPU route, seconds].
int abh_run_batched_peek(void *r, int ncams, const char *maskdir, const char *outdir, const char *run_number, int frameOffset,
                         int ngpus, int nthreads, int decodeThreads, int batchMB, int shardRank, int shardWorld, double *statsOut,
                         const char *peekDir, double *peekOut)
{
    Run *run = (Run *)r;
    try {
        const std::vector<std::string> events = abub::sortedEvents(*run->parser);
        std::vector<Trainer *> trainers;
        for (int c = 0; c < ncams; ++c) {
            auto it = run->trainers.find(c);
            if (it == run->trainers.end() || !it->second) {
                run->last.error = "no trainer for camera";
                return -1;
            }
            trainers.push_back(it->second);
        }
        abub::BatchedRunOptions bo;
        bo.ngpus = std::max(1, ngpus);
        bo.hostThreads = std::max(1, nthreads);
        bo.decodeThreads = std::max(1, decodeThreads);
        if (batchMB > 0)
            bo.batchBytes = (size_t)batchMB << 20;
        bo.shardRank = shardRank;
        bo.shardWorld = std::max(1, shardWorld);
        bo.maskDir = maskdir ? maskdir : "";
        bo.peekDir = peekDir ? peekDir : "";
        abub::BatchedRunStats bs;
        std::string why;
        const int rc = abub::RunBatched(run->parser, events, trainers, ncams, outdir, run_number, frameOffset, bo, &bs, &why);
        if (rc != 0)
            run->last.error = why;
        if (statsOut) {
            const double v[17] = {bs.total_s, bs.list_s, bs.decode_s, bs.gpu_s, bs.write_s, (double)bs.frames, (double)bs.framesFailed,
                                  (double)bs.batches, (double)bs.eventsPerBatch, (double)bs.gpus, (double)bs.framesGpuDecoded,
                                  (double)bs.framesHostDecoded, bs.gpudecode_s, (double)bs.framesGpuUnpacked, (double)bs.framesGpuBmp,
                                  (double)bs.framesGpuUnzipped, bs.unzip_s};
            std::memcpy(statsOut, v, sizeof v);
        }
        if (peekOut) {
            const double v[5] = {(double)bs.peekStacks, (double)bs.peekFiles, (double)bs.peekBytes, (double)bs.peekGpu, bs.peek_s};
            std::memcpy(peekOut, v, sizeof v);
        }
        return rc;
    } catch (std::exception &e) {
        run->last.error = e.what();
        return -1;
    }
}
int abh_run_batched(void *r, int ncams, const char *maskdir, const char *outdir, const char *run_number, int frameOffset,
                    int ngpus, int nthreads, int decodeThreads, int batchMB, int shardRank, int shardWorld, double *statsOut)
{
    return abh_run_batched_peek(r, ncams, maskdir, outdir, run_number, frameOffset, ngpus, nthreads, decodeThreads, batchMB, shardRank,
                                shardWorld, statsOut, nullptr, nullptr);
}

// the host route's two peek planes (peek.hpp: peekPlanesHost); rects: nrects rows of x, y, w, h
void abh_peek_planes_host(const uint8_t *D, const uint8_t *trig, int W, int H, int cut, const int *rects, int nrects, uint8_t *thr,
                          uint8_t *pres)
{
    std::vector<cv::Rect> rs;
    for (int i = 0; i < nrects; ++i)
        rs.push_back(cv::Rect(rects[4 * i], rects[4 * i + 1], rects[4 * i + 2], rects[4 * i + 3]));
    abub::peekPlanesHost(D, trig, W, H, cut, rs, thr, pres);
}

// reference main(): header once per run (AutoBubStart3.cpp:250-251)
void abh_write_header(const char *outdir, const char *run_number, int frameOffset, int ncams)
{
    OutputWriter w(outdir, run_number, frameOffset, ncams);
    w.writeHeader();
}

// reference main() loop body for one event (AutoBubStart3.cpp:352-387): a writer per event, one
// L3Localizer per camera driven by AnyCamAnalysis, then the block is appended to abub3hs_<run>.txt
int abh_event_to_file(void *r, const char *ev, int actualEventNumber, int ncams, const char *maskdir,
                      const char *outdir, const char *run_number, int frameOffset)
{
    Run *run = (Run *)r;
    OutputWriter writer(outdir, run_number, frameOffset, ncams);
    std::vector<AnalyzerUnit *> analyzers;
    for (int cam = 0; cam < ncams; ++cam) {
        auto it = run->trainers.find(cam);
        if (it == run->trainers.end() || !it->second)
            return -100;
        Trainer *t = it->second;
        AnalyzerUnit *A = new L3Localizer(ev, "", cam, true, &t, maskdir ? maskdir : "", run->parser->clone());
        analyzers.push_back(A);
        abub::AnyCamAnalysis(A, cam, true, &writer, "", actualEventNumber);
    }
    writer.writeCameraOutput(); // before the analyzers (owners of the bubbles) go away
    for (AnalyzerUnit *A : analyzers)
        delete A;
    return 0;
}

// writer probe for CPU unit tests: per camera a status, a trigger frame and bubbles given as descriptor
// rows (x,y,w,h,area,radius,m00,m10,m01,cx,cy); first row of a bubble = genesis
void abh_writer_probe(const char *outdir, const char *run_number, int frameOffset, int ncams, int event,
                      const int *status, const int *frame0, const int *nbub, const int *ndesc, const double *desc)
{
    OutputWriter w(outdir, run_number, frameOffset, ncams);
    abub::StagedBubbles staged;
    int bi = 0, di = 0;
    for (int c = 0; c < ncams; ++c) {
        abub::StackResult res;
        res.staged = status[c];
        res.trig = frame0[c];
        for (int k = 0; k < nbub[c]; ++k, ++bi) {
            abub::BubbleOut bo{};
            for (int d = 0; d < ndesc[bi]; ++d, ++di)
                bo.desc.push_back(abub::descFromRow(desc + abub::kDescRow * (size_t)di));
            res.bubbles.push_back(bo);
        }
        staged.stage(w, res, c, event);
    }
    w.writeCameraOutput();
}

// A StackResult read out: `res` comes from abh_run_last (valid until the run's next call) or abh_pipe_stack (until the
// pipeline's next run).  state: staged, trig, status, loc_thres, ok, nbubbles
const void *abh_run_last(void *r) { return &((Run *)r)->last; }
const char *abh_last_error(void *r) { return ((Run *)r)->last.error.c_str(); }
void abh_result_state(const void *res, int *out)
{
    const abub::StackResult &r = *(const abub::StackResult *)res;
    const int v[6] = {r.staged, r.trig, r.status, r.loc_thres, r.ok, (int)r.bubbles.size()};
    std::memcpy(out, v, sizeof v);
}
// the rectangles of the result (StackResult::rects) as rows of x, y, w, h: at most cap rows are written, the count returned
int abh_result_rects(const void *res, int *out, int cap)
{
    const abub::StackResult &r = *(const abub::StackResult *)res;
    for (int i = 0; i < (int)r.rects.size() && i < cap; ++i) {
        out[4 * i] = r.rects[i].x;
        out[4 * i + 1] = r.rects[i].y;
        out[4 * i + 2] = r.rects[i].width;
        out[4 * i + 3] = r.rects[i].height;
    }
    return (int)r.rects.size();
}
const char *abh_result_error(const void *res) { return ((const abub::StackResult *)res)->error.c_str(); }
int abh_result_ndesc(const void *res, int b) { return (int)((const abub::StackResult *)res)->bubbles[b].desc.size(); }
void abh_result_desc(const void *res, int b, int d, double *out)
{
    abub::descToRow(((const abub::StackResult *)res)->bubbles[b].desc[d], out);
}
int abh_result_ndz(const void *res, int b) { return (int)((const abub::StackResult *)res)->bubbles[b].dz.size(); }
float abh_result_dz(const void *res, int b, int i) { return ((const abub::StackResult *)res)->bubbles[b].dz[i]; }
float abh_result_dzdt(const void *res, int b) { return ((const abub::StackResult *)res)->bubbles[b].dzdt; }
float abh_result_drdt(const void *res, int b) { return ((const abub::StackResult *)res)->bubbles[b].drdt; }

// host-logic probes for CPU-side unit tests (no GPU needed)
int abh_contours(const uint32_t *idx, int n, int W, int H, int *npts_out, int *xy_out, int cap_contours, int cap_pts)
{
    std::vector<uint32_t> v(idx, idx + n);
    std::vector<std::vector<cv::Point>> cs;
    abub::ContourFinder f;
    f.find(v, W, H, cs);
    int k = 0, used = 0;
    for (auto &c : cs) {
        if (k >= cap_contours || used + (int)c.size() > cap_pts)
            return -1;
        npts_out[k++] = (int)c.size();
        for (auto &p : c) {
            xy_out[2 * used] = p.x;
            xy_out[2 * used + 1] = p.y;
            ++used;
        }
    }
    return k;
}
int abh_binarize_threshold(const uint32_t *hist, int P, int tozero) { return abub::binarizeThresholdFromHist(hist, (size_t)P, tozero); }
float abh_entropy(const uint32_t *hist, int nbins, int P) { return abub::entropyFromHist(hist, nbins, (size_t)P); }
void abh_blob_stats(const int *xy, int n, double *out /*x,y,w,h,area,m00,m10,m01*/)
{
    std::vector<cv::Point> pts;
    for (int i = 0; i < n; ++i)
        pts.push_back(cv::Point(xy[2 * i], xy[2 * i + 1]));
    cv::Rect r = abub::boundingRectOf(pts);
    cv::Moments m = abub::momentsOf(pts);
    out[0] = r.x;
    out[1] = r.y;
    out[2] = r.width;
    out[3] = r.height;
    out[4] = abub::contourAreaOf(pts);
    out[5] = m.m00;
    out[6] = m.m10;
    out[7] = m.m01;
}
void abh_best_match(const unsigned long long *num, const unsigned long long *wsum2, int rw, int rh, const uint8_t *tmpl,
                    int tw, int th, float *bx, float *by)
{
    cv::Mat t(th, tw, CV_8U);
    std::memcpy(t.data, tmpl, (size_t)tw * th);
    abub::bestMatchFromTerms(num, wsum2, rw, rh, t, *bx, *by);
}
float abh_entropy_frame(const uint8_t *img, int W, int H)
{
    cv::Mat m(H, W, CV_8U);
    std::memcpy(m.data, img, (size_t)W * H);
    return calculateEntropyFrame(m);
}
// significance state machine probe: feeds histograms sequentially
void *abh_sig_new() { return new std::vector<std::vector<int>>(256); }
void abh_sig_free(void *s) { delete (std::vector<std::vector<int>> *)s; }
double abh_sig_eval(void *s, const uint32_t *hist, int P, int store, int tss, int *loc_thres)
{
    return abub::significanceFromHist(*(std::vector<std::vector<int>> *)s, hist, (size_t)P, store != 0, tss, 3, *loc_thres);
}
}
