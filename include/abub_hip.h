/*
 * abub_hip.h -- C ABI of the MI355X (gfx950) bubble-detection hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types, no exceptions.
 * The reference (picoexperiment/AutoBub3hs) is a single C++ process with no FFI of its own; these
 * entry points are what its AnalyzerUnit / L3Localizer / Trainer methods would bind for the
 * per-pixel work they delegate to OpenCV today.  Each entry cites the reference code it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the call sites a maintainer edits.
 *
 * Two layers:
 *   (A) abub_*_dev  : stateless launchers on DEVICE pointers + a hipStream_t (passed as void*).
 *                     Used by bench.py / tests with torch-owned HBM and by layer (B).
 *   (B) abub_ctx_*  : a per-host-thread context that owns HBM slabs (frame stack, model, scratch)
 *                     and moves HOST buffers in and out.  One ctx per host thread (the reference runs
 *                     one analyzer per OpenMP thread, AutoBubStart3.cpp:342); contexts are independent
 *                     and re-entrant.
 *
 * All functions return 0 on success or a negative code (ABUB_E_*); abub_last_error() gives text.
 * Images are single-channel u8, row-major, pitch == W.
 */
#ifndef ABUB_HIP_H
#define ABUB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ABUB_OK 0
#define ABUB_E_INVALID (-1)   /* bad argument (shape, null pointer, range) */
#define ABUB_E_HIP (-2)       /* HIP runtime error (see abub_last_error) */
#define ABUB_E_NODEVICE (-3)  /* no usable gfx950 device */
#define ABUB_E_OVERFLOW (-4)  /* caller-provided capacity too small (count still reported) */

/* A unit of K2/K3 work: indices (in frames) into a frame slab and a model slab. */
typedef struct {
    uint32_t cur;   /* frame index of the current frame in `frames`            */
    uint32_t ref;   /* frame index of the reference frame in `frames` (K2)      */
    uint32_t model; /* index into the [nmodels][H][W] sigma6 / mu slabs         */
    uint32_t out;   /* output slot: hist[out][256] and, if stored, img[out][H][W] */
} abub_job;
/* The `out` values of one launch's njobs jobs are a permutation of 0 .. njobs - 1 (the launchers clear and finalise
 * exactly those slots); a job need not write its own index.  Per-slot arguments (hist, diff / img, cthr, the list slot)
 * are indexed by `out`; per-job arguments (the jobs themselves, `incomplete` and `want` of the deferred pieces) by the
 * job's position in the list. */

const char *abub_last_error(void);
int abub_device_count(void);
/* name/CU count/HBM bytes of a device, e.g. for bench.py's config block */
int abub_device_info(int device, char *name, int name_cap, int *cus, uint64_t *hbm_bytes);

/* ------------------------------------------------------------------------------------------- */
/* (A) stateless device-pointer launchers                                                      */
/* ------------------------------------------------------------------------------------------- */

/* sigma6[i] = min(6*sigma[i], 255): the saturated `6*TrainedSigmaImage` operand of
 * AnalyzerUnit.cpp:351-352 and L3Localizer.cpp:782, computed once per model. n = bytes. */
int abub_sigma6_dev(const uint8_t *sigma, uint8_t *sigma6, size_t n, void *stream);

/* Fill jobs for regular stacks: `nstacks` stacks of F frames laid out [nstacks][F][H][W]; for stack s
 * and i in [first, first+count): cur = s*F+i, ref = s*F+max(i-ref_offset,0), model = s % nmodels,
 * out = s*count + (i-first).  (FindTriggerFrame's frame pairing, AnalyzerUnit.cpp:175-177,218,312-313.) */
int abub_fill_stack_jobs_dev(abub_job *jobs, int nstacks, int F, int first, int count, int ref_offset,
                             int nmodels, void *stream);

/* K2: fused AnalyzerUnit::ProcessFrame (AnalyzerUnit.cpp:346-377: two saturating differences
 * minus 6 sigma, 5x5 Gaussian of each, absdiff) + cv::calcHist 256 bins (AnalyzerUnit.cpp:456).
 *   frames  : [..][H][W] u8 slab            sigma6 : [nmodels][H][W] from abub_sigma6_dev
 *   jobs    : njobs entries (device)         hist   : [nslots][256] u32 (device), fully overwritten
 *   diff    : NULL (trigger-only mode, 3*W*H algorithmic bytes/job) or [nslots][H][W] u8
 *             (store mode, 4*W*H bytes/job)
 *   rows_per_chunk: 0 = auto.  Fast register-rolling kernel when abub_fast_path(W) != 0: W % 4 == 0 and
 *   W / 4 = ndw * lanes with ndw <= 8 dwords per lane and lanes <= 64 (so W <= 2048, and e.g. 268 = 4 * 67,
 *   536 and 2052 are not fast-path widths); generic LDS-tile kernel otherwise (same results). */
int abub_diff_hist_dev(const uint8_t *frames, const uint8_t *sigma6, const abub_job *jobs, int njobs,
                       int W, int H, uint32_t *hist, uint8_t *diff, int rows_per_chunk, void *stream);

/* Same on a sub-rectangle (ProcessFrame ROI overload, AnalyzerUnit.cpp:346: borders reflect at the
 * ROI edge, zeros outside).  One job; always the generic kernel. */
int abub_diff_roi_dev(const uint8_t *cur, const uint8_t *ref, const uint8_t *sigma6, int W, int H,
                      int rx, int ry, int rw, int rh, uint8_t *diff, uint32_t *hist, void *stream);

/* K1: Trainer::CalculateMeanSigmaImageVector (Trainer.cpp:144-216): float32 Welford over the
 * N frames `idx[0..N)` (device array of frame indices, NULL = 0..N-1) of `frames`.  Any byte address will do for
 * frames, mu and sigma: four pixels per thread with 4-byte loads and stores when W*H % 4 == 0 and all three are
 * 4-byte aligned, one pixel per thread otherwise, with the same bytes. */
int abub_train_dev(const uint8_t *frames, const uint32_t *idx, int N, int W, int H, uint8_t *mu,
                   uint8_t *sigma, void *stream);

/* K1b: histogram (256 bins) of the saturating difference f1 - f0 for npairs frame pairs
 * (Trainer.cpp:279 + the calcHist of :365); pairs[k] = {cur=f1, ref=f0, -, out}. */
int abub_pair_hist_dev(const uint8_t *frames, const abub_job *pairs, int npairs, int W, int H,
                       uint32_t *hist, void *stream);

/* K3: fused L3Localizer::CalculatePostTriggerFrameParams pixel stage (L3Localizer.cpp:779-785:
 * absdiff against mu, minus 6 sigma, 3x3 box blur) + 256-bin histogram (for the Otsu of :787).
 * jobs[k] = {cur, -, model, out}; img = [nslots][H][W] (may be NULL: histogram only). */
int abub_posttrig_dev(const uint8_t *frames, const uint8_t *mu, const uint8_t *sigma6,
                      const abub_job *jobs, int njobs, int W, int H, uint32_t *hist, uint8_t *img,
                      void *stream);

/* K4: binarize (v > thr[k]) + stream-compaction of foreground pixel indices, for nimg images
 * img[k] (the TOZERO + BINARY|OTSU mask of L3Localizer.cpp:252-254,786-787 with
 * thr = max(loc_thres, otsu)).  idx: [nimg][cap] u32 raster indices (unordered); count: [nimg]
 * (true counts, may exceed cap -> caller falls back to abub_fetch; nothing is written past cap).
 * Any thr: a negative one lists value-0 pixels too.  Any byte address will do for img: it is read 16 bytes at a time
 * when W*H % 16 == 0 and img is 16-byte aligned (so that every image is), a byte at a time otherwise, with the same
 * lists. */
int abub_fg_compact_dev(const uint8_t *img, int nimg, int W, int H, const int32_t *thr,
                        uint32_t *idx, int cap, uint32_t *count, void *stream);

/* Fused forms for the batched run pipeline: K2 / K3 as above, and every output pixel with value
 * > cthr[slot] is appended to ONE shared list, pairs[2k] = slot | value << 24, pairs[2k+1] = y*W+x
 * with slot = slot_base + job.out; cthr is indexed by job.out
 * (unordered; *count = true total, may exceed cap; count must be zeroed by the caller).  With the
 * list the images need not be materialised (diff / img may be NULL): cthr = the TOZERO threshold is
 * known before the launch, the final Otsu cut is applied to the listed values on the host.
 * These lists never hold value-0 pixels: a negative cthr lists like cthr = 0 (pixels with value >= 1).
 * Fast path only (abub_fast_path(W) != 0). */
int abub_fast_path(int W);

/* abub_diff_hist_dev without the stored image (trigger search, AnalyzerUnit.cpp:119-324) plus a hint about the job
 * list: it consists of blocks of `chain_len` consecutive jobs in which job q takes the cur frame of job q - chain_stride
 * as its ref and all share a model -- what abub_fill_stack_jobs_dev(first = 1, count = F - 1, ref_offset) produces
 * with chain_len = F - 1, chain_stride = ref_offset.  The kernels then load every frame row once for the two jobs
 * that use it.  The hint is verified on the device per chain; a list that does not have the structure gives the same
 * histograms, only slower.  chain_len = 0: no hint. */
int abub_diff_hist_chained_dev(const uint8_t *frames, const uint8_t *sigma6, const abub_job *jobs, int njobs, int W,
                               int H, uint32_t *hist, int chain_len, int chain_stride, void *stream);

/* Store-mode form of the same: D is written too ([nslots][H][W]); the scan writes the rows it proves zero, the listed
 * groups and the handed-over rows overwrite their pixels.  BASELINE configs[2] (10k-frame slab, i = 2..9999, ref = i-2)
 * is this call with chain_len = njobs, chain_stride = 2. */
int abub_diff_hist_chained_store_dev(const uint8_t *frames, const uint8_t *sigma6, const abub_job *jobs, int njobs, int W,
                                     int H, uint32_t *hist, uint8_t *diff, int chain_len, int chain_stride, void *stream);

/* Deferred pieces.  The trigger search stops at a stack's trigger frame (AnalyzerUnit.cpp:191, break at :307), but a batched
 * launch covers whole blocks of frames before the host knows where that is.  abub_diff_hist_chained_deferred_dev() is
 * abub_diff_hist_chained_dev() with the row machine left out: row ranges the bound scan hands over (dense frames) go to the
 * caller's `pieces` list (abub_k2_pieces_cap(njobs, W, H) entries of 8 bytes, `*npieces` used) and incomplete[job] (njobs
 * bytes) is set to 1 for every job that has some -- the histograms of exactly those jobs are not final.
 * abub_diff_hist_pieces_dev() then runs the row machine on the pieces of the jobs with want[job] != 0 (njobs bytes) and
 * finalises their histograms; same frames / sigma6 / jobs / njobs / hist as the deferred call.  incomplete[] and want[]
 * are indexed by job (position in `jobs`), the histograms by the job's slot: job j is completed in hist[jobs[j].out].  A job must be completed at
 * most once.  Needs abub_fast_path(W) and the "bound" option on. */
size_t abub_k2_pieces_cap(int njobs, int W, int H);
int abub_diff_hist_chained_deferred_dev(const uint8_t *frames, const uint8_t *sigma6, const abub_job *jobs, int njobs, int W,
                                        int H, uint32_t *hist, int chain_len, int chain_stride, void *pieces,
                                        uint32_t pieces_cap, uint32_t *npieces, uint8_t *incomplete, void *stream);
int abub_diff_hist_pieces_dev(const uint8_t *frames, const uint8_t *sigma6, const abub_job *jobs, int njobs, int W, int H,
                              uint32_t *hist, const void *pieces, const uint32_t *npieces, const uint8_t *want, void *stream);

/* Run-time tuning knobs of the K2 launchers (defaults from ABUB_K2_BOUND / _CHAIN / _BUDGET / _PF / _SPLIT / _LIST / _WG /
 * _SYNC / _SCANPF in the environment):
 *   "bound"  1 = bound-and-verify pass (default), 0 = the plain row machine for every row (the dense-regime worst case)
 *   "chain"  jobs per wave of the chained scan: 2 or 4 (>= 3 means 4); 0 = never chain; -1 (default) = 4
 *   "split"  1 (default) = the chained scan's whole-piece lane mapping wherever the row width allows it, 0 = never
 *   "budget" suspect groups a (job, chunk) may list in LDS before it hands its remaining rows to the row machine
 *   "list"   1 = suspect groups go to a global list that a second kernel evaluates exactly with the whole chip;
 *            0 (default) = every scanning wave evaluates its own suspects at its end
 *   "pf"     software-prefetch depth of the row machine (1 or 2)
 *   "scanpf" rows the chained scan fetches ahead: 1, 2, -1 (default) = 2 where instantiated (trigger-only, W = 1280 class)
 *   "wg"     waves per workgroup of the chained scan = consecutive segments of one chain (1 .. 8; -1 default = 1)
 *   "sync"   row steps a wave of such a workgroup may run ahead of its slowest wave (0 = never waits; -1 default = 0)
 *   "chunks" chunks per frame where the launcher picks the chunk height itself (rows_per_chunk = 0, the chained, deferred
 *            and compact forms); 0 (default) = automatic, else 1 .. 4096 (chunks are at least 16 rows high)
 * Results never depend on them.  abub_k2_pieces_cap() and abub_diff_hist_pieces_dev() recompute the deferred launch's
 * chunking, so the options must not change between a deferred call and the pieces calls that complete it.
 * Unknown names and bad values return ABUB_E_INVALID. */
int abub_k2_set_option(const char *name, int value);

/* 1 when abub_diff_hist_chained_deferred_dev() accepts W x H frames under the current K2 options (fast-path width and
 * the "bound" option on), else 0.  Callers decide per launch, since the options can change at any time. */
int abub_k2_deferred_ok(int W, int H);

/* Run-time tuning knobs of the K3 launcher (abub_posttrig_dev / abub_posttrig_compact_dev; defaults from ABUB_K3_SCAN /
 * _LIST / _BUDGET / _CHUNKS in the environment, read at first use):
 *   "scan"   1 (default) = zero scan with exact suspect groups, 0 = the row machine on every row
 *   "list"   1 (default) = suspect groups go to a global list that a second kernel evaluates, 0 = the scanning waves
 *            evaluate their own
 *   "budget" suspect groups a (job, chunk) may keep in LDS before it hands a piece of rows over: 0 .. 512 (default 512)
 *   "chunks" chunks per frame: 0 (default) = automatic, else 1 .. 4096 (chunks are at least 16 rows high)
 * Results never depend on them.  Unknown names and bad values return ABUB_E_INVALID. */
int abub_k3_set_option(const char *name, int value);

/* The bound-and-verify form of abub_diff_hist_dev keeps a work list in device scratch memory that the
 * library owns, one buffer per (device, stream), grown on demand.  Call this before destroying a stream that was
 * used for such launches (or at any quiet moment) to give its buffer back; it waits for the stream to drain. */
int abub_scratch_release(void *stream);

/* Diagnostics of the LAST bound-and-verify launch (K2 or K3) on `stream`, read back from that scratch buffer after the
 * stream has drained: counts[0] = row pieces handed over to the row machine (32 rows each at most), counts[1] = entries
 * of the global suspect list (0 when the scanning waves evaluate their own suspects).  Measurement only. */
int abub_bound_counts_dev(void *stream, uint32_t counts[2]);
int abub_diff_hist_compact_dev(const uint8_t *frames, const uint8_t *sigma6, const abub_job *jobs, int njobs,
                               int W, int H, uint32_t *hist, uint8_t *diff, const int32_t *cthr,
                               uint32_t *pairs, uint32_t cap, uint32_t *count, uint32_t slot_base,
                               void *stream);
int abub_posttrig_compact_dev(const uint8_t *frames, const uint8_t *mu, const uint8_t *sigma6,
                              const abub_job *jobs, int njobs, int W, int H, uint32_t *hist, uint8_t *img,
                              const int32_t *cthr, uint32_t *pairs, uint32_t cap, uint32_t *count,
                              uint32_t slot_base, void *stream);

/* Group such a list by slot on the device (counting sort): offsets[s] .. offsets[s+1] delimit slot s
 * in idx_out / val_out (raster index, value); offsets[nslots] = total (<= cap).  Only the first min(*count, cap)
 * entries are read; entries with slot >= nslots are dropped.  `count` is read on the
 * device, no host synchronisation needed between the producing launches and this call. */
int abub_pairs_group_dev(const uint32_t *pairs, const uint32_t *count, uint32_t cap, int nslots,
                         uint32_t *scratch /* [2*nslots] */, uint32_t *offsets /* [nslots+1] */,
                         uint32_t *idx_out /* [cap] */, uint8_t *val_out /* [cap] */, void *stream);

/* Same, with the per-slot counts taken from the producers' histograms (entries of slot s = pixels of hist[s]
 * with value > max(cthr[s], 0), the rule of the fused lists) instead of a counting pass over the list; valid when the
 * list did not overflow (on overflow nothing is written at or past idx_out[cap] / val_out[cap]).  A K4 list made with
 * a negative threshold holds value-0 pixels: group it with abub_pairs_group_dev. */
int abub_pairs_group_hist_dev(const uint32_t *pairs, const uint32_t *count, uint32_t cap, int nslots,
                              uint32_t *scratch, uint32_t *offsets, uint32_t *idx_out, uint8_t *val_out,
                              const uint32_t *hist /* [nslots][256] */, const int32_t *cthr /* [nslots] */,
                              void *stream);

/* K4, batched form: one shared output list for all nimg images, pairs[2*k] = image | value << 24,
 * pairs[2*k+1] = y*W+x (unordered); *count = true total (may exceed cap; nothing is written past cap).
 * Any thr and any address of img, as abub_fg_compact_dev. */
int abub_fg_compact_pairs_dev(const uint8_t *img, int nimg, int W, int H, const int32_t *thr,
                              uint32_t *pairs, uint32_t cap, uint32_t *count, void *stream);

/* Otsu threshold per slot on the device, bit for bit host/hostlogic.cpp binarizeThresholdFromHist (the TOZERO + BINARY|OTSU
 * cut of L3Localizer.cpp:252-254, 786-787): thr[s] = max(tozero[s], Otsu of hist[s] after TOZERO at tozero[s]) over
 * W*H pixels.  hist: [nslots][256] u32, tozero / thr: [nslots] int32 (device). */
int abub_binarize_thr_dev(const uint32_t *hist, const int32_t *tozero, int nslots, int W, int H, int32_t *thr, void *stream);

/* One 8-connected component of a slot's foreground: first (smallest) raster index, inclusive bbox, pixel count. */
typedef struct abub_blob {
    uint32_t first;
    int32_t x0, y0, x1, y1;
    uint32_t npix;
} abub_blob;

/* K4b: which candidate pixels belong to a blob that can matter, for the contour tracing of L3Localizer.cpp:254-256 and
 * :787-836 (cv::findContours on the thresholded image; tracking drops contours with box area <= 10, :800-805).
 * Input: a grouped candidate list (abub_pairs_group_dev / _hist_dev: offsets [nslots+1], idx / val [in_cap]; entries at
 * or past in_cap are never read), per slot thr (foreground = val > thr[s]) and min_box_area (a component is kept iff
 * bbox_w * bbox_h > min_box_area; -1 keeps everything).  Output, per slot s:
 *   kept_idx[kept_off[s] .. kept_off[s+1]) = the raster indices of every pixel of every kept component, increasing;
 *   ncomp[s] components, nkept_comp[s] of them kept; comp[comp_off[s] .. comp_off[s+1]) their descriptors in order of
 *   first raster index (comp may be NULL: no descriptors; then scratch sized with with_comp = 0).
 * Offsets are true counts; nothing is written at or past kept_idx[cap] / comp[comp_cap].  Exact and deterministic.
 * stats[4] (device, overwritten): slots labelled on the global-memory path, foreground pixels, components, kept components.
 * scratch: abub_label_blobs_scratch_bytes(nslots, W, H, in_cap, comp != NULL) bytes, 256-byte aligned. */
int abub_label_blobs_dev(const uint32_t *offsets, const uint32_t *idx, const uint8_t *val, uint32_t in_cap, int nslots, int W,
                         int H, const int32_t *thr, const int32_t *min_box_area, uint32_t *kept_off, uint32_t *kept_idx,
                         uint32_t cap, uint32_t *ncomp, uint32_t *nkept_comp, uint32_t *comp_off, abub_blob *comp,
                         uint32_t comp_cap, uint32_t *stats, void *scratch, size_t scratch_bytes, void *stream);
/* 0 for impossible shapes */
size_t abub_label_blobs_scratch_bytes(int nslots, int W, int H, uint32_t in_cap, int with_comp);

/* K5: the contours of each slot of a K4b kept list, traced on the device -- what cv::findContours(RETR_EXTERNAL,
 * CHAIN_APPROX_TC89_L1) returns for the thresholded image (L3Localizer.cpp:264, 374, 793), bit for bit what
 * host/hostlogic.cpp ContourFinder::find returns for the slot's kept pixels: the same contours in the same order (the
 * last discovered first), the same vertices in the order approxChainTC89L1 emits them.
 * Input: kept_off [nslots+1] / kept_idx of abub_label_blobs_dev (raster indices increasing within a slot; entries at or
 * past in_cap are never read), for images of W x H (each <= 65535).  Output, per slot s:
 *   status[s] = 0: traced.  cont_npts[cont_off[s] .. cont_off[s+1]) = the vertex count of each of its ncont[s] contours,
 *               pts[pt_off[s] .. pt_off[s+1]) = their vertices one after the other, one dword x | y << 16 each.
 *   status[s] = 1: declined (more than max_pixels kept pixels, or a border chain of more than max_chain codes, see
 *               abub_trace_contours_limits): ncont[s] = 0, nothing written; trace the slot on the host.
 * Offsets are true counts; nothing is written at or past cont_npts[cont_cap] / pts[pts_cap].  Exact and deterministic.
 * stats[4] (device, overwritten): slots traced, slots declined, contours, vertices.
 * scratch: abub_trace_contours_scratch_bytes(nslots, in_cap) bytes, 256-byte aligned. */
int abub_trace_contours_dev(const uint32_t *kept_off, const uint32_t *kept_idx, uint32_t in_cap, int nslots, int W, int H,
                            uint32_t *status, uint32_t *ncont, uint32_t *cont_off, uint32_t *cont_npts, uint32_t cont_cap,
                            uint32_t *pt_off, uint32_t *pts, uint32_t pts_cap, uint32_t *stats, void *scratch,
                            size_t scratch_bytes, void *stream);
/* Scratch of abub_trace_contours_dev (the contour tracing of L3Localizer.cpp:264, 374, 793); 0 for impossible shapes */
size_t abub_trace_contours_scratch_bytes(int nslots, uint32_t in_cap);
/* The limits under which abub_trace_contours_dev traces a slot (L3Localizer.cpp:264, 374, 793 stay on the host above
 * them): kept pixels per slot, Freeman codes per border chain.  Needs no device. */
int abub_trace_contours_limits(int *max_pixels, int *max_chain);

/* K6: AnalyzerUnit::FindTriggerFrame with calculateSignificanceFrame and CalcMean / CalcStdDev (AnalyzerUnit.cpp:119-324,
 * 435-504, 514-532) on finished 256-bin histograms that are already in device memory: one decision per stack, bit for bit
 * what host/AnalyzerUnit.cpp FindTriggerFrame makes of the same histograms (host/hostlogic.cpp significanceFromHist).
 * The histograms of a stack come in segments (the frame blocks of a lazy search); frame 0 has none. */
typedef struct abub_trig_seg {      /* frames [first, first + count) of one stack */
    const uint32_t *hist;           /* device: histogram of frame i at (i - first) * 256 */
    const uint8_t *pending;         /* device or NULL: pending[i - first] != 0 => that histogram is not final */
    int32_t first, count;
} abub_trig_seg;
typedef struct abub_trig_stack {
    uint32_t seg0, nseg;            /* its segments in the segment array, ascending, not overlapping */
    int32_t F;                      /* CameraFrames.size() of this stack */
    int32_t start;                  /* startframe (values < 1 mean 1) */
    int32_t tss;                    /* TrainingSetSize */
    int32_t first_bad;              /* smallest frame index with frameOk == false, or F */
} abub_trig_stack;
#define ABUB_TRIG_DONE 0            /* the search ran to its end: status / trig / loc_thres are the analyzer's new state */
#define ABUB_TRIG_NEED_FRAMES 1     /* no segment covers frame need_frame */
#define ABUB_TRIG_NEED_FINAL 2      /* a segment covers frame need_frame, but its pending flag is set */
#define ABUB_TRIG_BAD_LOOKAHEAD 3   /* a look-ahead frame is >= first_bad (the host search throws there) */
typedef struct abub_trig_result {
    int32_t state;                  /* ABUB_TRIG_* */
    int32_t status, trig;           /* TriggerFrameIdentificationStatus (0, -3, -9), MatTrigFrame (valid when status == 0, else 0) */
    int32_t loc_thres;              /* of the last store = true evaluation; -1: none ran, keep the old value */
    int32_t need_frame;             /* NEED_*: the first frame the search touched and could not read; else 0 */
    int32_t evaluated;              /* main-loop frames evaluated (statistics) */
    float sig;                      /* singleEntropy of the last main-loop frame */
    int32_t reserved;
} abub_trig_result;
#define ABUB_TRIG_MAX_PIXELS 2147483583 /* 2^31 - 65: the largest W * H abub_trigger_search_dev takes (see there) */
/* One search per stack (AnalyzerUnit.cpp:119-324, 435-504, 514-532), all in one launch.  stacks[nstacks] and segs[nsegs] are HOST arrays: they are checked here, before
 * anything is launched (a stack beyond abub_trigger_search_limits, overlapping segments: ABUB_E_INVALID), then copied to
 * `desc` on the stream -- device memory of abub_trigger_search_desc_bytes(nstacks, nsegs) bytes, 256-byte aligned; keep the
 * host arrays unchanged until the stream has passed the call.  out[nstacks] (device).  The search reports the first frame
 * the host search would have touched and cannot be read, counting the frames before `start` (its history) as touched
 * first: state NEED_FRAMES / NEED_FINAL with need_frame, every other field then as in a fresh record (status -3, trig 0,
 * loc_thres -1, evaluated 0, sig 0).  A frame behind a missing one never influences anything.  n < 5 gives DONE, -9.
 * sig_main: NULL, or device [nstacks][sig_pitch] doubles (sig_pitch >= every F): entry [s][i] receives the significance
 * of every main-loop frame i the search of stack s evaluated, when its state is DONE or BAD_LOOKAHEAD; other entries,
 * and the whole row of a search that needs frames, are left alone.
 * W * H <= ABUB_TRIG_MAX_PIXELS, else ABUB_E_INVALID: the search converts a float bin count and the float pixel counter
 * (`pix_rem -= binEntry`, AnalyzerUnit.cpp:493) to int, which is defined only below 2^31; no histogram bin of a W x H frame
 * and no value of the counter exceeds W * H, and (float)(W * H) is 2^31 - 128 up to 2^31 - 65 and 2^31 from 2^31 - 64 on. */
int abub_trigger_search_dev(const abub_trig_stack *stacks, const abub_trig_seg *segs, int nstacks, int nsegs, int W, int H,
                            void *desc, size_t desc_bytes, abub_trig_result *out, double *sig_main, int sig_pitch,
                            void *stream);
/* pending[j] = 0 for every j < n with done[j] != 0 (device arrays): the deferred flags of the jobs that
 * abub_diff_hist_pieces_dev has just completed (its `want`), so that the next search (AnalyzerUnit.cpp:119-324, 435-504,
 * 514-532) reads their histograms; queue it on the stream of that launch. */
int abub_trigger_clear_pending_dev(uint8_t *pending, const uint8_t *done, size_t n, void *stream);
/* Descriptor scratch of abub_trigger_search_dev (AnalyzerUnit.cpp:119-324, 435-504, 514-532); 0 for nstacks <= 0 */
size_t abub_trigger_search_desc_bytes(int nstacks, int nsegs);
/* The static limits of abub_trigger_search_dev (AnalyzerUnit.cpp:119-324, 435-504, 514-532 stay on the host above them):
 * frames per stack (F), segments per stack.  Needs no device. */
int abub_trigger_search_limits(int *max_frames, int *max_segs);

/* ---- K7: the localizer's arithmetic and decisions on K5's polygons (abub_localize.hip) ---------------------------------- */
/* One record per contour of abub_trace_contours_dev, in the order of its contour list: the columns of a descriptor row
 * (box, ContArea, ContRadius, m00, m10, m01, centroid) with the centroid in both forms the localizer uses. */
typedef struct abub_contour_desc {
    int32_t x, y, w, h;          /* cv::boundingRect */
    double area, radius;         /* fabs(cv::contourArea), sqrt(area / 3.14159) */
    double m00, m10, m01;        /* cv::moments of the polygon */
    float cx, cy;                /* tracking form: (float)(m10 / m00), NaN when m00 == 0 */
    float gx, gy;                /* genesis form: the vertex mean instead when m00 > 0 is false */
    uint32_t npts, reserved;
} abub_contour_desc;
/* K7a: describes every contour of a traced contour list (boundingRect, contourArea, moments and the centroid of
 * L3Localizer.cpp:401-418 and :808-823), bit for bit host/hostlogic.cpp boundingRectOf / contourAreaOf / momentsOf and
 * host/L3Localizer.cpp describe.  Input as abub_trace_contours_dev left it: status, cont_off [nslots+1], cont_npts,
 * pt_off [nslots+1], pts (x | y << 16); cont_cap / pts_cap: the capacities those lists were traced with.
 * desc[k] receives contour k for every k < min(cont_off[nslots], cont_cap, desc_cap) whose vertices lie below pts_cap;
 * nothing is written past desc_cap (the caller sees the true count in cont_off[nslots]). */
int abub_describe_contours_dev(const uint32_t *status, const uint32_t *cont_off, const uint32_t *cont_npts, uint32_t cont_cap,
                               const uint32_t *pt_off, const uint32_t *pts, uint32_t pts_cap, int nslots,
                               abub_contour_desc *desc, uint32_t desc_cap, void *stream);

typedef struct abub_loc_mask { /* the masks of one camera: device images of 8-bit pixels, rows of `w` bytes */
    const uint8_t *fid;        /* cam<N>_mask.bmp, or NULL: no mask dir / not loadable */
    const uint8_t *bel;        /* cam<N>_bellows_mask.bmp, or NULL */
    int32_t fw, fh, bw, bh;
} abub_loc_mask;
#define ABUB_LOC_MAXTRACK 10 /* NumFramesBubbleTrack */
typedef struct abub_loc_stack {
    int32_t cam;                       /* index into masks[] */
    int32_t genesis;                   /* slot of the genesis image */
    int32_t ntrack;                    /* tracking slots, in frame order (the caller applied L3Localizer.cpp:947-955) */
    int32_t bad;                       /* != 0: the stack holds an undecodable frame */
    int32_t track[ABUB_LOC_MAXTRACK];
    int32_t reserved[2];
} abub_loc_stack;
/* status of a stack after abub_localize_stacks_dev: 0 = localised, otherwise the host route takes it */
#define ABUB_LOC_DONE 0
#define ABUB_LOC_LIMIT 1       /* a slot over the contour limit, or more bubbles than the bubble limit */
#define ABUB_LOC_SLOT 2        /* a slot abub_trace_contours_dev declined (status 1) */
#define ABUB_LOC_BAD_FRAME 3   /* abub_loc_stack.bad */
#define ABUB_LOC_BELLOWS 4     /* every genesis contour lies in the bellows mask: the veto (L3Localizer.cpp:292-390) */
#define ABUB_LOC_INCOMPLETE 5  /* a slot's records lie beyond ndesc (the contour lists overflowed: redo the batch) */
typedef struct abub_loc_result {
    int32_t status;
    uint32_t nrects, rect_off;   /* bubbleRects: rects[4 * rect_off ..] = x, y, w, h of each, in order */
    uint32_t nbubbles;
    uint32_t ntrack, track_off;  /* tracks[track_off ..]: per bubble its descriptor count n, then n record indices (into
                                    desc[]) in sighting order, the genesis first; ntrack = nbubbles + all the counts */
    uint32_t reserved[2];
} abub_loc_result;
/* K7b: CalculateInitialBubbleParams and CalculatePostTriggerFrameParams with isInMask (L3Localizer.cpp:215-460, 764-869,
 * 971-1012) per stack on the records of abub_describe_contours_dev, one launch for all stacks.  stacks[nstacks] and
 * masks[ncams] are HOST arrays, checked here (a camera or slot index out of range, ntrack beyond ABUB_LOC_MAXTRACK:
 * ABUB_E_INVALID) and copied to `scratch` on the stream -- device memory of abub_localize_scratch_bytes(nstacks, ncams)
 * bytes, 256-byte aligned; keep them unchanged until the stream has passed the call.  slot_status / cont_off: of
 * abub_trace_contours_dev; desc[ndesc]: the records.  out[nstacks] (device) is written for every stack.  A stack with
 * status 0 reserves its part of `rects` (rect_cap boxes of 4 int32) and `tracks` (track_cap dwords); totals[2] (device,
 * zeroed here) count every reservation: a stack whose part would end beyond a capacity writes nothing there, so
 * totals[0] > rect_cap or totals[1] > track_cap asks for larger lists and another launch.  When several reasons decline
 * a stack the status is the first of BAD_FRAME, SLOT, INCOMPLETE, LIMIT, BELLOWS. */
int abub_localize_stacks_dev(const abub_loc_stack *stacks, int nstacks, const abub_loc_mask *masks, int ncams,
                             const uint32_t *slot_status, const uint32_t *cont_off, int nslots,
                             const abub_contour_desc *desc, uint32_t ndesc, void *scratch, size_t scratch_bytes,
                             abub_loc_result *out, int32_t *rects, uint32_t rect_cap, uint32_t *tracks, uint32_t track_cap,
                             uint32_t *totals, void *stream);
/* Descriptor scratch of abub_localize_stacks_dev (L3Localizer.cpp:215-460, 764-869, 971-1012); 0 for nstacks <= 0 */
size_t abub_localize_scratch_bytes(int nstacks, int ncams);
/* The static limits of abub_localize_stacks_dev (L3Localizer.cpp:215-460, 764-869, 971-1012 stay on the host above them):
 * contours per slot, bubbles per stack.  Needs no device. */
int abub_localize_limits(int *max_contours, int *max_bubbles);

/* Raw terms of cv::matchTemplate(CV_TM_CCORR_NORMED) for the bellows veto (L3Localizer::TrackAFeature,
 * L3Localizer.cpp:499-500): for each of the (W-tw+1) x (H-th+1) placements the exact integer sums
 * num = sum(T*I) and wsum2 = sum(I*I) over the window.  Normalisation is host work (double). */
int abub_match_ccorr_dev(const uint8_t *img, int W, int H, const uint8_t *tmpl, int tw, int th,
                         unsigned long long *num, unsigned long long *wsum2, void *stream);
/* Batched form of abub_match_ccorr_dev (same integers) for the bellows veto of many stacks at once
 * (L3Localizer.cpp:292-390, TrackAFeature :473-510, whose matchTemplate searches the whole frame, :485): job k
 * matches the template against frame frame_idx[k] of the slab `frames` ([..][H][W]); frame_idx: njobs u32 (device).
 * num / wsum2: [njobs][H-th+1][W-tw+1].  Limits: W <= 4096, tw <= 4093, th <= 66051 (the u32 column sums of the
 * window energy), njobs <= 65535, (W-tw+1) * (H-th+1) < 2^32 - 1 (placement indices are u32); beyond them, or with
 * tw > W, th > H or njobs <= 0 -> ABUB_E_INVALID before anything is launched. */
int abub_match_ccorr_batch_dev(const uint8_t *frames, int W, int H, const uint32_t *frame_idx, int njobs,
                               const uint8_t *tmpl, int tw, int th, unsigned long long *num, unsigned long long *wsum2,
                               void *stream);
/* The whole of TrackAFeature on the device (L3Localizer.cpp:499-510: CCORR_NORMED, normalize(NORM_MINMAX), minMaxLoc,
 * 3x3 sub-pixel centre of mass), bit for bit what the host's bestMatchFromTerms makes of the terms above:
 * best_xy[2k], best_xy[2k+1] = best match of job k (float x, y).  scratch: device memory of at least
 * abub_match_best_scratch_bytes(W, H, tw, th, njobs) bytes, 256-byte aligned (ABUB_E_INVALID if smaller or
 * misaligned).  The limits of abub_match_ccorr_batch_dev hold here too. */
int abub_match_best_batch_dev(const uint8_t *frames, int W, int H, const uint32_t *frame_idx, int njobs,
                              const uint8_t *tmpl, int tw, int th, float *best_xy, void *scratch, size_t scratch_bytes,
                              void *stream);
/* 0 for every shape the two entries above refuse */
size_t abub_match_best_scratch_bytes(int W, int H, int tw, int th, int njobs);
/* img = saturate(img - sub) in place + its 256-bin histogram (`overTheSigma -= diff_frame`, L3Localizer.cpp:362). */
int abub_subsat_hist_dev(uint8_t *img, const uint8_t *sub, int W, int H, uint32_t *hist, void *stream);

/* ------------------------------------------------------------------------------------------- */
/* (B) context API (host buffers in/out)                                                       */
/* ------------------------------------------------------------------------------------------- */

typedef struct abub_ctx abub_ctx;

/* One context per host thread; owns a frame slab for up to max_frames frames of W x H. */
int abub_ctx_create(abub_ctx **out, int device, int W, int H, int max_frames);
void abub_ctx_destroy(abub_ctx *ctx);

/* Trainer::CalculateMeanSigmaImageVector on N host frames (Trainer.cpp:316); fills host mu/sigma.
 * N is not limited by max_frames: a training set larger than the ctx slab gets a temporary device slab of
 * N frames for the call (the Welford recurrence needs every frame of a pixel in order).
 * The trained model becomes the context's current model.  The resident frame stack is given up, whatever N is:
 * the frame calls below are refused until the next abub_ctx_upload_stack.  Every frame pointer is checked
 * before the first copy (a null one: ABUB_E_INVALID, model and stack untouched). */
int abub_ctx_train(abub_ctx *ctx, const uint8_t *const *frames, int N, uint8_t *mu_out,
                   uint8_t *sigma_out);
/* 256-bin histogram of sat(f1 - f0) (training entropy veto, Trainer.cpp:279-280).  Uses the frame slab: the
 * resident frame stack is given up, as after abub_ctx_train. */
int abub_ctx_pair_hist(abub_ctx *ctx, const uint8_t *f0, const uint8_t *f1, uint32_t hist[256]);

/* Make (mu, sigma) the context's current model (AnalyzerUnit.cpp:27 deep-copies the Trainer per
 * analyzer; here the model lives once in HBM). */
int abub_ctx_set_model(abub_ctx *ctx, const uint8_t *mu, const uint8_t *sigma);

/* Upload the frame stack of one (event, camera): F host frame pointers (Parser::GetImage results).
 * F > max_frames or a null pointer among them: ABUB_E_INVALID, and the previous stack stays as it was. */
int abub_ctx_upload_stack(abub_ctx *ctx, const uint8_t *const *frames, int F);

/* Histograms of D(frame[i]; frame[max(i-ref_offset,0)]) for i in [first, first+count):
 * everything FindTriggerFrame needs (AnalyzerUnit.cpp:191-314).  hist_out: [count][256] host. */
int abub_ctx_diff_hist_batch(abub_ctx *ctx, int ref_offset, int first, int count, uint32_t *hist_out);

/* D(frame[i]; frame[ref]) materialised (L3Localizer.cpp:232); D_out/hist_out may be NULL.
 * The image stays resident as the context's "current image" for abub_ctx_foreground. */
int abub_ctx_diff_frame(abub_ctx *ctx, int i, int ref, uint8_t *D_out, uint32_t *hist_out);

/* ROI overload of ProcessFrame on resident frames (AnalyzerUnit.cpp:346, bellows path L3Localizer.cpp:355). */
int abub_ctx_diff_frame_roi(abub_ctx *ctx, int i, int ref, int rx, int ry, int rw, int rh, uint8_t *D_out,
                            uint32_t *hist_out);

/* Post-trigger image of frame i (L3Localizer.cpp:779-785) + histogram; becomes the current image. */
int abub_ctx_posttrig(abub_ctx *ctx, int i, uint8_t *O_out, uint32_t *hist_out);

/* Foreground pixels (v > thr) of the current image as raster indices; *n = true count.
 * Returns ABUB_E_OVERFLOW if *n > cap (idx_out then holds the first cap found).  Any cap: the context's index
 * buffers grow on demand beyond their initial 65536 entries (up to W*H). */
int abub_ctx_foreground(abub_ctx *ctx, int thr, uint32_t *idx_out, int cap, int *n);

/* Bellows veto: correlation terms of resident frame i against a host template (see abub_match_ccorr_dev);
 * num_out / wsum2_out: [(H-th+1)][(W-tw+1)] host arrays. */
int abub_ctx_match_template(abub_ctx *ctx, int i, const uint8_t *tmpl, int tw, int th, unsigned long long *num_out,
                            unsigned long long *wsum2_out);
/* current image = saturate(current image - sub) with sub a host image; returns the new histogram. */
int abub_ctx_subtract_image(abub_ctx *ctx, const uint8_t *sub, uint32_t *hist_out);
/* Replace the current image by a host image (re-install D after a ROI ProcessFrame used the slot). */
int abub_ctx_set_image(abub_ctx *ctx, const uint8_t *img);

/* Copy the current image to the host (debug write-out / overflow fallback). */
int abub_ctx_fetch_image(abub_ctx *ctx, uint8_t *out);

/* ---- PNG frames decoded on the GPU (abub_png.hip) -------------------------------------------------------------
 * Replaces, for batches of frames, the host decode behind Parser::GetImage (ZipParser.cpp:186-239, RawParser.cpp:30-47:
 * cv::imdecode / cv::imread = libpng + zlib).  The caller uploads the FILES as they are on disk and describes each
 * frame: where its IDAT chunks lie, where its zlib stream may be assembled, where the decoded frame goes.  Handles
 * 8-bit grey and 8-bit palette images without interlace, any filter type, any deflate block type; a frame the kernels
 * refuse gets a positive status (below) and is left as it is -- the caller decodes such a frame on the host.
 * abub_png_decode_typed_dev also takes the other non-interlaced PNG types (abub_png_frame.kind) and gives their 8-bit grey
 * value as cv::imdecode(..., 0) does.  abub_png_decode_adam7_dev (ABUB_GPU_PNG_ADAM7=1, off by default) also takes
 * Adam7-interlaced files of all 15 kinds (ABUB_PNG_KIND_ADAM7 in abub_png_frame.kind): the inflated stream is the scanlines of
 * the passes that have pixels, each pass filtered on its own; k_png_unfilter_adam7 runs one wave per (frame, pass) and stores
 * every pixel once, at its place in the frame.  The host decoder (cv::imdecode, cvlite.cpp) reads the same files and is the
 * definition (tests/test_png_adam7.py, tests/test_gpu_adam7.py, tests/test_gpu_adam7_routes.py).  The width limit is that of
 * the other entries.  All pointers are device pointers; nothing here reads host memory. */
typedef struct abub_png_seg {
    uint32_t off; /* byte offset of an IDAT chunk's DATA in `files` */
    uint32_t len; /* its length */
} abub_png_seg;
typedef struct abub_png_frame {
    uint32_t seg_begin; /* first entry of this frame in segs[] */
    uint32_t seg_count; /* its IDAT chunks, in file order */
    uint32_t zoff;      /* where the frame's zlib stream is assembled in `zbuf`: a multiple of 16, with room for zlen
                           rounded up to 16, plus 16 */
    uint32_t zlen;      /* sum of the segment lengths */
    uint32_t lut;       /* palette images: index of the frame's 256-byte palette-index -> grey table in `luts`;
                           0xffffffff for grey images */
    uint32_t kind;      /* 0: an 8-bit image, grey or palette by `lut` (abub_png_decode_dev reads nothing else here).
                           abub_png_decode_typed_dev: colour type | bit depth << 8 of one of the 13 typed kinds --
                           grey (0) at 1, 2, 4, 16 bits, palette (3) at 1, 2, 4 (`lut`: the table, its entries past the
                           palette 0), grey+alpha (4), RGB (2) and RGBA (6) at 8 and 16; `lut` is ignored elsewhere.
                           abub_png_decode_adam7_dev: any of these 15 values, with ABUB_PNG_KIND_ADAM7 or-ed in for an
                           Adam7-interlaced file (kind 0 with the flag: 8-bit grey, or 8-bit palette by `lut`) */
    uint64_t dst;       /* byte offset of the decoded W*H frame from `out` (a multiple of 4) */
} abub_png_frame;
#define ABUB_PNG_KIND_ADAM7 (1u << 16) /* abub_png_frame.kind: the file is Adam7-interlaced (abub_png_decode_adam7_dev only) */
/* status[frame] after abub_png_decode_dev: 0 = decoded */
#define ABUB_PNG_E_DESC 1       /* descriptor out of the stated buffer sizes */
#define ABUB_PNG_E_HEADER 2     /* zlib header (RFC 1950) */
#define ABUB_PNG_E_TRUNCATED 3  /* stream ends early */
#define ABUB_PNG_E_BLOCKTYPE 4  /* deflate block type 3 */
#define ABUB_PNG_E_STORED 5     /* stored block: LEN / NLEN mismatch */
#define ABUB_PNG_E_SYMBOLS 6    /* more than 286 literal/length or 30 distance codes */
#define ABUB_PNG_E_CODES 7      /* over-subscribed / incomplete code, bad repeat */
#define ABUB_PNG_E_NOEOB 8      /* no end-of-block code */
#define ABUB_PNG_E_CODE 9       /* invalid literal/length or distance code in the data */
#define ABUB_PNG_E_DISTANCE 10  /* distance reaches before the start of the output */
#define ABUB_PNG_E_TOOMUCH 11   /* more than H*(W+1) bytes (a typed frame: more than H*(its row bytes + 1); an Adam7 frame:
                                   more than the scanlines of its passes) */
#define ABUB_PNG_E_TOOLITTLE 12 /* fewer */
#define ABUB_PNG_E_ADLER 13     /* Adler-32 of the output differs from the trailer */
#define ABUB_PNG_E_FILTER 14    /* filter type above 4 */
#define ABUB_PNG_E_INTERNAL 15  /* the two waves of a stream lost each other (never expected) */
/* bytes of `rawbuf` one frame takes (its inflated, still filtered scanlines) */
size_t abub_png_raw_stride(int W, int H);
/* files: the uploaded file bytes (4-byte aligned, files_bytes of them); frames[nframes], segs[nsegs], luts[nluts][256];
 * zbuf / rawbuf: scratch (16-byte aligned; rawbuf >= nframes * abub_png_raw_stride); out: where frames go (out_bytes);
 * status[nframes] (written for every frame).  W: a multiple of 4 in [4, 2048]. */
int abub_png_decode_dev(const uint8_t *files, size_t files_bytes, const abub_png_frame *frames, int nframes,
                        const abub_png_seg *segs, int nsegs, const uint8_t *luts, int nluts, int W, int H,
                        uint8_t *zbuf, size_t zbuf_bytes, uint8_t *rawbuf, size_t rawbuf_bytes, uint8_t *out,
                        size_t out_bytes, int32_t *status, void *stream);
/* Typed frames.  Bytes of `rawbuf` a frame of `kind` takes: H * (ceil(W * samples * depth / 8) + 1), rounded up to 16, plus
 * 16; 0 for a kind outside the table.  Kind 0 gives abub_png_raw_stride(W, H). */
size_t abub_png_raw_stride_kind(int W, int H, uint32_t kind);
/* abub_png_decode_dev with abub_png_frame.kind honoured.  raw_stride: the bytes of `rawbuf` every frame of the launch
 * gets, a multiple of 16 (the largest abub_png_raw_stride_kind among the launch's frames; rawbuf >= nframes * raw_stride).
 * A frame of kind 0 goes through the kernels of abub_png_decode_dev; the others are unfiltered at their own filter
 * distance and converted to grey by a kernel of their own.  ABUB_PNG_E_DESC also for a kind outside the table and for a
 * frame whose scanlines do not fit raw_stride; TOOMUCH / TOOLITTLE are relative to the frame's own size. */
int abub_png_decode_typed_dev(const uint8_t *files, size_t files_bytes, const abub_png_frame *frames, int nframes,
                              const abub_png_seg *segs, int nsegs, const uint8_t *luts, int nluts, int W, int H,
                              uint8_t *zbuf, size_t zbuf_bytes, uint8_t *rawbuf, size_t rawbuf_bytes, size_t raw_stride,
                              uint8_t *out, size_t out_bytes, int32_t *status, void *stream);
/* Adam7 frames.  Bytes of `rawbuf` a frame of `kind` takes.  With ABUB_PNG_KIND_ADAM7 set: the scanlines of the seven passes,
 * sum over the passes with pixels of ph * (ceil(pw * samples * depth / 8) + 1) (pass p: origin (x0, y0), step (dx, dy), pw =
 * ceil((W - x0) / dx) or 0, ph likewise), rounded up to 16, plus 16.  Without it: abub_png_raw_stride_kind(W, H, kind).  0 for
 * a kind outside the table. */
size_t abub_png_raw_stride_adam7(int W, int H, uint32_t kind);
/* abub_png_decode_typed_dev with ABUB_PNG_KIND_ADAM7 honoured (in the two other entries a kind with that bit is what it always
 * was: ignored by abub_png_decode_dev, ABUB_PNG_E_DESC in abub_png_decode_typed_dev).  raw_stride: the largest
 * abub_png_raw_stride_adam7 among the launch's frames.  Frames without the flag go through the kernels of a typed launch.  A
 * flagged frame is inflated to the size of its passes (TOOMUCH / TOOLITTLE are relative to it) and unfiltered, converted and
 * stored by k_png_unfilter_adam7, one wave per pass; every pixel of the frame is written exactly once, so a decoded frame needs
 * no clearing, and a refused one (any positive status; ABUB_PNG_E_FILTER from any pass) may be partly written.
 * ABUB_PNG_E_DESC as in a typed launch, the frame's passes in place of its scanlines. */
int abub_png_decode_adam7_dev(const uint8_t *files, size_t files_bytes, const abub_png_frame *frames, int nframes,
                              const abub_png_seg *segs, int nsegs, const uint8_t *luts, int nluts, int W, int H,
                              uint8_t *zbuf, size_t zbuf_bytes, uint8_t *rawbuf, size_t rawbuf_bytes, size_t raw_stride,
                              uint8_t *out, size_t out_bytes, int32_t *status, void *stream);

/* ---- packed frames ("ABF1") decoded on the GPU (abub_abf.hip) ---------------------------------------------------
 * The frame format of repacked runs (abub3hs --repack; layout and rules: DESIGN section 3, "Packed frames"; host codec: cv::abfEncode /
 * cv::abfDecodeInto).  Lossless, about the size of the PNG, every row and every 64-pixel block decodable on its own:
 * the decode needs no more than one read of the file and one write of the frame (the design goal; what the kernel
 * reaches: DESIGN).  The caller uploads the FILES as they are on disk;
 * the kernel trusts nothing in them: every offset is checked against the file's stated length, and that against
 * files_bytes, before it is used; nothing is read outside `files`, nothing written outside a frame's own W*H bytes. */
typedef struct abub_abf_frame {
    uint32_t off, len; /* the file in `files` (no alignment rule) */
    uint64_t dst;      /* byte offset of the decoded W*H frame from `out` (no alignment rule) */
} abub_abf_frame;
/* status[frame] after abub_abf_decode_dev: 0 = decoded.  1-3 are found identically by every wave of the frame and win;
 * of 4-6 (found per row) the largest wins.  A refused frame may be half written. */
#define ABUB_ABF_E_DESC 1   /* descriptor outside files_bytes / out_bytes */
#define ABUB_ABF_E_HEADER 2 /* magic, W, H, nblk */
#define ABUB_ABF_E_SIZE 3   /* len != computed file size */
#define ABUB_ABF_E_WIDTH 4  /* a width above 8 */
#define ABUB_ABF_E_ROWS 5   /* row offsets inconsistent */
#define ABUB_ABF_E_CHECK 6  /* a row check differs */
/* One launch per batch; every pointer is a device pointer; W, H in [1, 65535]; status[nframes] is written for every
 * frame.  Null pointers, nframes < 0 and W or H out of range: ABUB_E_INVALID before anything touches the device. */
int abub_abf_decode_dev(const uint8_t *files, size_t files_bytes, const abub_abf_frame *frames, int nframes, int W, int H,
                        uint8_t *out, size_t out_bytes, int32_t *status, void *stream);

/* ---- BMP frames decoded on the GPU (abub_bmp.hip) -------------------------------------------------------------------
 * Replaces the cv::imread / cv::imdecode of a BMP frame (RawParser.cpp:34-47, ZipParser.cpp:186-239) for the series whose
 * cameras wrote BMP; host definition: decodeBMP (host/cvlite.cpp), bit for bit.  The caller uploads the FILES as they are
 * on disk and walks each header on the host (host/bmpwalk.hpp); the kernel never reads a header and believes the descriptor
 * alone, which every wave of a frame checks against the stated sizes before it reads a pixel: off + len <= files_bytes,
 * data_off + stride * H <= len, stride >= ceil(W * bpp / 8), bpp one of the five, lut == 0xffffffff or < nluts,
 * dst + W * H <= out_bytes.  A frame that fails one gets ABUB_BMP_E_DESC and not one byte of `out`; nothing is read
 * outside `files`, nothing written outside a frame's own W*H bytes.  Output row y is stored row (top-down ? y : H-1-y);
 * 8, 4 (high nibble first) and 1 bit (bit 7 first) pixels go through the frame's table (or stay the index), 24 and 32 bit
 * pixels are (b*1868 + g*9617 + r*4899 + 8192) >> 14 of bytes 0, 1, 2. */
typedef struct abub_bmp_frame {
    uint32_t off, len;   /* the file inside `files` */
    uint32_t data_off;   /* of the pixel array inside the file */
    uint32_t stride;     /* bytes from one stored row to the next */
    uint16_t bpp, flags; /* 1 | 4 | 8 | 24 | 32; bit 0: top-down */
    uint32_t lut;        /* index of a 256-byte table, 0xffffffff = none (identity / no palette) */
    uint64_t dst;        /* byte offset of the W*H frame in `out` (no alignment rule) */
} abub_bmp_frame;        /* 32 bytes */
/* status[frame] after abub_bmp_decode_dev: 0 = decoded */
#define ABUB_BMP_E_DESC 1 /* descriptor outside the stated sizes, or not a shape the kernel takes */
/* One launch per batch; every pointer is a device pointer; luts[nluts][256] may be null only when nluts == 0; W, H in
 * [1, 65535]; status[nframes] is written for every frame.  Null pointers, negative counts and W or H out of range:
 * ABUB_E_INVALID before anything touches the device; nframes == 0: ABUB_OK, nothing touched.  No host synchronisation,
 * no allocation. */
int abub_bmp_decode_dev(const uint8_t *files, size_t files_bytes, const abub_bmp_frame *frames, int nframes,
                        const uint8_t *luts, int nluts, int W, int H, uint8_t *out, size_t out_bytes, int32_t *status,
                        void *stream);

/* ---- deflated zip entries inflated on the GPU (abub_png.hip) ---------------------------------------------------------
 * Replaces, for batches of archive entries of method 8, the zlib inflate of ZipParser::readEntry (host/ZipParser.cpp) that
 * ZipParser::ReadImageFile runs on the reading thread.  A zip entry is a RAW deflate stream (RFC 1951): no header, no
 * trailer; its output length and CRC-32 come from the archive's central directory and differ from entry to entry.  The
 * caller uploads the COMPRESSED bytes as they lie in the archive; the inflate is k_png_inflate's (same device functions,
 * the raw mode a template parameter: the stream starts at bit 0 and is read in place, no Adler-32), a second kernel takes
 * the CRC-32 of every inflated entry.  Every descriptor is checked against comp_bytes and out_bytes before a byte is read:
 * a bad one gets ABUB_ZIP_E_DESC and not one byte of `out`; nothing is read outside `comp`, nothing written outside
 * [dst, dst + align16(ulen)) of an entry.  Acceptance is ZipParser::readEntry's (zlib's Z_FINISH on a raw stream): status 0
 * iff the stream reaches its final block's end having produced exactly ulen bytes -- input behind that point is ignored,
 * ulen == 0 with an empty final block is accepted -- and their CRC-32 is `crc`.  A refused entry (positive status) may be
 * partly or wholly written inside its own range; the caller inflates it on the host.  clen or ulen >= 2^28:
 * ABUB_ZIP_E_DESC. */
typedef struct abub_zip_entry {
    uint32_t off, clen;  /* the raw deflate stream in `comp`: off a multiple of 16; clen rounded up to 16, plus 16, readable */
    uint32_t ulen, crc;  /* exactly ulen bytes are expected; their CRC-32 (the zip / IEEE one) */
    uint64_t dst;        /* byte offset of the inflated file from `out`: a multiple of 16, room for ulen rounded up to 16 */
} abub_zip_entry;        /* 24 bytes */
/* status[entry] after abub_unzip_dev: 0 = inflated and checked.  The deflate findings keep the numbers of
 * ABUB_PNG_E_TRUNCATED ... ABUB_PNG_E_TOOLITTLE and ABUB_PNG_E_INTERNAL (TOOMUCH / TOOLITTLE: more / fewer than ulen bytes;
 * a stream cut short is ABUB_PNG_E_TRUNCATED whatever the bytes behind it in `comp` are: they are read as zeros.  Near the
 * stream's end ABUB_PNG_E_TRUNCATED can stand for either: an invalid code that starts inside the last 48 bits, or a block
 * header error inside the last 14, is reported as TRUNCATED although the stream may be complete and wrong -- the kernel does
 * not tell a code the missing bits would have completed from one they made). */
#define ABUB_ZIP_E_DESC 1 /* descriptor outside comp_bytes / out_bytes, misaligned, or a length of 2^28 and more */
#define ABUB_ZIP_E_CRC 16 /* exactly ulen bytes came out, but their CRC-32 is not `crc` */
/* Two launches on `stream` (inflate: one workgroup of two waves per entry, 40 KiB of LDS; ABUB_PNG_WAVES=1: one wave; then
 * the CRC-32: one workgroup per entry); every pointer is a device pointer, comp and out 16-byte aligned; status[nentries]
 * is written for every entry.  Null pointers, nentries < 0 or a misaligned buffer: ABUB_E_INVALID before anything touches
 * the device; nentries == 0: ABUB_OK, nothing touched.  No host synchronisation, no allocation. */
int abub_unzip_dev(const uint8_t *comp, size_t comp_bytes, const abub_zip_entry *entries, int nentries,
                   uint8_t *out, size_t out_bytes, int32_t *status, void *stream);
/* The CRC kernel alone: crc[e] = CRC-32 (zlib.crc32) of the ulen bytes at buf + dst of entry e (off, clen and crc are not
 * looked at); status[e] = 0, or ABUB_ZIP_E_DESC (dst not a multiple of 16, dst + align16(ulen) > buf_bytes, ulen >= 2^28:
 * nothing read, crc[e] untouched).  Arguments as for abub_unzip_dev. */
int abub_crc32_dev(const uint8_t *buf, size_t buf_bytes, const abub_zip_entry *entries, int nentries, uint32_t *crc,
                   int32_t *status, void *stream);

/* ---- packed frames ("ABF1") encoded on the GPU (abub_abf_enc.hip) -------------------------------------------------
 * What cv::abfEncode does on a host thread, for a batch of resident frames: file f is exactly the bytes
 * cv::abfEncode(pixels + src[f], W, H) writes (the host encoder is canonical: smallest width per block, zero padding
 * bits, zero table padding).  The files lie in `out` in frame order, each at a multiple of 16: off[0] = 0,
 * off[f + 1] = align16(off[f] + len[f]); nothing is written between them, nothing at or behind out + out_cap.
 * *total = off + len of the last file, a true count whatever out_cap is: a caller whose buffer was too small grows it
 * and encodes the batch again.  Four launches on `stream` (measure, place rows, place files, write: DESIGN), no host
 * synchronisation. */
/* the largest file of a W x H frame: 32 + 8 * H + pad4(H * ceil(W / 64)) + W * H (every block 8 bits wide);
 * 0 if W or H is outside [1, 65535] or the value is >= 2^32 */
size_t abub_abf_file_bound(int W, int H);
/* bytes of `scratch` a launch over nframes frames needs; 0 for arguments abub_abf_encode_dev refuses */
size_t abub_abf_encode_scratch_bytes(int nframes, int W, int H);
typedef struct abub_abf_file {
    uint64_t off;   /* of the file from `out` */
    uint32_t len;   /* its length */
    int32_t status; /* 0 = written */
} abub_abf_file;
#define ABUB_ABF_ENC_E_SRC 1 /* src + W*H > pixels_bytes: nothing read, len = 0, takes no room */
#define ABUB_ABF_ENC_E_CAP 2 /* off + len > out_cap: off and len are true, none of the file's bytes is written */
/* pixels: frames of W*H bytes anywhere in a buffer of pixels_bytes (the slab the decoders wrote, for one); src[nframes]:
 * byte offset of each frame from `pixels`, any alignment; files[nframes] and *total are written for every launch with
 * nframes > 0.  src, files, total and scratch are device memory, 8-byte aligned.  Null pointers, nframes < 0, W or H
 * outside [1, 65535], abub_abf_file_bound(W, H) == 0, a scratch smaller than abub_abf_encode_scratch_bytes or misaligned:
 * ABUB_E_INVALID before anything touches the device.  nframes == 0: ABUB_OK, nothing is touched. */
int abub_abf_encode_dev(const uint8_t *pixels, size_t pixels_bytes, const uint64_t *src, int nframes, int W, int H,
                        uint8_t *out, size_t out_cap, abub_abf_file *files, uint64_t *total, void *scratch,
                        size_t scratch_bytes, void *stream);

/* ---- canonical Huffman-only PNG files written on the GPU (abub_png_enc.hip) ------------------------------------------
 * What cv::pngHuffEncode does on a host thread, for a batch of resident frames (abub3hs --unpack --unpack-gpu; the format's
 * rules, the launches and the limits: DESIGN section 3, "Unpacking a run"): file f is exactly the bytes
 * cv::pngHuffEncode(pixels + src[f], W, H) writes -- an ordinary 8-bit grey PNG with the Sub filter on every row and one
 * dynamic-Huffman deflate block of literals.  The conventions are those of abub_abf_encode_dev, and its record type and
 * status codes are reused: the files lie in `out` in frame order, each at a multiple of 16; nothing is written between
 * them, nothing at or behind out + out_cap; *total is a true count whatever out_cap is; ABUB_ABF_ENC_E_SRC takes no room,
 * ABUB_ABF_ENC_E_CAP writes none of the file's bytes.  Every byte of `out` is stored once with a plain store (a byte that
 * two rows share is written by the row its first bit lies in); `out` is not cleared and not read before it is written.
 * A memset and eight launches on `stream`, no host synchronisation, no allocation. */
/* the longest file of a W x H frame: 63 + ceil((1880 + 15 * (H * (W + 1) + 1)) / 8) (15 bits per symbol, the longest
 * header, the container); 0 if W or H is outside [1, 65535] or the value is >= 2^32 */
size_t abub_png_file_bound(int W, int H);
/* bytes of `scratch` a launch over nframes frames needs; 0 for arguments abub_png_encode_dev refuses */
size_t abub_png_encode_scratch_bytes(int nframes, int W, int H);
/* Arguments as for abub_abf_encode_dev.  Null pointers, nframes < 0, W or H outside [1, 65535], abub_png_file_bound(W, H)
 * == 0, a scratch smaller than abub_png_encode_scratch_bytes or misaligned: ABUB_E_INVALID before anything touches the
 * device.  nframes == 0: ABUB_OK, nothing is touched. */
int abub_png_encode_dev(const uint8_t *pixels, size_t pixels_bytes, const uint64_t *src, int nframes, int W, int H,
                        uint8_t *out, size_t out_cap, abub_abf_file *files, uint64_t *total, void *scratch,
                        size_t scratch_bytes, void *stream);

/* ---- resident files packed into a segment of a zip archive (abub_zip_pack.hip) ----------------------------------------
 * The files a GPU encoder left in device memory become stored entries of the canonical archive of abub3hs --archive
 * ("A run as one archive"; the host writer host/zipwrite.cpp is the definition).  Per item the call
 * writes exactly [dst, dst + 30 + name_len + extra_len + len) of `seg`: the local header with the CRC-32 in it (signature
 * 0x04034b50, version 20, flags 0, method 0, time 0, date 0x0021, crc, len, len, name_len, extra_len), the name, the
 * padding field (u16 0x4241, u16 extra_len - 4, zeros; none when extra_len is 0) and the len bytes from buf + src.  It
 * writes crc[i] (zlib.crc32 of those bytes) and status[i] = 0.  Nothing else of `seg` is touched and `seg` is never read;
 * the gaps between the items are the host's.  Two items may name the same src; their dst ranges must not overlap.
 * An item is refused with status[i] = ABUB_ZIP_E_DESC, crc[i] = 0 and not one byte of `seg` written when: src is no
 * multiple of 16 or [src, src + len) leaves buf_bytes; len is 2^32 - 1; [name, name + name_len) leaves names_bytes;
 * extra_len is 1, 2 or 3; [dst, dst + 30 + name_len + extra_len + len) leaves seg_bytes; or len > 0 and
 * dst + 30 + name_len + extra_len is no multiple of 16 (an item of length 0 has no data to align).
 * ABUB_ZIP_PACK_TILE bytes of a file are one tile: the second launch runs over (item, tile), loads every source byte once
 * with 16-byte loads for both its store and its CRC, and adds the tile's CRC register, moved over the bytes behind the
 * tile by a carry-less multiplication with x^(8 * bytes), into crc[i] (xor is commutative: the result does not depend on
 * the order).  Three launches on `stream` (check the descriptors and clear crc; the tiles; condition the CRCs and write
 * the headers): every dependence between workgroups is a launch boundary.  Every pointer is a device pointer, buf and seg
 * 16-byte aligned, items 8-byte, crc and status 4-byte.  Null pointers, nitems < 0 or a misaligned pointer: ABUB_E_INVALID
 * before anything touches the device; nitems == 0: ABUB_OK, nothing touched.  No host synchronisation, no allocation. */
#define ABUB_ZIP_PACK_TILE 65536
typedef struct abub_zip_item {
    uint64_t src;        /* the file's bytes at buf + src, a multiple of 16 */
    uint64_t dst;        /* its local header at seg + dst; dst + 30 + name_len + extra_len is a multiple of 16 */
    uint32_t len;        /* < 2^32 - 1 */
    uint32_t name;       /* the name at names + name */
    uint16_t name_len, extra_len;
    uint32_t reserved;
} abub_zip_item;         /* 32 bytes */
int abub_zip_pack_dev(const uint8_t *buf, size_t buf_bytes, const abub_zip_item *items, int nitems,
                      const uint8_t *names, size_t names_bytes, uint8_t *seg, size_t seg_bytes,
                      uint32_t *crc, int32_t *status, void *stream);

/* ---- resident frames compared byte for byte (abub_compare.hip) ------------------------------------------------------
 * What memcmp of two decoded frames, and a byte loop behind it, does on a host thread, for a batch of resident frames:
 * results[p] says how many of the frame_bytes bytes at a + pairs[p].a and b + pairs[p].b differ, where the first one is
 * and how far apart the two sides get.  The check of a repacked run against its source (abub3hs --verify-repack
 * --verify-gpu; verdicts and mapping: DESIGN section 3, "Verifying a repacked run").  Two launches on `stream` (the
 * records' initial state, then pairs x 16 KiB tiles), no host synchronisation, no allocation; a tile without a
 * difference issues no atomic, and the three atomics of one with a difference commute: the records are deterministic. */
typedef struct abub_cmp_pair { uint64_t a, b; } abub_cmp_pair;   /* byte offsets of the two frames from `a` and `b`; no alignment rule */
typedef struct abub_cmp_result {
    uint32_t status;  /* 0, or ABUB_CMP_E_RANGE */
    uint32_t ndiff;   /* bytes that differ */
    uint32_t first;   /* lowest index of a differing byte; 0xffffffff when ndiff == 0 */
    uint32_t max_abs; /* largest |a[i] - b[i]|; 0 when ndiff == 0 */
} abub_cmp_result;
#define ABUB_CMP_E_RANGE 1 /* a + frame_bytes > a_bytes or b + frame_bytes > b_bytes: nothing of the pair is read; ndiff 0, first 0xffffffff, max_abs 0 */
/* Every pointer is a device pointer; pairs and results are 8-byte aligned; a and b may be the same buffer; frame_bytes in
 * [1, 2^32 - 2].  results[npairs] is written in full by every call with npairs > 0, whatever it held before.  Frames
 * whose addresses are congruent mod 16 are read 16 bytes at a time; any other combination is as exact, and slower.  Null
 * pointers, npairs < 0, frame_bytes out of range or a misaligned pairs / results: ABUB_E_INVALID before anything touches
 * the device.  npairs == 0: ABUB_OK, nothing is touched. */
int abub_frames_compare_dev(const uint8_t *a, size_t a_bytes, const uint8_t *b, size_t b_bytes, const abub_cmp_pair *pairs,
                            int npairs, size_t frame_bytes, abub_cmp_result *results, void *stream);

/* ---- per-frame statistics of resident frames (abub_stats.hip) -------------------------------------------------------
 * What a survey of a run (abub3hs --survey; record, pairing and report: DESIGN section 3, "Surveying a run") wants to know
 * of every frame without analysing any, for a batch of resident frames: results[j] holds, over the frame_bytes pixels p at
 * frames + jobs[j].cur, the grey-level range, sum and sum of squares and the counts of black (0) and saturated (255)
 * pixels; with m and s the bytes of `mu` and `sigma6` at jobs[j].model (sigma6 = min(6 sigma, 255), abub_sigma6_dev; a
 * sigma that truncates to 0, reference Trainer.cpp:191-195, gives s = 0) the count and sum of sat(|p - m| - s), the
 * post-trigger image before its box filter (reference L3Localizer.cpp:779-787); and with r the bytes at frames +
 * jobs[j].ref the count and sum of sat(|p - r| - s), pos + neg of ProcessFrame before the blur (reference
 * AnalyzerUnit.cpp:341-351).  Every value is an exact integer: two launches on `stream` (the records' initial state, then
 * jobs x 16 KiB tiles, each block summing its tile on chip and issuing one atomic of each kind: u32 add / min / max and
 * u64 add, all of which commute), no host synchronisation, no allocation. */
typedef struct abub_stat_job { uint64_t cur, ref, model; } abub_stat_job;
   /* byte offsets: cur/ref into `frames`, model into `mu` and `sigma6`; no alignment rule;
      ref == UINT64_MAX: no reference frame; model == UINT64_MAX or mu == NULL: no model */
typedef struct abub_stat_result {   /* 64 bytes */
    uint32_t status;                /* 0, ABUB_STAT_E_RANGE */
    uint32_t min, max, n_zero, n_sat;          /* pixels == 0, == 255 */
    uint32_t n_out, n_moved, flags;            /* flags: bit0 model columns valid, bit1 ref columns valid */
    uint64_t sum, sumsq, sum_out, sum_moved;
} abub_stat_result;
#define ABUB_STAT_E_RANGE 1 /* a stream the job names runs past its buffer: nothing of the job is read; every other field 0 */
#define ABUB_STAT_F_MODEL 1u /* n_out / sum_out are valid: the job names a model */
#define ABUB_STAT_F_REF 2u   /* n_moved / sum_moved are valid: the job names a model and a reference frame */
/* Every pointer is a device pointer; jobs and results are 8-byte aligned; frame_bytes in [1, 2^32 - 2].  mu == NULL: no
 * job has a model (sigma6 is then not looked at); else sigma6 must not be NULL.  A column whose inputs are absent is 0 and
 * its flag bit is clear; a reference frame without a model is checked for its range and not read.  results[njobs] is
 * written in full by every call with njobs > 0, whatever it held before.  Streams whose addresses are congruent mod 16
 * are read 16 bytes at a time, mod 4 four at a time, else byte by byte: as exact, and slower.  Null pointers, njobs < 0,
 * frame_bytes out of range or a misaligned jobs / results: ABUB_E_INVALID before anything touches the device.
 * njobs == 0: ABUB_OK, nothing is touched. */
int abub_frame_stats_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, const uint8_t *sigma6,
                         size_t model_bytes, const abub_stat_job *jobs, int njobs, size_t frame_bytes,
                         abub_stat_result *results, void *stream);

/* ---- per-pixel activity planes of resident frames (abub_stats.hip) ---------------------------------------------------
 * The per-pixel view of a survey (abub3hs --survey --survey-planes; DESIGN section 3, "Surveying a run per pixel"): the
 * terms abub_frame_stats_dev sums over the pixels of a frame, summed over the frames of ONE camera instead.  With p the
 * pixel of the frame at frames + jobs[j].cur, m and s the bytes of `mu` and `sigma6` at that pixel and r the pixel of the
 * frame at frames + jobs[j].ref, every job ADDS to the six u32 planes at planes + k * plane_stride, k = 0 .. 5:
 *   0 n_zero: p == 0        2 n_out:   sat(|p - m| - s) > 0      4 n_moved:   sat(|p - r| - s) > 0
 *   1 n_sat:  p == 255      3 sum_out: sat(|p - m| - s)          5 sum_moved: sat(|p - r| - s)
 * The call adds and never overwrites: the caller clears the planes once, and a run is a sequence of calls.  mu == NULL
 * (then sigma6 == NULL too): planes 2 to 5 are not touched.  ref == UINT64_MAX: the job adds nothing to planes 4 and 5.
 * A job whose cur, or whose ref where it is not UINT64_MAX, runs past frames_bytes adds nothing at all and makes *status
 * ABUB_ACT_E_RANGE; the other jobs are added.  *status is cleared by the call, on `stream`.  A thread owns 8 consecutive
 * pixels for the whole call, so every plane word has one owner and nothing is atomic: the planes are bit-identical
 * whatever the order of the jobs and however they are split over calls.  A memset and at most two launches on `stream`,
 * no host synchronisation, no allocation.  A caller adds at most 16,777,215 jobs into one set of planes (255 * 2^24 <
 * 2^32).  Only planes[k * plane_stride + i], k < 6, i < frame_bytes, and *status are written. */
typedef struct abub_act_job { uint64_t cur, ref; } abub_act_job;   /* byte offsets into frames; ref == UINT64_MAX: none */
#define ABUB_ACT_E_RANGE 1
/* Every pointer is a device pointer; mu and sigma6 are ONE camera's planes, or both NULL; jobs is 8-byte aligned, status
 * 4-byte aligned, planes 16-byte aligned and plane_stride a multiple of 4 and >= frame_bytes; frame_bytes in
 * [1, 2^32 - 2].  Streams whose addresses are multiples of 8 after the same head bytes are read 8 bytes at a time, of 4
 * four at a time, else byte by byte: as exact, and slower.  Anything else: ABUB_E_INVALID before anything touches the
 * device.  njobs == 0: ABUB_OK, nothing is touched. */
int abub_pixel_activity_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, const uint8_t *sigma6,
                            const abub_act_job *jobs, int njobs, size_t frame_bytes, uint32_t *planes, size_t plane_stride,
                            uint32_t *status, void *stream);

/* ---- per-frame shift search of resident frames (abub_stats.hip) -------------------------------------------------------
 * Did the camera or the chamber image move against the trained model (abub3hs --survey --survey-shift; definition, report
 * and measurements: DESIGN section 3, "Surveying a run for movement")?  For a batch of resident W x H frames, with p the
 * frame at frames + jobs[j].cur, m the plane of `mu` at mu + jobs[j].model, a radius R and the interior
 * I = { (x, y) : R <= x < W - R, R <= y < H - R }, for every -R <= dx, dy <= R
 *   sad[j * (2R+1)^2 + (dy + R) * (2R+1) + (dx + R)] = sum over (x, y) in I of | p(x + dx, y + dy) - m(x, y) |     (u64).
 * Every displacement sums over the same |I| pixels; there is no border rule and no sigma term.  Every value is an exact
 * integer, bit-identical to the host definition (host/survey.cpp frameShiftHost) whatever the order of the jobs or the
 * blocks: two launches on `stream` (status and a cleared surface, then jobs x tiles of 256 x 64 interior pixels, each
 * block reading its tile and halo once into LDS, summing v_sad_u8 of byte-shifted dwords on chip and issuing one u64 atomic
 * add per displacement, which commute), no host synchronisation, no allocation, no workgroup waiting for another.  Which
 * displacement is the best one is the host's to say (abub::shiftBest, one tie rule for both routes). */
typedef struct abub_shift_job { uint64_t cur, model; } abub_shift_job;   /* byte offsets into frames / mu */
#define ABUB_SHIFT_E_RANGE 1
/* Every pointer is a device pointer; jobs and sad are 8-byte aligned, status 4-byte aligned; R in [1, 8]; W and H in
 * [2R+1, 65535].  No alignment rule on the offsets: a stream is read through aligned dwords wherever it lies.  status[j] (0
 * or ABUB_SHIFT_E_RANGE) and all (2R+1)^2 values of sad[j] are written in full by every call with njobs > 0, whatever they
 * held before, and nothing else is written.  A job whose frame runs past frames_bytes or whose model plane runs past
 * model_bytes gets ABUB_SHIFT_E_RANGE and a zero surface; nothing of it is read.  Null pointers, njobs < 0, R, W or H out
 * of range or a misaligned jobs / status / sad: ABUB_E_INVALID before anything touches the device.  njobs == 0: ABUB_OK,
 * nothing is touched. */
int abub_frame_shift_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, size_t model_bytes,
                         const abub_shift_job *jobs, int njobs, int W, int H, int R,
                         uint32_t *status /*[njobs]*/, uint64_t *sad /*[njobs * (2R+1)^2]*/, void *stream);

/* ---- per-cell shift field of resident frames (abub_stats.hip) ---------------------------------------------------------
 * Did a part of the image move, or the whole of it other than rigidly (abub3hs --survey --survey-field; definition, files
 * and measurements: DESIGN section 3, "Surveying a run for local movement")?  The sums of abub_frame_shift_dev kept apart
 * per cell of ABUB_FIELD_CELL x ABUB_FIELD_CELL interior pixels.  Only whole cells exist, centred in the interior:
 * abub_frame_cells_grid gives ncx = floor((W - 2R) / 128), ncy = floor((H - 2R) / 128), x0 = R + floor(((W - 2R) - 128 ncx) / 2)
 * and y0 likewise; a frame with W or H < 128 + 2R has ncx * ncy = 0 and no field.  It is the one copy of the rule: the
 * launcher, the host definition and the tests call it.  It touches no device; ABUB_E_INVALID for a null pointer, R outside
 * [1, 8] or a negative side.  For cell (cx, cy) of job j and every -R <= dx, dy <= R
 *   sad[((j * ncy + cy) * ncx + cx) * (2R+1)^2 + (dy + R) * (2R+1) + (dx + R)] = sum of | p(x + dx, y + dy) - m(x, y) |  (u32)
 * over x0 + 128 cx <= x < x0 + 128 (cx + 1), y0 + 128 cy <= y < y0 + 128 (cy + 1): 16384 pixels, at most 16384 * 255 < 2^32.
 * Every value is an exact integer, bit-identical to the host definition (host/survey.cpp fieldCellsHost) whatever the
 * order of the jobs or the blocks: one launch on `stream` of cells x jobs blocks, each reading its cell and halo once into
 * LDS, summing as abub_frame_shift_dev does and writing the words of its cell's surface with plain stores.  Every output
 * word has one owning workgroup: no atomics, no clearing launch, no host synchronisation, no allocation, no workgroup
 * waiting for another.  What a surface means (best displacement, rated or not) is the host's to say (abub::fieldCell). */
#define ABUB_FIELD_CELL 128
int abub_frame_cells_grid(int W, int H, int R, int *ncx, int *ncy, int *x0, int *y0);
/* Every pointer is a device pointer; jobs is 8-byte aligned, status and sad 4-byte aligned; R in [1, 8]; W and H in
 * [128 + 2R, 65535].  No alignment rule on the offsets.  status[j] (0 or ABUB_SHIFT_E_RANGE) and all ncx * ncy * (2R+1)^2
 * values of sad[j] are written in full by every call with njobs > 0, whatever they held before, and nothing else is
 * written.  A job whose frame runs past frames_bytes or whose model plane runs past model_bytes gets ABUB_SHIFT_E_RANGE and
 * a zero surface; nothing of it is read.  Null pointers, njobs < 0, R, W or H out of range (a frame without a whole cell
 * included) or a misaligned jobs / status / sad: ABUB_E_INVALID before anything touches the device.  njobs == 0: ABUB_OK,
 * nothing is touched. */
int abub_frame_shift_cells_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, size_t model_bytes,
                               const abub_shift_job *jobs, int njobs, int W, int H, int R,
                               uint32_t *status /*[njobs]*/, uint32_t *sad /*[njobs * ncy * ncx * (2R+1)^2]*/, void *stream);

/* ---- per-cell light record of resident frames (abub_stats.hip) -------------------------------------------------------
 * Did the light change, and where (abub3hs --survey --survey-light; definition, files and measurements: DESIGN section 3,
 * "Surveying a run for lighting changes")?  Per cell of ABUB_FIELD_CELL x ABUB_FIELD_CELL pixels on the grid the caller
 * gives (ncx x ncy whole cells, the first at (x0, y0); the survey passes abub_frame_cells_grid's) six u32 sums over the
 * cell's pixels p of the frame at frames + jobs[j].cur and m of the plane at mu + jobs[j].model:
 *   rec[((j * ncy + cy) * ncx + cx) * 6 + 0 .. 5] = sum p, sum p^2, sum p m, sum |p - m|, pixels with p == 0, with p == 255
 * over x0 + 128 cx <= x < x0 + 128 (cx + 1), y0 + 128 cy <= y < y0 + 128 (cy + 1): 16384 pixels, at most
 * 16384 * 255^2 = 1065369600 < 2^31.  Every value is an exact integer, bit-identical to the host definition
 * (host/survey.cpp lightCellsHost) whatever the order of the jobs or the blocks: one launch on `stream` of cells x jobs
 * blocks of four waves, each reading its cell once into registers and writing its six words with plain stores.  Every
 * output word has one owning workgroup: no atomics, no clearing launch, no scratch buffer, no host synchronisation, no
 * allocation, no workgroup waiting for another.  What a record means is the host's to say (abub::lightCell).
 * Every pointer is a device pointer; jobs is 8-byte aligned, status and rec 4-byte aligned; W and H in [128, 65535];
 * ncx, ncy >= 1, x0, y0 >= 0, x0 + 128 ncx <= W, y0 + 128 ncy <= H.  No alignment rule on the offsets or on x0.  status[j]
 * (0 or ABUB_SHIFT_E_RANGE) and all ncx * ncy * 6 values of rec[j] are written in full by every call with njobs > 0,
 * whatever they held before, and nothing else is written.  A job whose frame runs past frames_bytes or whose model plane
 * runs past model_bytes gets ABUB_SHIFT_E_RANGE and a zero record; nothing of it is read.  Null pointers, njobs < 0, W, H
 * or the grid out of range or a misaligned jobs / status / rec: ABUB_E_INVALID before anything touches the device.
 * njobs == 0: ABUB_OK, nothing is touched.  njobs may exceed 65535. */
#define ABUB_LIGHT_WORDS 6
int abub_frame_light_cells_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, size_t model_bytes,
                               const abub_shift_job *jobs, int njobs, int W, int H, int x0, int y0, int ncx, int ncy,
                               uint32_t *status /*[njobs]*/, uint32_t *rec /*[njobs * ncy * ncx * 6]*/, void *stream);

/* ---- per-cell edge agreement of resident frames (abub_stats.hip) ------------------------------------------------------
 * Do the frame's edges still agree with the model's, and where (abub3hs --survey --survey-focus; definition, files and
 * measurements: DESIGN section 3, "Surveying a run for lost focus")?  Per cell of ABUB_FIELD_CELL x ABUB_FIELD_CELL pixels
 * on the grid the caller gives (ncx x ncy whole cells, the first at (x0, y0); the survey passes abub_frame_cells_grid's)
 * five i32 over the cell's pixels, with gx = p(x + 1, y) - p(x - 1, y) and gy = p(x, y + 1) - p(x, y - 1) of the frame at
 * frames + jobs[j].cur and hx, hy the same differences of the plane at mu + jobs[j].model:
 *   rec[((j * ncy + cy) * ncx + cx) * 5 + 0 .. 4] = sum gx^2, sum gy^2, sum gx hx, sum gy hy, pixels with p == 0 or p == 255
 * over x0 + 128 cx <= x < x0 + 128 (cx + 1), y0 + 128 cy <= y < y0 + 128 (cy + 1): 16384 pixels, a magnitude of at most
 * 16384 * 255^2 = 1065369600 < 2^31.  Every value is an exact integer, bit-identical to the host definition
 * (host/survey.cpp focusCellsHost) whatever the order of the jobs or the blocks: one launch on `stream` of cells x jobs
 * blocks of four waves, each reading its cell and the ring of one pixel around it once into two LDS tiles (the frame's and
 * mu's, 34320 bytes) and writing its five words with plain stores.  Every output word has one owning workgroup: no atomics,
 * no clearing launch, no scratch buffer, no host synchronisation, no allocation, no workgroup waiting for another.  What a
 * record means is the host's to say (abub::focusCell).
 * Every pointer is a device pointer; jobs is 8-byte aligned, status and rec 4-byte aligned; W and H in [130, 65535];
 * ncx, ncy >= 1, x0, y0 >= 1, x0 + 128 ncx + 1 <= W, y0 + 128 ncy + 1 <= H.  No alignment rule on the offsets or on x0.
 * status[j] (0 or ABUB_SHIFT_E_RANGE) and all ncx * ncy * 5 values of rec[j] are written in full by every call with
 * njobs > 0, whatever they held before, and nothing else is written.  A job whose frame runs past frames_bytes or whose
 * model plane runs past model_bytes gets ABUB_SHIFT_E_RANGE and a zero record; nothing of it is read.  Null pointers,
 * njobs < 0, W, H or the grid out of range or a misaligned jobs / status / rec: ABUB_E_INVALID before anything touches the
 * device.  njobs == 0: ABUB_OK, nothing is touched.  njobs may exceed 65535. */
#define ABUB_FOCUS_WORDS 5
int abub_frame_focus_cells_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, size_t model_bytes,
                               const abub_shift_job *jobs, int njobs, int W, int H, int x0, int y0, int ncx, int ncy,
                               uint32_t *status /*[njobs]*/, int32_t *rec /*[njobs * ncy * ncx * 5]*/, void *stream);

/* ---- per-cell frame-pair noise record of resident frames (abub_stats.hip) ----------------------------------------------
 * Is the noise of the run still the noise the model was trained on, and where (abub3hs --survey --survey-noise;
 * definition, files and measurements: DESIGN section 3, "Surveying a run for noise changes")?  Per cell of
 * ABUB_FIELD_CELL x ABUB_FIELD_CELL pixels on the grid the caller gives (ncx x ncy whole cells, the first at (x0, y0); the
 * survey passes abub_frame_cells_grid's) six i32 over the cell's pixels p of the frame at frames + jobs[j].cur, r of the
 * reference frame at frames + jobs[j].ref and s of the plane at sigma6 + jobs[j].model (min(6 sigma, 255)), with d = p - r:
 *   rec[((j * ncy + cy) * ncx + cx) * 6 + 0 .. 5] = n_over, the pixels with |d| > s; n_clip, the pixels where p or r is 0 or
 *   255; s1_in = sum d and s2_in = sum d^2 over the pixels with |d| <= s; sad = sum |d| and s2_all = sum d^2 over all
 * 16384 pixels: a magnitude of at most 16384 * 255^2 = 1065369600 < 2^31.  mu is not read.  Every value is an exact
 * integer, bit-identical to the host definition (host/survey.cpp noiseCellsHost) whatever the order of the jobs or the
 * blocks: one launch on `stream` of cells x jobs blocks of four waves, each reading its cell once into registers and
 * writing its six words with plain stores.  Every output word has one owning workgroup: no atomics, no clearing launch, no
 * scratch buffer, no host synchronisation, no allocation, no workgroup waiting for another.  What a record means is the
 * host's to say (abub::noiseCell).
 * Every pointer is a device pointer; jobs is 8-byte aligned, status and rec 4-byte aligned; W and H in [128, 65535];
 * ncx, ncy >= 1, x0, y0 >= 0, x0 + 128 ncx <= W, y0 + 128 ncy <= H.  No alignment rule on the three offsets or on x0.
 * status[j] (0 or ABUB_SHIFT_E_RANGE) and all ncx * ncy * 6 values of rec[j] are written in full by every call with
 * njobs > 0, whatever they held before, and nothing else is written.  A job of which the frame or the reference frame runs
 * past frames_bytes or the sigma6 plane past model_bytes (an offset of UINT64_MAX included) gets ABUB_SHIFT_E_RANGE and a
 * zero record; nothing of it is read.  ref == cur is legal: a record with d = 0.  Null pointers, njobs < 0, W, H or the
 * grid out of range or a misaligned jobs / status / rec: ABUB_E_INVALID before anything touches the device.  njobs == 0:
 * ABUB_OK, nothing is touched.  njobs may exceed 65535. */
#define ABUB_NOISE_WORDS 6
int abub_frame_noise_cells_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *sigma6, size_t model_bytes,
                               const abub_stat_job *jobs, int njobs, int W, int H, int x0, int y0, int ncx, int ncy,
                               uint32_t *status /*[njobs]*/, int32_t *rec /*[njobs * ncy * ncx * 6]*/, void *stream);

/* ---- per-line sums of whole resident frames (abub_stats.hip) -----------------------------------------------------------
 * Is a frame torn, repeated or banded: does a run of its rows equal the rows of the frame two before it, do single rows or
 * columns stand above the model (abub3hs --survey --survey-lines; definition, rule, files and measurements: DESIGN section
 * 3, "Surveying a run for torn, repeated and banded frames")?  Per image row y of the W x H frame p at frames + jobs[j].cur,
 * against the plane m at mu + jobs[j].model and the reference frame r at frames + jobs[j].ref, five u32 over the row's W
 * pixels:
 *   rows[(j * H + y) * 5 + 0 .. 4] = sum p; sum |p - m|; n_clip, the pixels with p == 0 or p == 255; sum |p - r|; n_same,
 *   the pixels with p == r
 * and per image column x the first three of them over the column's H pixels: cols[(j * W + x) * 3 + 0 .. 2].  A job with
 * ref == UINT64_MAX has no reference frame: its words 3 and 4 are 0.  ref == cur is legal: n_same = W and word 3 = 0.  Every
 * value is an exact integer of at most 65535 * 255 = 16711425, bit-identical to the host definition (host/survey.cpp
 * linesHost) whatever the order of the jobs or the blocks: one launch on `stream`, a block of four waves per job, which
 * reads the job's three streams once (16-byte loads where the address allows, aligned dwords elsewhere) and owns every
 * output word of the job: plain stores, no atomics on memory, no clearing launch, no scratch buffer, no host
 * synchronisation, no allocation, no workgroup waiting for another.  What the sums mean is the host's to say
 * (abub::lineRate, abub::linesFrame).
 * Every pointer is a device pointer; jobs is 8-byte aligned, status, rows and cols 4-byte aligned; W and H in [1, 65535].
 * No alignment rule on the three offsets.  status[j] (0 or ABUB_SHIFT_E_RANGE) and all H * 5 values of rows[j] and W * 3 of
 * cols[j] are written in full by every call with njobs > 0, whatever they held before, and nothing else is written.  A job
 * of which the frame or a reference frame that is there runs past frames_bytes or the plane past model_bytes gets
 * ABUB_SHIFT_E_RANGE and zero records; nothing of it is read.  Null pointers, njobs < 0, W or H out of range or a
 * misaligned jobs / status / rows / cols: ABUB_E_INVALID before anything touches the device.  njobs == 0: ABUB_OK, nothing
 * is touched.  njobs may exceed 65535. */
#define ABUB_LINES_ROW_WORDS 5
#define ABUB_LINES_COL_WORDS 3
int abub_frame_lines_dev(const uint8_t *frames, size_t frames_bytes, const uint8_t *mu, size_t model_bytes,
                         const abub_stat_job *jobs, int njobs, int W, int H,
                         uint32_t *status /*[njobs]*/, uint32_t *rows /*[njobs * H * 5]*/,
                         uint32_t *cols /*[njobs * W * 3]*/, void *stream);

/* ---- the two DebugPeek planes of a batch of resident frames (abub_peek.hip) ------------------------------------------
 * What L3Localizer::CalculateInitialBubbleParams builds on the analyzer's thread for its debug write-out (reference
 * L3Localizer.cpp:252-257, 397, 448; DESIGN section 3, "The peek planes"), for a batch of items.  Per item two W x H u8
 * planes are written into `out`:
 *   the thresholded image  out[thr_out + i] = diff[diff + i] > thr ? 255 : 0 -- the mask contoursOfCurrentImage hands back
 *                          from foregroundKept(thr, -1), written as _3_OtsuThresholded;
 *   the presentation frame the W * H bytes at frames + frame, then cv::rectangle (host/cvlite.cpp) of every rectangle
 *                          rects[rect_begin .. rect_begin + rect_count): 255 on the rows y and y + h - 1 and the columns x
 *                          and x + w - 1, each clipped to the frame; w <= 0 or h <= 0 draws nothing; rectangles may
 *                          overlap and may lie partly or wholly outside the frame; written as _4_BubbleDetected.
 * The planes lie at multiples of 16, where abub_png_encode_dev takes them through src[].  A copy launch, then (nrects > 0)
 * a draw launch on `stream`; no flags, no atomics, no host synchronisation, no allocation.  A source whose address is a
 * multiple of 16 is read 16 bytes at a time; any other is as exact, and slower. */
typedef struct abub_peek_item {
    uint64_t diff;      /* byte offset of D from `diff`, any alignment */
    uint64_t frame;     /* byte offset of the trigger frame from `frames`, any alignment */
    uint64_t thr_out;   /* byte offset of the thresholded plane from `out`, a multiple of 16 */
    uint64_t pres_out;  /* byte offset of the presentation plane from `out`, a multiple of 16 */
    int32_t thr;        /* any value: below 0 the whole plane is 255, from 255 on it is 0 */
    int32_t rect_begin; /* the item's rectangles in `rects` */
    int32_t rect_count;
    int32_t reserved;
} abub_peek_item;
typedef struct abub_peek_rect { int32_t x, y, w, h; } abub_peek_rect;
#define ABUB_PEEK_E_SRC 1  /* diff + W*H > diff_bytes or frame + W*H > frames_bytes */
#define ABUB_PEEK_E_DST 2  /* a plane not at a multiple of 16, running past out_bytes, or the two planes overlapping */
#define ABUB_PEEK_E_RECT 3 /* rect_begin < 0, rect_count < 0 or rect_begin + rect_count > nrects */
/* Every pointer is a device pointer; items is 8-byte, rects and status 4-byte, out 16-byte aligned; `out` overlaps neither
 * `diff` nor `frames`, which may be the same buffer; planes of different items do not overlap.  status[nitems] is written
 * for every item: 0, or the first ABUB_PEEK_E_* that applies in the order above -- then nothing of the item is read and
 * not one byte of its planes is written.  Nothing is written outside the two planes of an item.  rects may be null when
 * nrects == 0.  Null pointers, negative counts, W or H outside [1, 65535] or a misaligned buffer: ABUB_E_INVALID before
 * anything touches the device.  nitems == 0: ABUB_OK, nothing is touched. */
int abub_peek_planes_dev(const uint8_t *diff, size_t diff_bytes, const uint8_t *frames, size_t frames_bytes,
                         const abub_peek_item *items, int nitems, const abub_peek_rect *rects, int nrects, int W, int H,
                         uint8_t *out, size_t out_bytes, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif
