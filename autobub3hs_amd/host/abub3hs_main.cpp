// abub3hs_main.cpp -- command-line driver with the reference's argument surface and run flow
// (AutoBubStart3.cpp:127-405): -d data_dir -r run_ID -o out_dir [-z] [-c mask_dir] [-m] [-D series] [-e event]
// [--debug code]; per-series image naming / frameOffset / camera count (:220-245); header, event list, training
// (-7 rows if it fails), event loop with ordered output, -5 if the run cannot be read.  boost::program_options and
// OpenMP are replaced by a small parser and a std::thread pool (ABUB_THREADS, default min(16, cores)).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include <sched.h>

#include "AlgorithmTraining/Trainer.hpp"
#include "BubbleLocalizer/L3Localizer.hpp"
#include "PICOFormatWriter/PICOFormatWriterV4.hpp"
#include "ParseFolder/RawParser.hpp"
#include "ParseFolder/ZipParser.hpp"
#include "driver.hpp"
#include "runbatch.hpp"
#include "zipwrite.hpp"

static std::string usage()
{
    return "Usage: abub3hs [-hzme] [-D data_series] [-c cam_mask_dir] [--debug code] -d data_dir -r run_ID -o out_dir\n"
           "       abub3hs [-hzm] [-D data_series] [-c cam_mask_dir] -d data_dir --runs ID[,ID...] | --run-list FILE -o out_dir\n"
           "       abub3hs [-z] [-D data_series] -d data_dir -r run_ID --repack out_data_dir [--repack-gpu] [--archive]\n"
           "       abub3hs [-z] [-D data_series] -d data_dir -r run_ID --unpack out_data_dir [--unpack-gpu] [--archive]\n"
           "       abub3hs [-z] [-D data_series] -d data_dir -r run_ID --verify-repack other_data_dir [--verify-gpu] [--archive]\n"
           "       abub3hs [-z] [-D data_series] -d data_dir -r run_ID --survey FILE [--survey-gpu] [--survey-planes DIR]\n"
           "               [--survey-shift FILE [--survey-shift-radius R]]\n"
           "               [--survey-field DIR [--survey-field-radius R]]\n"
           "               [--survey-light DIR [--survey-field-radius R]]\n"
           "               [--survey-focus DIR [--survey-field-radius R]]\n"
           "               [--survey-noise DIR [--survey-field-radius R]]\n"
           "               [--survey-lines DIR]\n"
           "Run the AutoBub3hs bubble finding algorithm on a PICO run (MI355X hot path)\n\n"
           "Required arguments:\n"
           "  -d, --data_dir = Dir\t\tpath to the directory in which the run folder/file is stored\n"
           "  -r, --run_id = Str\t\trun ID, formatted as YYYYMMDD_*\n"
           "  or --runs = ID[,ID...]\truns of one data series processed by this one process (a campaign), each written to\n"
           "\t\t\t\tits own abub3hs_<run>.txt; the next run trains on the GPU while the current one is detected\n"
           "  or --run-list = File\t\tthe same with one run ID per line (blank lines and # comments ignored); may be\n"
           "\t\t\t\tcombined with --runs, the order is kept; not with -r, no run twice\n"
           "  -o, --out_dir = Dir\t\tdirectory to write the output file to\n\n"
           "Optional arguments:\n"
           "  -h, --help\t\t\tgive this help message\n"
           "  -z, --zip\t\t\tindicate the run is stored as a zip file; otherwise assumed to be in a directory\n"
           "  -c, --cam_mask_dir = Dir\tdirectory containing the camera mask images\n"
           "  -m, --mask_check\t\tuse camera masks in default directory. Not needed if directory specified\n"
           "  -D, --data_series = Str\tname of the data series, e.g. 40l-19, 30l-16, etc.\n"
           "  -e, --event = Int\t\tspecify a single event to process. Mostly just useful for debugging and testing\n"
           "  --debug = Int\t\t\t3 digit int; eg: 101: first digit = localizer debug; second digit = multithread off; third digit = analyzer debug\n"
           "MI355X options:\n"
           "  --gpus = Int\t\t\tGPUs to spread the event batches over (one worker thread per GPU; default 1)\n"
           "  --gpu-shard = r/N\t\tprocess only the events whose index in the sorted event list is r modulo N;\n"
           "\t\t\t\twrites abub3hs_<run>.part<r>of<N>.txt (N > 1)\n"
           "  --merge = N\t\t\tassemble abub3hs_<run>.txt in --out_dir from the N part files of a sharded run (of every\n"
           "\t\t\t\trun of --runs / --run-list)\n"
           "  --per-event\t\t\tone analyzer at a time like the reference's loop (also chosen by -e and --debug);\n"
           "\t\t\t\tdefault: whole batches of events decoded into pinned memory and analysed together;\n"
           "\t\t\t\t-e, --debug and --per-event take a single run\n"
           "  --peek = Dir\t\t\twith the batched path: write the six DebugPeek images of every accepted (event, camera) to\n"
           "\t\t\t\tDir/<run_ID>/ev<event>_cam<c>_*.png, formed and encoded on the GPU (ABUB_PEEK_GPU=0: on host\n"
           "\t\t\t\tthreads, the same files); not with -e, --debug, --per-event, --merge, --repack, --unpack, --verify-repack\n"
           "  --repack = Dir\t\twrite the run to Dir/<run_ID>/ with every frame in the packed format the GPU decodes\n"
           "\t\t\t\twithout an inflate (24x the PNG decode; file names stay; files that do not decode are copied); no GPU, no analysis,\n"
           "\t\t\t\tno -o; not with -e, --merge, --runs / --run-list, --gpu-shard, and not into the\n"
           "\t\t\t\tdata_dir it reads.  Analyse it with -d Dir\n"
           "  --repack-gpu\t\t\twith --repack: decode and pack the frames on GPU 0 (the same files, byte for byte; what the\n"
           "\t\t\t\tGPU decoders do not take is packed by host threads); an error when there is no HIP device\n"
           "  --unpack = Dir\t\tthe way back from --repack: write the run (packed, PNG, BMP or mixed) to Dir/<run_ID>/ with every\n"
           "\t\t\t\tframe as an ordinary 8-bit grey PNG under its own name (Sub filter, one Huffman-only deflate block:\n"
           "\t\t\t\tthe same pixels give the same bytes); everything else as --repack; not together with --repack\n"
           "  --unpack-gpu\t\t\twith --unpack: decode the frames and write the PNG files on GPU 0 (the same files, byte for byte);\n"
           "\t\t\t\tan error when there is no HIP device\n"
           "  --verify-repack = Dir\t\tcompare the run with its copy Dir/<run_ID>/ (what --repack Dir wrote), frame by frame: every\n"
           "\t\t\t\tframe decoded on both sides and compared pixel for pixel, missing and extra frames and events,\n"
           "\t\t\t\tthe event file; one line per finding (the first 20) and a summary; exit status 0 = verified,\n"
           "\t\t\t\t1 = something failed; no analysis, no -o; not with -e, --merge, --runs / --run-list, --gpu-shard;\n"
           "\t\t\t\twith --repack Dir or --unpack Dir (the same Dir): repack or unpack first, then verify\n"
           "  --verify-gpu\t\t\twith --verify-repack: decode both sides and compare them on GPU 0 (the same findings and\n"
           "\t\t\t\tcounters); an error when there is no HIP device\n"
           "  --archive\t\t\twith --repack, --unpack or --verify-repack: the copy is the one file Dir/<run_ID>.zip instead of\n"
           "\t\t\t\tthe tree Dir/<run_ID>/: a zip archive of stored entries with the same files, every byte fixed by\n"
           "\t\t\t\trule (the data of each entry at a multiple of 16; zip64 where it is needed), written as .zip.part\n"
           "\t\t\t\tand renamed when it is complete; with the -gpu flags the entries are formed on the GPU and a batch\n"
           "\t\t\t\tis one write.  Analyse it with -z -d Dir\n"
           "  --survey = File\t\tmeasure every frame of the run without analysing any and write the report to File: per camera\n"
           "\t\t\t\tthe model (pixels with sigma = 0, with 6 sigma >= 255), per frame its state (ok, undecodable,\n"
           "\t\t\t\tmissing, other_size), grey-level range, sum, sum of squares, black and saturated pixels, and count\n"
           "\t\t\t\tand sum of what the model and the frame two before leave above 6 sigma; a `run` line with the\n"
           "\t\t\t\ttotals; exit status 0, or 1 if a frame is not ok; no -o; not with -e, --debug, --per-event, --merge,\n"
           "\t\t\t\t--repack, --unpack, --verify-repack, --peek, --runs / --run-list, --gpu-shard\n"
           "  --survey-gpu\t\t\twith --survey: decode the frames and measure them on GPU 0 (the same report, byte for byte); an\n"
           "\t\t\t\terror when there is no HIP device\n"
           "  --survey-planes = Dir\t\twith --survey: also sum the frames per pixel and camera and write Dir/<run_ID>/: per camera\n"
           "\t\t\t\tcam<c>_activity.npy, six u32 planes [6, H, W] (frames in which the pixel was 0, was 255, count and\n"
           "\t\t\t\tsum of what the model leaves above 6 sigma, count and sum of what the frame two before leaves),\n"
           "\t\t\t\tcam<c>_moved.png (the share of frames in which the pixel moved, 255 = all) and activity.txt (the\n"
           "\t\t\t\tdenominators, dead / stuck / ever-moved pixel counts and the 16 hottest pixels); the same bytes\n"
           "\t\t\t\twith --survey-gpu; the report does not change\n"
           "  --survey-shift = File\t\twith --survey: also search every ok frame of a camera with a model for its displacement\n"
           "\t\t\t\tagainst the model's mean image (the sum of absolute differences over the interior at every integer\n"
           "\t\t\t\tdx, dy within the radius) and write File: per frame the best dx, dy, whether it lies on the edge of\n"
           "\t\t\t\tthe search, the sums at (0, 0) and at the best, and the gain; per camera and for the run how many\n"
           "\t\t\t\tframes moved and from which event on; the same bytes with --survey-gpu; the report and the planes\n"
           "\t\t\t\tdo not change\n"
           "  --survey-shift-radius = R\twith --survey-shift: the radius of the search in pixels, 1 to 8 (4); the frames must be at\n"
           "\t\t\t\tleast 2 R + 1 wide and high\n"
           "  --survey-field = Dir\t\twith --survey: also search the same frames per cell of 128 x 128 pixels (whole cells, centred\n"
           "\t\t\t\tin the interior) and write into Dir/<run_ID>/ cam<c>_field.npy (i32 [frames, cells down, cells\n"
           "\t\t\t\tacross, 5]: per cell the best dx, dy, the sums at (0, 0), at the best and the largest) and\n"
           "\t\t\t\tfield.txt: per frame how many cells are rated (the best sum at most half the largest) and how\n"
           "\t\t\t\tmany of those moved, their most frequent displacement and its range, and the frame's kind (blind,\n"
           "\t\t\t\tstill, rigid, warped, local); per camera and for the run the counts of each kind and per cell the\n"
           "\t\t\t\tframes in which it moved; the same bytes with --survey-gpu; the report, the planes and the shift\n"
           "\t\t\t\tfile do not change\n"
           "  --survey-field-radius = R\twith --survey-field: the radius of the search in pixels, 1 to 8 (4); the frames must be at\n"
           "\t\t\t\tleast 128 + 2 R wide and high; with --survey-light, --survey-focus or --survey-noise, with or without\n"
           "\t\t\t\t--survey-field: the radius that places the cells\n"
           "  --survey-light = Dir\t\twith --survey: also sum the same frames per cell of the field's grid (the cells of\n"
           "\t\t\t\t--survey-field at --survey-field-radius, 4 unless given, whether or not the field is written) and\n"
           "\t\t\t\twrite into Dir/<run_ID>/ cam<c>_light.npy (i32 [frames, cells down, cells across, 6]: per cell the\n"
           "\t\t\t\tsums of p, p^2, p mu and |p - mu|, the black and the saturated pixels), cam<c>_light_model.npy\n"
           "\t\t\t\t(i32 [cells down, cells across, 3]: the sums of mu, mu^2 and min(6 sigma, 255)) and light.txt: per\n"
           "\t\t\t\tframe how many cells are rated, clipped and changed (the mean level moved by more than the mean\n"
           "\t\t\t\t6 sigma), up or down, the level in thousandths of a grey level, the range of the cells' ratios in\n"
           "\t\t\t\tthousandths, the pooled gain and offset in thousandths, and the frame's kind (blind, steady, level,\n"
           "\t\t\t\tuneven); per camera and for the run the counts of each kind and per cell the frames in which it\n"
           "\t\t\t\tchanged; the same bytes with --survey-gpu; the report, the planes, the shift file and the field do\n"
           "\t\t\t\tnot change\n"
           "  --survey-focus = Dir\t\twith --survey: also compare the edges of the same frames with the model's per cell of the\n"
           "\t\t\t\tfield's grid (at --survey-field-radius, 4 unless given, whether or not the field or the light is\n"
           "\t\t\t\twritten) and write into Dir/<run_ID>/ cam<c>_focus.npy (i32 [frames, cells down, cells across, 5]:\n"
           "\t\t\t\tper cell the sums of gx^2, gy^2, gx hx and gy hy, g and h the central differences of the frame and\n"
           "\t\t\t\tof mu, and the pixels at 0 or 255), cam<c>_focus_model.npy (i64 [cells down, cells across, 3]: the\n"
           "\t\t\t\tsums of hx^2 and hy^2 and the square of six standard deviations of the agreement under the trained\n"
           "\t\t\t\tnoise) and focus.txt: per frame how many cells are rated, clipped and changed (the agreement moved\n"
           "\t\t\t\tby more than that), softer or harder, the pooled agreement and edge energy in thousandths of the\n"
           "\t\t\t\tmodel's, the range of the cells' agreement, and the frame's kind (blind, steady, soft, uneven); per\n"
           "\t\t\t\tcamera and for the run the counts of each kind and per cell the frames in which it changed; the\n"
           "\t\t\t\tsame bytes with --survey-gpu; the report, the planes, the shift file, the field and the light do\n"
           "\t\t\t\tnot change\n"
           "  --survey-noise = Dir\t\twith --survey: also compare every such frame whose reference frame (the frame two before in\n"
           "\t\t\t\tits stack) is another ok frame with that frame, per cell of the field's grid (at\n"
           "\t\t\t\t--survey-field-radius, 4 unless given, whatever else is written), and write into Dir/<run_ID>/\n"
           "\t\t\t\tcam<c>_noise.npy (i32 [frames, cells down, cells across, 6]: per cell, with d the difference of\n"
           "\t\t\t\tthe two frames, the pixels with |d| over min(6 sigma, 255), the pixels at 0 or 255 in either\n"
           "\t\t\t\tframe, the sums of d and d^2 over the other pixels, the sums of |d| and d^2 over all),\n"
           "\t\t\t\tcam<c>_noise_model.npy (i64 [cells down, cells across, 5]: the baseline measured from the run's\n"
           "\t\t\t\town second frames, its pixels and frames, the sum of min(6 sigma, 255)^2 and the pixels with sigma\n"
           "\t\t\t\t0) and noise.txt: per frame how many cells are rated, clipped, busy (more than a quarter of the\n"
           "\t\t\t\tpixels over), noisy (the variance over 1.5 times the baseline's) and quiet (under 0.667 times),\n"
           "\t\t\t\tthe pooled variance ratio in thousandths and its range, the ratio of all pixels, and the frame's\n"
           "\t\t\t\tkind (blind, busy, steady, noisy, quiet, uneven); per camera and for the run the counts of each\n"
           "\t\t\t\tkind and per cell the frames in which it changed; the same bytes with --survey-gpu; nothing else\n"
           "\t\t\t\tchanges\n"
           "  --survey-lines = Dir\t\twith --survey: also sum every such frame along its image rows and columns (any size, no grid)\n"
           "\t\t\t\tagainst mu and against the frame two before in its stack where that is another ok frame, and\n"
           "\t\t\t\twrite into Dir/<run_ID>/ cam<c>_lines_rows.npy (i32 [frames, H, 5]: per row the sums of p and of\n"
           "\t\t\t\t|p - mu|, the pixels at 0 or 255, the sum of |p - r| and the pixels with p == r),\n"
           "\t\t\t\tcam<c>_lines_cols.npy (i32 [frames, W, 3]: the first three per column),\n"
           "\t\t\t\tcam<c>_lines_model_rows.npy and cam<c>_lines_model_cols.npy (i32 [H, 3] and [W, 3]: the sums of mu\n"
           "\t\t\t\tand of min(6 sigma, 255), the pixels with sigma 0) and lines.txt: per frame the rated, off and\n"
           "\t\t\t\tstale rows (stale: equal to the reference frame's row pixel for pixel), the first and last stale\n"
           "\t\t\t\trow, the rated and off columns, the first and last off row and column, the level in thousandths\n"
           "\t\t\t\tand the frame's kind (blind, repeated, torn, banded, striped, steady); per camera and for the run\n"
           "\t\t\t\tthe counts of each kind and per row and column the frames in which it was off or stale; the\n"
           "\t\t\t\tsame bytes with --survey-gpu; nothing else changes\n"
           "Environment: ABUB_TRAIN_ON_GPU=0 trains the runs of a campaign with the host Trainer\n"
           "             ABUB_REPACK_BATCH=n (a test knob) lowers the frames per batch of --repack-gpu and --unpack-gpu to n; the files\n"
           "             are the same\n"
           "             ABUB_GPU_BMP=1 decodes BMP frames on the GPU in every device reading route (the batched run, training on the\n"
           "             GPU, --repack-gpu, --unpack-gpu, --verify-gpu); ABUB_GPU_BMP=0, the default, leaves them to host threads;\n"
           "             results are the same\n"
           "             ABUB_GPU_PNG_TYPES=1 also decodes 16-bit, RGB(A), grey+alpha and 1/2/4-bit PNG frames on the GPU in those\n"
           "             routes (interlaced files stay with the host); unset or 0, the default, leaves them to host threads; results\n"
           "             are the same\n"
           "             ABUB_GPU_PNG_ADAM7=1 also decodes Adam7-interlaced PNG frames on the GPU in those routes: 8-bit grey and palette\n"
           "             files, with ABUB_GPU_PNG_TYPES=1 the other types too; unset or 0, the default, leaves them to host threads,\n"
           "             which read interlaced files of every type; results are the same\n";
}

// cores this process may use: the affinity mask (taskset, cpuset) AND the cgroup's CPU quota (cpu.max: a container may see
// 256 cores and be allowed 16 of them) -- the reference's omp_get_max_threads() (AutoBubStart3.cpp:338) sees only the former
static int usableCores()
{
    int n = (int)std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof set, &set) == 0 && CPU_COUNT(&set) > 0)
        n = CPU_COUNT(&set);
    std::ifstream q("/sys/fs/cgroup/cpu.max"); // cgroup v2: "<quota> <period>" or "max <period>"
    std::string quota;
    long long period = 0;
    if (q >> quota >> period && quota != "max" && period > 0) {
        const long long c = (atoll(quota.c_str()) + period - 1) / period;
        if (c >= 1 && c < n)
            n = (int)c;
    }
    return n;
}

// --merge N: the reference writes ONE file in event order (the `ordered` clause, AutoBubStart3.cpp:380-383).  Shard r of N
// holds the events r, r + N, .. of the sorted event list, one block of rows per event, in order: the header comes from
// part 0, then the blocks are dealt back round-robin.  A block = consecutive rows with the same event number (column 2).
static int mergeParts(const std::string &out_dir, const std::string &run_number, int N)
{
    std::vector<std::vector<std::string>> blocks((size_t)N);
    std::string header;
    for (int r = 0; r < N; ++r) {
        const std::string path = out_dir + "abub3hs_" + run_number + ".part" + std::to_string(r) + "of" + std::to_string(N) + ".txt";
        std::ifstream in(path);
        if (!in) {
            std::cerr << "--merge: cannot read " << path << std::endl;
            return -1;
        }
        std::string line, head, lastEv;
        for (int k = 0; k < 6 && std::getline(in, line); ++k) // 3 header lines, "8", two blank lines (writeHeader)
            head += line + "\n";
        if (r == 0)
            header = head;
        else if (head != header) {
            std::cerr << "--merge: " << path << " has a different header" << std::endl;
            return -1;
        }
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            std::string run, ev;
            ls >> run >> ev;
            if (blocks[r].empty() || ev != lastEv)
                blocks[r].push_back(std::string());
            blocks[r].back() += line + "\n";
            lastEv = ev;
        }
    }
    std::ofstream out(out_dir + "abub3hs_" + run_number + ".txt");
    if (!out) {
        std::cerr << "--merge: cannot write into " << out_dir << std::endl;
        return -1;
    }
    out << header;
    size_t longest = 0;
    for (auto &b : blocks)
        longest = std::max(longest, b.size());
    for (size_t j = 0; j < longest; ++j)
        for (int r = 0; r < N; ++r)
            if (j < blocks[r].size())
                out << blocks[r][j];
    return out.good() ? 0 : -1;
}

// how the different experiments stored their images (AutoBubStart3.cpp:216-245); per run: for 40l-19 the camera count and
// the frame offset depend on the run ID
static void runConstants(const std::string &data_series, const std::string &run_number, std::string &imageFormat,
                         std::string &imageFolder, int &frameOffset, int &numCams)
{
    if (data_series == "01l-21" || data_series == "2l-16") {
        imageFormat = "cam%dimage %u.bmp";
        imageFolder = "/";
        frameOffset = 0;
        numCams = 2;
    } else if (data_series == "40l-19") {
        imageFormat = "cam%d_image%u.png";
        imageFolder = "/Images/";
        frameOffset = 30;
        numCams = run_number >= "20200713_7" ? 4 : 2;
        if (run_number < "20200501_1")
            frameOffset = 20;
    } else {
        imageFormat = "cam%d_image%u.png";
        imageFolder = "/Images/";
        frameOffset = 30;
        numCams = 4;
    }
    if (const char *nc = getenv("ABUB_NUM_CAMS")) // synthetic runs with fewer cameras
        numCams = atoi(nc);
}

// a run of the command line: its event directory and the series' constants
static abub::RunSpec runSpec(const std::string &dataLoc, const std::string &data_series, const std::string &run, bool zipped)
{
    abub::RunSpec sp;
    sp.runId = run;
    sp.eventDir = dataLoc + "/" + run + "/";
    sp.zipped = zipped;
    runConstants(data_series, run, sp.imageFormat, sp.imageFolder, sp.frameOffset, sp.numCams);
    return sp;
}

// the batched path's options from the command line and the environment
static abub::BatchedRunOptions batchedOptions(int ngpus, int hostThreads, int decodeThreads, int shardRank, int shardWorld,
                                              const std::string &mask_dir)
{
    abub::BatchedRunOptions bo;
    bo.ngpus = ngpus;
    if (const char *d = getenv("ABUB_DEVICE"))
        bo.firstDevice = atoi(d);
    bo.hostThreads = hostThreads;
    bo.decodeThreads = decodeThreads;
    if (const char *t = getenv("ABUB_DECODE_THREADS"))
        bo.decodeThreads = std::max(1, atoi(t));
    if (const char *b = getenv("ABUB_BATCH_MB"))
        bo.batchBytes = (size_t)std::max(1, atoi(b)) << 20;
    bo.shardRank = shardRank;
    bo.shardWorld = shardWorld;
    bo.maskDir = mask_dir;
    return bo;
}

// --run-list FILE: one run ID per line; blank lines and '#' comments are ignored
static bool readRunList(const std::string &path, std::vector<std::string> &runs)
{
    std::ifstream in(path);
    if (!in)
        return false;
    std::string line;
    while (std::getline(in, line)) {
        const size_t hash = line.find('#');
        if (hash != std::string::npos)
            line.erase(hash);
        const size_t a = line.find_first_not_of(" \t\r"), b = line.find_last_not_of(" \t\r");
        if (a != std::string::npos)
            runs.push_back(line.substr(a, b - a + 1));
    }
    return true;
}

int main(int argc, char **argv)
{
    std::string dataLoc, run_number, out_dir, mask_dir, data_series, repackDir, verifyDir;
    bool haveUnpack = false, unpackGpu = false; // (--unpack takes --repack's route with another frame format)
    bool haveShard = false, haveRepack = false, repackGpu = false, haveVerify = false, verifyGpu = false;
    int event_user = -1, debug_mode = 0, ngpus = 1, shardRank = 0, shardWorld = 1, mergeN = 0;
    bool zipped = false, mask_check = false, help = argc == 1, perEvent = false;
    bool haveRun = false, haveList = false; // -r; --runs / --run-list
    std::vector<std::string> runs;          // of --runs / --run-list, in command-line order
    std::string peekDir;                    // --peek DIR: the DebugPeek images of the batched path (BatchedRunOptions::peekDir)
    bool havePeek = false;
    bool archive = false; // --archive: the copy of --repack / --unpack / --verify-repack is Dir/<run_ID>.zip
    std::string surveyFile; // --survey FILE: the run measured frame by frame (abub::SurveyRun), nothing else
    bool haveSurvey = false, surveyGpu = false;
    std::string surveyPlanesDir; // --survey-planes DIR: the survey's per-pixel planes go to DIR/<run_ID>/
    bool haveSurveyPlanes = false;
    std::string surveyShiftFile; // --survey-shift FILE: the survey's shift search, its answers go to FILE
    bool haveSurveyShift = false, haveShiftRadius = false;
    int surveyShiftRadius = 4;
    std::string surveyFieldDir; // --survey-field DIR: the survey's per-cell shift field goes to DIR/<run_ID>/
    bool haveSurveyField = false, haveFieldRadius = false;
    int surveyFieldRadius = 4;
    std::string surveyLightDir; // --survey-light DIR: the survey's per-cell light records go to DIR/<run_ID>/
    bool haveSurveyLight = false;
    std::string surveyFocusDir; // --survey-focus DIR: the survey's per-cell focus records go to DIR/<run_ID>/
    bool haveSurveyFocus = false;
    std::string surveyNoiseDir; // --survey-noise DIR: the survey's per-cell noise records go to DIR/<run_ID>/
    bool haveSurveyNoise = false;
    std::string surveyLinesDir; // --survey-lines DIR: the survey's per-line records go to DIR/<run_ID>/
    bool haveSurveyLines = false;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i], v;
        auto value = [&](std::string &dst) {
            size_t eq = a.find('=');
            if (a.rfind("--", 0) == 0 && eq != std::string::npos)
                dst = a.substr(eq + 1);
            else if (i + 1 < argc)
                dst = argv[++i];
        };
        auto is = [&](const char *s, const char *l) { return a == s || a == l || a.rfind(std::string(l) + "=", 0) == 0; };
        if (is("-h", "--help"))
            help = true;
        else if (is("-z", "--zip"))
            zipped = true;
        else if (is("-m", "--mask_check"))
            mask_check = true;
        else if (is("-d", "--data_dir"))
            value(dataLoc);
        else if (is("-r", "--run_num") || a == "--run_id") {
            value(run_number);
            haveRun = true;
        } else if (a == "--runs" || a.rfind("--runs=", 0) == 0) {
            value(v);
            haveList = true;
            for (size_t at = 0; at <= v.size();) {
                const size_t comma = std::min(v.find(',', at), v.size());
                if (comma > at)
                    runs.push_back(v.substr(at, comma - at));
                at = comma + 1;
            }
        } else if (a == "--run-list" || a.rfind("--run-list=", 0) == 0) {
            value(v);
            haveList = true;
            if (!readRunList(v, runs)) {
                std::cerr << "--run-list: cannot read " << v << std::endl;
                return -1;
            }
        }
        else if (is("-o", "--out_dir"))
            value(out_dir);
        else if (is("-c", "--cam_mask_dir"))
            value(mask_dir);
        else if (is("-D", "--data_series"))
            value(data_series);
        else if (is("-e", "--event")) {
            value(v);
            event_user = atoi(v.c_str());
        } else if (a.rfind("--debug", 0) == 0) {
            value(v);
            debug_mode = atoi(v.c_str());
        } else if (a.rfind("--gpus", 0) == 0) {
            value(v);
            ngpus = std::max(1, atoi(v.c_str()));
        } else if (a.rfind("--gpu-shard", 0) == 0) {
            value(v);
            haveShard = true;
            if (sscanf(v.c_str(), "%d/%d", &shardRank, &shardWorld) != 2 || shardWorld < 1 || shardRank < 0 || shardRank >= shardWorld) {
                std::cerr << "--gpu-shard expects r/N with 0 <= r < N" << std::endl;
                return -1;
            }
        } else if (a.rfind("--merge", 0) == 0) {
            value(v);
            mergeN = atoi(v.c_str());
            if (mergeN < 1) {
                std::cerr << "--merge expects the number of shards" << std::endl;
                return -1;
            }
        } else if (a == "--repack" || a.rfind("--repack=", 0) == 0) {
            if (haveUnpack) {
                std::cerr << "--unpack cannot be combined with --repack" << std::endl;
                return -1;
            }
            value(repackDir);
            haveRepack = true;
        } else if (a == "--repack-gpu") {
            repackGpu = true;
        } else if (a == "--unpack" || a.rfind("--unpack=", 0) == 0) {
            if (haveRepack && !haveUnpack) {
                std::cerr << "--unpack cannot be combined with --repack" << std::endl;
                return -1;
            }
            value(repackDir);
            haveRepack = haveUnpack = true;
        } else if (a == "--unpack-gpu") {
            unpackGpu = true;
        } else if (a == "--verify-repack" || a.rfind("--verify-repack=", 0) == 0) {
            value(verifyDir);
            haveVerify = true;
        } else if (a == "--verify-gpu") {
            verifyGpu = true;
        } else if (a == "--archive") {
            archive = true;
        } else if (a == "--survey" || a.rfind("--survey=", 0) == 0) {
            value(surveyFile);
            haveSurvey = true;
        } else if (a == "--survey-gpu") {
            surveyGpu = true;
        } else if (a == "--survey-planes" || a.rfind("--survey-planes=", 0) == 0) {
            value(surveyPlanesDir);
            haveSurveyPlanes = true;
        } else if (a == "--survey-shift-radius" || a.rfind("--survey-shift-radius=", 0) == 0) {
            v.clear();
            value(v);
            haveShiftRadius = true;
            char *end = nullptr;
            const long radius = strtol(v.c_str(), &end, 10);
            if (v.empty() || *end || radius < 1 || radius > 8) {
                std::cerr << "--survey-shift-radius expects a radius from 1 to 8" << std::endl;
                return -1;
            }
            surveyShiftRadius = (int)radius;
        } else if (a == "--survey-shift" || a.rfind("--survey-shift=", 0) == 0) {
            value(surveyShiftFile);
            haveSurveyShift = true;
        } else if (a == "--survey-field-radius" || a.rfind("--survey-field-radius=", 0) == 0) {
            v.clear();
            value(v);
            haveFieldRadius = true;
            char *end = nullptr;
            const long radius = strtol(v.c_str(), &end, 10);
            if (v.empty() || *end || radius < 1 || radius > 8) {
                std::cerr << "--survey-field-radius expects a radius from 1 to 8" << std::endl;
                return -1;
            }
            surveyFieldRadius = (int)radius;
        } else if (a == "--survey-field" || a.rfind("--survey-field=", 0) == 0) {
            value(surveyFieldDir);
            haveSurveyField = true;
        } else if (a == "--survey-light" || a.rfind("--survey-light=", 0) == 0) {
            value(surveyLightDir);
            haveSurveyLight = true;
        } else if (a == "--survey-focus" || a.rfind("--survey-focus=", 0) == 0) {
            value(surveyFocusDir);
            haveSurveyFocus = true;
        } else if (a == "--survey-noise" || a.rfind("--survey-noise=", 0) == 0) {
            value(surveyNoiseDir);
            haveSurveyNoise = true;
        } else if (a == "--survey-lines" || a.rfind("--survey-lines=", 0) == 0) {
            value(surveyLinesDir);
            haveSurveyLines = true;
        } else if (a == "--per-event") {
            perEvent = true;
        } else if (a == "--peek" || a.rfind("--peek=", 0) == 0) {
            value(peekDir);
            havePeek = true;
        } else {
            std::cerr << "unrecognised option '" << a << "'" << std::endl;
            return -1;
        }
    }
    if (help) {
        std::cout << usage() << std::endl;
        return 1;
    }
    if (havePeek) {
        // --peek belongs to the batched path: the per-event loop has its own write-out (--debug), the other modes detect nothing
        const char *bad = event_user >= 0 ? "-e/--event" : debug_mode ? "--debug" : perEvent ? "--per-event" : mergeN > 0 ? "--merge"
                          : haveUnpack ? "--unpack" : haveRepack ? "--repack" : haveVerify ? "--verify-repack" : nullptr;
        if (bad) {
            std::cerr << "--peek cannot be combined with " << bad << std::endl;
            return -1;
        }
        if (peekDir.empty()) {
            std::cerr << "--peek needs the directory to write to" << std::endl;
            return -1;
        }
    }
    // the --survey-* flags, in the order they are checked: the flag it is valid only together with, and of those that take
    // a place to write to that place and what it is
    const struct {
        const char *flag;
        bool have;
        const char *with;
        bool haveWith;
        const std::string *value;
        const char *noun;
    } surveyFlags[] = {
        {"--survey-gpu", surveyGpu, "--survey", haveSurvey, nullptr, nullptr},
        {"--survey-planes", haveSurveyPlanes, "--survey", haveSurvey, &surveyPlanesDir, "directory"},
        {"--survey-shift", haveSurveyShift, "--survey", haveSurvey, &surveyShiftFile, "file"},
        {"--survey-shift-radius", haveShiftRadius, "--survey-shift", haveSurveyShift, nullptr, nullptr},
        {"--survey-field", haveSurveyField, "--survey", haveSurvey, &surveyFieldDir, "directory"},
        {"--survey-light", haveSurveyLight, "--survey", haveSurvey, &surveyLightDir, "directory"},
        {"--survey-focus", haveSurveyFocus, "--survey", haveSurvey, &surveyFocusDir, "directory"},
        {"--survey-noise", haveSurveyNoise, "--survey", haveSurvey, &surveyNoiseDir, "directory"},
        {"--survey-lines", haveSurveyLines, "--survey", haveSurvey, &surveyLinesDir, "directory"},
        // (the light's, the focus' and the noise's cells are the field's)
        {"--survey-field-radius", haveFieldRadius, "--survey-field", haveSurveyField || haveSurveyLight || haveSurveyFocus || haveSurveyNoise,
         nullptr, nullptr},
    };
    for (const auto &f : surveyFlags)
        if (f.have && !f.haveWith) {
            std::cerr << f.flag << " is valid only together with " << f.with << std::endl;
            return -1;
        }
    if (haveSurvey) {
        const char *bad = haveUnpack ? "--unpack" : haveRepack ? "--repack" : haveVerify ? "--verify-repack" : mergeN > 0 ? "--merge"
                          : debug_mode ? "--debug" : perEvent ? "--per-event" : event_user >= 0 ? "-e/--event" : havePeek ? "--peek"
                          : haveList ? "--runs / --run-list" : haveShard ? "--gpu-shard" : nullptr;
        if (bad) {
            std::cerr << "--survey cannot be combined with " << bad << std::endl;
            return -1;
        }
        if (dataLoc.empty() || run_number.empty() || surveyFile.empty()) {
            std::cerr << "--survey needs --data_dir, --run_id and the file to write the report to" << std::endl;
            return -1;
        }
        for (const auto &f : surveyFlags)
            if (f.have && f.value && f.value->empty()) {
                std::cerr << f.flag << " needs the " << f.noun << " to write to" << std::endl;
                return -1;
            }
    }
    if (unpackGpu && !haveUnpack) {
        std::cerr << "--unpack-gpu is valid only together with --unpack" << std::endl;
        return -1;
    }
    if (repackGpu && haveUnpack) {
        std::cerr << "--repack-gpu is valid only together with --repack" << std::endl;
        return -1;
    }
    const char *const rewrite = haveUnpack ? "unpack" : "repack"; // the flag and the word in the messages
    repackGpu = repackGpu || unpackGpu;
    if (repackGpu && !haveRepack) {
        std::cerr << "--repack-gpu is valid only together with --repack" << std::endl;
        return -1;
    }
    if (verifyGpu && !haveVerify) {
        std::cerr << "--verify-gpu is valid only together with --verify-repack" << std::endl;
        return -1;
    }
    if (archive && !haveRepack && !haveVerify) {
        std::cerr << "--archive is valid only together with --repack, --unpack or --verify-repack" << std::endl;
        return -1;
    }
    if (haveRepack || haveVerify) {
        // ---- --repack: the run rewritten with packed frames (abub::RepackRun); --verify-repack: the run compared with such
        // a copy (abub::VerifyRun); with both, one after the other; nothing else happens ---------------------------------------
        const char *bad = mergeN > 0 ? "--merge" : haveList ? "--runs / --run-list" : haveShard ? "--gpu-shard"
                          : event_user >= 0 ? "-e/--event" : nullptr;
        if (bad) {
            std::cerr << (haveUnpack ? "--unpack" : haveRepack ? "--repack" : "--verify-repack") << " cannot be combined with " << bad << std::endl;
            return -1;
        }
        if (haveRepack && (dataLoc.empty() || run_number.empty() || repackDir.empty())) {
            std::cerr << "--" << rewrite << " needs --data_dir, --run_id and the directory to write to" << std::endl;
            return -1;
        }
        if (haveVerify && (dataLoc.empty() || run_number.empty() || verifyDir.empty())) {
            std::cerr << "--verify-repack needs --data_dir, --run_id and the directory of the copy" << std::endl;
            return -1;
        }
        if (haveRepack && haveVerify && repackDir != verifyDir) {
            std::cerr << "--" << rewrite << " and --verify-repack together must name the same directory" << std::endl;
            return -1;
        }
    }
    // the run of a RunSpec through its parser; null (and the -5 message) when it cannot be read
    auto openRun = [&](const abub::RunSpec &sp) {
        std::unique_ptr<Parser> parser;
        try {
            if (sp.zipped)
                parser.reset(new ZipParser(sp.eventDir, sp.imageFolder, sp.imageFormat));
            else
                parser.reset(new RawParser(sp.eventDir, sp.imageFolder, sp.imageFormat));
        } catch (...) {
            std::cerr << "Failed to read the images from run " << run_number << "." << std::endl;
        }
        return parser;
    };
    auto poolThreads = [&]() {
        int threads = std::min(usableCores(), 128);
        if (const char *t = getenv("ABUB_THREADS"))
            threads = std::max(1, atoi(t));
        return threads;
    };
    if (haveRepack) {
        const abub::RunSpec sp = runSpec(dataLoc, data_series, run_number, zipped);
        const std::unique_ptr<Parser> parser = openRun(sp);
        if (!parser)
            return -5;
        const int threads = poolThreads();
        abub::RepackStats rs;
        int rc = 1;
        try {
            const std::string srcDir = zipped ? std::string() : sp.eventDir;
            const std::string srcFile = zipped ? std::string() : sp.eventDir + run_number + ".txt";
            const std::string dst = repackDir + "/" + run_number;
            const abub::ArchiveTarget target{archive, zipped ? abub::zipPathOf(sp.eventDir) : std::string()};
            rc = repackGpu ? (haveUnpack ? abub::UnpackRunDevice : abub::RepackRunDevice)(parser.get(), srcDir, srcFile, dst,
                                                                                          sp.imageFolder, sp.numCams, threads, 0, &rs, target)
                           : (haveUnpack ? abub::UnpackRun : abub::RepackRun)(parser.get(), srcDir, srcFile, dst, sp.imageFolder,
                                                                              sp.numCams, threads, &rs, target);
        } catch (std::exception &e) {
            std::cerr << rewrite << " failed: " << e.what() << std::endl;
            return -6;
        } catch (...) { // (the parsers throw their status codes)
            std::cerr << "Failed to read the images from run " << run_number << "." << std::endl;
            return -5;
        }
        printf("%s: %d events, %lld frames %s (%lld -> %lld bytes), %lld copied as they are, %lld not written, %.2f s, "
               "%.1f frames/s\n",
               rewrite, rs.events, rs.packed, haveUnpack ? "written as PNG" : "packed", rs.bytesIn, rs.bytesOut, rs.copied, rs.failed, rs.total_s,
               rs.total_s > 0 ? (rs.packed + rs.copied) / rs.total_s : 0.0);
        if (archive)
            printf("%s: archive %s/%s.zip: %lld bytes, %lld entries\n", rewrite, repackDir.c_str(), run_number.c_str(), rs.archiveBytes,
                   rs.archiveEntries);
        if (repackGpu) {
            if (rs.device < 0)
                printf("%s-gpu: 0 frames encoded on the GPU, %lld took the host route (no frame of a width the GPU decoders "
                       "take)\n",
                       rewrite, rs.framesHostRoute);
            else
                printf("%s-gpu: %lld frames encoded on GPU %d (%lld decoded by the PNG kernel, %lld by the packed kernel, "
                       "%lld by a host thread), %lld took the host route, %d batches; read %.2f s, upload + decode %.2f s, "
                       "encode %.2f s, copy back %.2f s, write %.2f s\n",
                       rewrite, rs.framesGpuEncoded, rs.device, rs.framesGpuPngDecoded, rs.framesGpuUnpacked, rs.framesHostDecoded,
                       rs.framesHostRoute, rs.batches, rs.read_s, rs.decode_s, rs.encode_s, rs.copy_s, rs.write_s);
            if (rs.framesGpuBmpDecoded)
                printf("%s-gpu: %lld frames decoded by the BMP kernel\n", rewrite, rs.framesGpuBmpDecoded);
            if (rs.framesGpuUnzipped)
                printf("%s-gpu: %lld archive entries inflated on the GPU\n", rewrite, rs.framesGpuUnzipped);
            if (archive && rs.device >= 0)
                printf("%s-gpu: archive entries formed on GPU %d: pack %.2f s\n", rewrite, rs.device, rs.pack_s);
        }
        if (!haveVerify || rc != 0)
            return rc;
    }
    if (haveVerify) {
        const abub::RunSpec sp = runSpec(dataLoc, data_series, run_number, zipped);
        const abub::RunSpec other = runSpec(verifyDir, data_series, run_number, archive); // (--archive: Dir/<run_ID>.zip)
        const std::unique_ptr<Parser> parser = openRun(sp), copy = parser ? openRun(other) : nullptr;
        if (!parser || !copy)
            return -5;
        abub::VerifyStats vs;
        std::vector<abub::VerifyFinding> findings;
        int rc = 1;
        try {
            const std::string srcFile = zipped ? std::string() : sp.eventDir + run_number + ".txt";
            const std::string otherFile = other.eventDir + run_number + ".txt";
            rc = verifyGpu ? abub::VerifyRunDevice(parser.get(), copy.get(), srcFile, otherFile, sp.numCams, poolThreads(), 0, &vs, &findings, archive)
                           : abub::VerifyRun(parser.get(), copy.get(), srcFile, otherFile, sp.numCams, poolThreads(), &vs, &findings, archive);
        } catch (std::exception &e) {
            std::cerr << "verify failed: " << e.what() << std::endl;
            return -6;
        } catch (...) { // (the parsers throw their status codes)
            std::cerr << "Failed to read the images from run " << run_number << "." << std::endl;
            return -5;
        }
        const size_t shown = std::min<size_t>(findings.size(), 20);
        for (size_t i = 0; i < shown; ++i)
            printf("verify: %s\n", findings[i].text().c_str());
        if (findings.size() > shown)
            printf("... and %zu more\n", findings.size() - shown);
        printf("verify: %d events, %lld frames: %lld same, %lld same but not packed, %lld copied, %lld differ, %lld missing, "
               "%lld undecodable, %lld extra; event file %s; %.2f s, %.1f frames/s\n",
               vs.events, vs.frames, vs.same, vs.sameNotPacked, vs.copied, vs.differ, vs.missing, vs.undecodable, vs.extra,
               vs.eventFileName(), vs.total_s, vs.total_s > 0 ? vs.frames / vs.total_s : 0.0);
        if (verifyGpu) {
            if (vs.device < 0)
                printf("verify-gpu: 0 frames compared on the GPU, %lld took the host route (no frame of a width the GPU decoders "
                       "take)\n",
                       vs.framesHostRoute);
            else
                printf("verify-gpu: %lld frames compared on GPU %d (the source's decoded: %lld by the PNG kernel, %lld by the packed "
                       "kernel, %lld by a host thread; the copy's: %lld, %lld, %lld), %lld took the host route, %d batches; read %.2f s, "
                       "upload + decode %.2f s, compare %.2f s\n",
                       vs.framesKernel, vs.device, vs.srcGpuPngDecoded, vs.srcGpuUnpacked, vs.srcHostDecoded, vs.otherGpuPngDecoded,
                       vs.otherGpuUnpacked, vs.otherHostDecoded, vs.framesHostRoute, vs.batches, vs.read_s, vs.decode_s, vs.compare_s);
            if (vs.srcGpuBmpDecoded || vs.otherGpuBmpDecoded)
                printf("verify-gpu: %lld frames decoded by the BMP kernel (the source's %lld, the copy's %lld)\n",
                       vs.srcGpuBmpDecoded + vs.otherGpuBmpDecoded, vs.srcGpuBmpDecoded, vs.otherGpuBmpDecoded);
        }
        return rc;
    }
    if (haveSurvey) {
        // ---- --survey: the run listed and trained as for detect (abub::PrepareRun), then measured; nothing else happens --------
        const abub::RunSpec sp = runSpec(dataLoc, data_series, run_number, zipped);
        abub::BatchedRunOptions po;
        po.trainOnGpu = 0; // (a single run trains through the host Trainer, as the reference does)
        abub::SurveyStats ss;
        abub::SurveyRequest rq;
        rq.reportPath = surveyFile;
        rq.srcRunDir = zipped ? std::string() : sp.eventDir;
        const auto under = [&](bool have, const std::string &dir) { return have ? dir + "/" + run_number : std::string(); };
        rq.planesDir = under(haveSurveyPlanes, surveyPlanesDir);
        rq.shiftPath = surveyShiftFile;
        rq.shiftRadius = surveyShiftRadius;
        rq.fieldDir = under(haveSurveyField, surveyFieldDir);
        rq.cellRadius = surveyFieldRadius;
        rq.lightDir = under(haveSurveyLight, surveyLightDir);
        rq.focusDir = under(haveSurveyFocus, surveyFocusDir);
        rq.noiseDir = under(haveSurveyNoise, surveyNoiseDir);
        rq.linesDir = under(haveSurveyLines, surveyLinesDir);
        int rc = 1;
        try {
            abub::PreparedRun prep = abub::PrepareRun(sp, po, 0, nullptr, false);
            if (prep.rc == -5)
                return -5;
            if (prep.rc)
                printf("survey: a camera did not train: the report has no model columns for it\n");
            // (--survey-gpu is GPU 0, so "no such HIP device" for a negative one cannot arise here; SurveyRun refuses a missing GPU 0)
            rc = abub::SurveyRun(prep.parser.get(), prep.trainers, sp.numCams, sp.imageFormat, rq, poolThreads(), surveyGpu ? 0 : -1, &ss);
        } catch (std::exception &e) {
            std::cerr << "survey failed: " << e.what() << std::endl;
            return -6;
        } catch (...) { // (the parsers throw their status codes)
            std::cerr << "Failed to read the images from run " << run_number << "." << std::endl;
            return -5;
        }
        printf("survey: %d events, %lld frames %dx%d: %lld ok, %lld undecodable, %lld missing, %lld of another size; %d cameras with a "
               "model; %.2f s, %.1f frames/s\n",
               ss.events, ss.frames, ss.W, ss.H, ss.ok, ss.undecodable, ss.missing, ss.otherSize, ss.modelCams, ss.total_s,
               ss.total_s > 0 ? ss.frames / ss.total_s : 0.0);
        if (surveyGpu) {
            if (ss.device < 0)
                printf("survey-gpu: 0 frames measured on the GPU, %lld took the host route (no frame of a width the GPU decoders "
                       "take)\n",
                       ss.framesHostRoute);
            else
                printf("survey-gpu: %lld frames measured on GPU %d (decoded: %lld by the PNG kernel, %lld by the packed kernel, %lld by "
                       "the BMP kernel, %lld by a host thread; %lld read again, %lld archive entries inflated on the GPU), %lld took the "
                       "host route, %d batches; read %.2f s, upload + decode %.2f s, measure %.2f s\n",
                       ss.framesKernel, ss.device, ss.gpuPngDecoded, ss.gpuUnpacked, ss.gpuBmpDecoded, ss.hostDecoded, ss.reread,
                       ss.gpuUnzipped, ss.framesHostRoute, ss.batches, ss.read_s, ss.decode_s, ss.stats_s);
        }
        if (haveSurveyPlanes)
            printf("survey-planes: %s: %lld rows added on the GPU, %lld on the host; activity launches %.3f s, copy back %.3f s, files "
                   "%.3f s\n",
                   rq.planesDir.c_str(), ss.planeRowsKernel, ss.planeRowsHost, ss.activity_s, ss.planes_copy_s, ss.planes_write_s);
        const struct {
            bool have;
            const char *name, *to, *verb;
            int radius;
        } products[abub::SurveyProducts] = {{haveSurveyShift, "shift", rq.shiftPath.c_str(), "searched", rq.shiftRadius},
                                            {haveSurveyField, "field", rq.fieldDir.c_str(), "searched", rq.cellRadius},
                                            {haveSurveyLight, "light", rq.lightDir.c_str(), "summed", rq.cellRadius},
                                            {haveSurveyFocus, "focus", rq.focusDir.c_str(), "summed", rq.cellRadius},
                                            {haveSurveyNoise, "noise", rq.noiseDir.c_str(), "summed", rq.cellRadius},
                                            {haveSurveyLines, "lines", rq.linesDir.c_str(), "summed", 0}};
        for (int p = 0; p < abub::SurveyProducts; ++p)
            if (products[p].have)
                printf("survey-%s: %s: radius %d, %lld frames %s on the GPU in %d launches, %lld on the host; %s leg %.3f s, host "
                       "threads %.3f s\n",
                       products[p].name, products[p].to, products[p].radius, ss.product[p].framesKernel, products[p].verb,
                       ss.product[p].launches, ss.product[p].framesHost, products[p].name, ss.product[p].leg_s, ss.product[p].host_s);
        return rc;
    }
    if (haveList) {
        if (haveRun) {
            std::cerr << "-r cannot be combined with --runs or --run-list" << std::endl;
            return -1;
        }
        if (runs.empty()) {
            std::cerr << "--runs / --run-list: no run ID given" << std::endl;
            return -1;
        }
        for (size_t i = 0; i < runs.size(); ++i)
            for (size_t j = 0; j < i; ++j)
                if (runs[i] == runs[j]) {
                    std::cerr << "duplicate run ID '" << runs[i] << "' in --runs / --run-list (both would write abub3hs_"
                              << runs[i] << ".txt)" << std::endl;
                    return -1;
                }
        if (runs.size() > 1) {
            const char *pe = getenv("ABUB_PER_EVENT"), *bad = event_user >= 0 ? "-e/--event" : debug_mode ? "--debug" : perEvent ? "--per-event"
                              : pe && atoi(pe) != 0 ? "ABUB_PER_EVENT" : nullptr;
            if (bad) {
                std::cerr << bad << " cannot be used with more than one run" << std::endl;
                return -1;
            }
        }
        if (mergeN > 0) {
            if (out_dir.empty()) {
                std::cerr << "--merge needs --out_dir" << std::endl;
                return -1;
            }
            if (out_dir[out_dir.length() - 1] != '/')
                out_dir += "/";
            int rc = 0;
            for (const std::string &r : runs) {
                const int m = mergeParts(out_dir, r, mergeN);
                if (m && !rc)
                    rc = m;
            }
            return rc;
        }
        // one run with -e / --debug / --per-event: the single-run path
        const char *pe = getenv("ABUB_PER_EVENT");
        if (runs.size() == 1 && (event_user >= 0 || debug_mode || perEvent || (pe && atoi(pe) != 0))) {
            run_number = runs[0];
            runs.clear();
        }
    }
    if (mergeN > 0) {
        if (run_number.empty() || out_dir.empty()) {
            std::cerr << "--merge needs --run_id and --out_dir" << std::endl;
            return -1;
        }
        if (out_dir[out_dir.length() - 1] != '/')
            out_dir += "/";
        return mergeParts(out_dir, run_number, mergeN);
    }
    if (dataLoc.empty() || (run_number.empty() && runs.empty()) || out_dir.empty()) {
        std::cerr << "Insufficient required arguments; use \"autobub3hs -h\" to view required arguments" << std::endl;
        return -1;
    }
    printf("This is AutoBub v3, the automatic unified bubble finder code for all chambers\n");

    std::string this_path = argv[0];
    std::string abub_dir = this_path.substr(0, this_path.find_last_of("/") + 1);
    if (mask_check && mask_dir == "")
        mask_dir = abub_dir + "cam_masks/" + data_series;
    else if (!mask_check && mask_dir == "")
        std::cout << "Not performing mask check on this run." << std::endl;

    if (out_dir[out_dir.length() - 1] != '/')
        out_dir += "/";
    std::string eventDir = dataLoc + "/" + run_number + "/";

    std::string imageFormat, imageFolder;
    int frameOffset, numCams;
    runConstants(data_series, run_number, imageFormat, imageFolder, frameOffset, numCams);

    // Threads.  The reference runs omp_get_max_threads() events at once (AutoBubStart3.cpp:338-342): the per-event loop and
    // the decoders of the batched path take every core this process may use (at most 128); the host stages of the batched
    // pipeline (state machines, contours) saturate at about 16.  ABUB_THREADS / ABUB_DECODE_THREADS override.
    const int cores = usableCores();
    int nthreads = std::min(cores, 128), hostThreads = std::min(cores, 16), decodeThreads = std::min(cores, 128);
    if (const char *t = getenv("ABUB_THREADS"))
        nthreads = hostThreads = decodeThreads = std::max(1, atoi(t));
    if (debug_mode % 100 / 10)
        nthreads = hostThreads = decodeThreads = 1;
    if (shardWorld > 1) // every shard writes its own part file (--merge N assembles the run's file)
        OutputWriter::PartSuffix = ".part" + std::to_string(shardRank) + "of" + std::to_string(shardWorld);

    // ---- a campaign: every run of --runs / --run-list in this process (abub::RunCampaign) ------------------------------
    if (!runs.empty()) {
        std::vector<abub::RunSpec> specs;
        for (const std::string &r : runs)
            specs.push_back(runSpec(dataLoc, data_series, r, zipped));
        abub::BatchedRunOptions bo = batchedOptions(ngpus, hostThreads, decodeThreads, shardRank, shardWorld, mask_dir);
        bo.outDir = out_dir;
        bo.peekDir = peekDir;
        bo.perEventThreads = nthreads;
        if (const char *t = getenv("ABUB_TRAIN_ON_GPU"))
            bo.trainOnGpu = atoi(t) != 0;
        abub::CampaignStats cs;
        const int rc = abub::RunCampaign(specs, bo, &cs);
        std::string notRun;
        for (const std::string &r : cs.notRun)
            notRun += (notRun.empty() ? "" : ",") + r;
        printf("campaign: %d runs, %lld frames, %.2f s, %.1f frames/s; training %.2f s (exposed %.2f s); pipelines built %d; "
               "not run: %s\n",
               cs.runs, cs.frames, cs.total_s, cs.total_s > 0 ? cs.frames / cs.total_s : 0.0, cs.train_s, cs.trainExposed_s,
               cs.pipelinesBuilt, notRun.empty() ? "none" : notRun.c_str());
        if (cs.framesGpuUnzipped || cs.trainGpuUnzipped)
            printf("campaign: %lld archive entries inflated on the GPU for the detect, %lld for the training\n", cs.framesGpuUnzipped,
                   cs.trainGpuUnzipped);
        return rc;
    }

    // header, event list (-5 rows if the run cannot be read), training (-7 rows if a camera fails): the campaign's steps
    abub::RunSpec spec = runSpec(dataLoc, data_series, run_number, zipped);
    abub::BatchedRunOptions po = batchedOptions(ngpus, hostThreads, decodeThreads, shardRank, shardWorld, mask_dir);
    po.outDir = out_dir;
    po.trainOnGpu = 0; // (a single run trains through the host Trainer, as the reference does)
    abub::PreparedRun prep = abub::PrepareRun(spec, po, debug_mode / 100, nullptr, false);
    abub::CommitRun(spec, po, prep);
    if (prep.rc)
        return prep.rc;
    Parser *FileParser = prep.parser.get();
    const std::vector<std::string> &EventList = prep.events;
    const std::vector<Trainer *> &Trainers = prep.trainers;

    // ---- batched detect (default): every event of a batch decoded once into pinned memory, one set of launches per
    // batch, output in event order.  The per-event loop below stays for -e / --debug / --per-event and as the
    // fallback when the batched path declines the run.
    if (const char *e = getenv("ABUB_PER_EVENT"))
        perEvent = perEvent || atoi(e) != 0;
    if (!perEvent && event_user < 0 && debug_mode == 0) {
        abub::BatchedRunOptions bo = batchedOptions(ngpus, hostThreads, decodeThreads, shardRank, shardWorld, mask_dir);
        bo.peekDir = peekDir;
        abub::BatchedRunStats bs;
        std::string why;
        int rc = 1;
        try {
            rc = abub::RunBatched(FileParser, EventList, Trainers, numCams, out_dir, run_number, frameOffset, bo, &bs, &why);
        } catch (std::exception &e) {
            std::cout << "batched detect failed: " << e.what() << std::endl;
            return -6;
        }
        if (rc == 0) {
            abub::PrintBatchedLine(bs);
            printf("run complete.\n");
            printf("AutoBub done analyzing this run. Thank you.\n");
            return 0;
        }
        std::cout << "batched detect not used (" << why << "): falling back to the per-event loop" << std::endl;
    }
    if (havePeek) // (ABUB_PER_EVENT=1, or a run the batched path declined)
        std::cout << "peek: no peek images were written (the per-event loop ran; --debug is its write-out)" << std::endl;

    abub::RunPerEvent(FileParser, EventList, Trainers, numCams, eventDir, out_dir, run_number, frameOffset, mask_dir, nthreads,
                      event_user, debug_mode, shardRank, shardWorld);
    printf("run complete.\n");
    printf("AutoBub done analyzing this run. Thank you.\n");
    return 0;
}
