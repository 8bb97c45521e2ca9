// devtrain.hpp -- the background models of every camera of a run trained in one pass on the device: the same frames, skip
// rules, entropy veto and float Welford recurrence as Trainer::MakeAvgSigmaImage (Trainer.cpp, the reference's
// AlgorithmTraining/Trainer.cpp:221-331), with the training frames decoded by abub_png_decode_dev / abub_abf_decode_dev into one slab, the veto
// histograms of every (camera, event) pair from one abub_pair_hist_dev launch and one abub_train_dev per camera.
#ifndef ABUB3HS_DEVTRAIN_HPP
#define ABUB3HS_DEVTRAIN_HPP

#include <cstddef>
#include <string>
#include <vector>

#include "framefiles.hpp"

class Parser;
class Trainer;

namespace abub {

// What TrainOnDevice allocates, kept by a caller that trains run after run (RunCampaign): the pinned file buffer is
// page-locked once, not per run.  Declaration order: the stream finishes its work before the buffers go.
struct DeviceTrainBuffers {
    FileBatch batch; // the training frames' files, the decoders' scratch, the slab
    DeviceBuffer pairs, hist, idx, mu, sigma;
    Stream stream;
};

struct DeviceTrainOptions {
    int device = 0;
    int threads = 4;                     // host threads that read the files (and decode what the GPU decoder refuses)
    size_t capBytes = (size_t)3 << 30;   // the training slab (every camera's training frames) may not be larger
    int gpuDecode = -1;                  // 0: every frame decoded by host threads (ABUB_GPU_DECODE=0 as in RunBatched)
    DeviceTrainBuffers *buffers = nullptr; // kept from one call to the next (null: allocated for this call)
    std::string *log = nullptr;          // the host path's stdout lines go here instead of stdout (null: printed)
};

struct DeviceTrainStats {
    double total_s = 0;
    long long frames = 0, framesGpuDecoded = 0, framesHostDecoded = 0;
    long long framesGpuUnpacked = 0; // of framesGpuDecoded: packed frames, by abub_abf_decode_dev
    long long framesGpuBmp = 0;      // of framesGpuDecoded: BMP frames, by abub_bmp_decode_dev
    long long framesGpuUnzipped = 0; // ABUB_GPU_UNZIP=1: archive entries whose zip layer abub_unzip_dev inflated
    size_t slabBytes = 0;
    int decodeLaunches = 0;
};

// Trains Trainers[c] (camera c, the run's EventList in output order) for every c.  Returns 0 when the models were made here:
// each Trainer then holds what MakeAvgSigmaImage would (TrainedAvgImage, TrainedSigmaImage, TrainingSetSize, StatusCode,
// a fresh ModelId; -7 where the host path fails: a parser exception, an empty training set).  Frame size: the first training
// frame that decodes sets it; an event whose two frames both decode but not both at that size fails the camera (-7).  The
// host path throws there when the pair is kept, and computes the veto histogram of two frames of different sizes past the
// end of the smaller one; one case differs: a pair of two frames of the same other size that the veto drops (the host
// skips it, here the camera fails).  An event with a missing or corrupt frame is skipped whatever the size of the other.
// The PNG frames are decoded in launches of at most 4 frames per CU (the decoder's scratch stays that of RunBatched).
// Returns a positive code, with `why` set and the Trainers untouched, when the run does not fit (slab above the cap, cameras
// of different frame sizes, a training sequence other than two frames): the caller then trains on the host.  Throws on
// GPU failures.
int TrainOnDevice(Parser *parser, const std::vector<std::string> &EventList, std::vector<Trainer *> &Trainers,
                  const DeviceTrainOptions &opt, DeviceTrainStats *stats = nullptr, std::string *why = nullptr);

} // namespace abub
#endif
