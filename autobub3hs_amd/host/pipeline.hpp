// pipeline.hpp -- what the batched ingestion (runbatch.cpp: RunBatched) needs from the run pipeline (pipeline.cpp:
// RunPipeline).  Internal to the host library: the pipeline's own types stay in pipeline.cpp.
#ifndef ABUB3HS_PIPELINE_HPP
#define ABUB3HS_PIPELINE_HPP

#include <chrono>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

class OutputWriter;

namespace abub {

#define HIPOK(x)                                                                          \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess)                                                             \
            throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_));     \
    } while (0)

inline double nowMs()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// What a batched driver knows about one (event, camera) stack that came from a Parser: the reference's event id,
// the real frame names in the Parser's order and which of them decoded
struct StackMeta {
    std::string eventID;
    std::vector<std::string> names;
    std::vector<uint8_t> ok;
};

class RunPipeline;
struct RunPipelineDelete {
    void operator()(RunPipeline *p) const;
};
using RunPipelinePtr = std::unique_ptr<RunPipeline, RunPipelineDelete>;

// a pipeline for batches of E events of C cameras, F frames of W x H each, on `device`
RunPipelinePtr newRunPipeline(int device, int W, int H, int F, int E, int C, const int *tss, int nthreads,
                              const char *maskDir);
// a new model's training-set sizes (one per camera) for the runs to come; false, and nothing changed, when they would
// change the trigger search's frame offset the pipeline was built for (a new pipeline is needed then)
bool setTrainingSetSizes(RunPipeline &p, const int *tss);
// sigma (not 6 * sigma) of every camera, for the stacks that need the one-at-a-time path
void setSigmaRaw(RunPipeline &p, const uint8_t *d_sigma);
// the next run's ids, frame names and decode flags, one entry per stack
void setStackMeta(RunPipeline &p, std::vector<StackMeta> &&meta);
// the analysis of every stack of d_frames [E][C][F][H][W]; work queued on `stream` (the upload) is waited for first
void run(RunPipeline &p, const uint8_t *d_frames, const uint8_t *d_mu, const uint8_t *d_sigma6, hipStream_t stream);
// stacks of the last run whose bellows veto ran inside the batch
int bellowsVetoed(const RunPipeline &p);
// stack s = event * C + camera of the last run: its result, and the event id setStackMeta gave it
struct StackResult;
const StackResult &stackResult(const RunPipeline &p, int s);
const std::string &stackEventID(const RunPipeline &p, int s);
// event k's cameras of the last run staged into `out` and written as one block
void writeEvent(RunPipeline &p, int k, int eventNumber, OutputWriter &out);

} // namespace abub
#endif
