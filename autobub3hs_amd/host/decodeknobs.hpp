// decodeknobs.hpp -- the opt-in knobs of the device reading path (framefiles.hpp), read from the environment once per batch
// or run and handed down from there; never cached: a process may change them between two runs.  All off by default:
// results are the same either way.  No HIP in here.
#ifndef ABUB3HS_DECODEKNOBS_HPP
#define ABUB3HS_DECODEKNOBS_HPP

#include <cstdlib>

namespace abub {

// is the variable set to a nonzero number?
inline bool envOn(const char *name)
{
    const char *e = getenv(name);
    return e && atoi(e) != 0;
}

struct DecodeKnobs {
    // ABUB_GPU_BMP=1: BMP files go to the GPU decoder.  Unset, they stay with the reading threads and RunBatched's probe
    // does not accept them: the batched run of a BMP directory measured slower with it than without ("BMP frames on the GPU")
    bool bmp = false;
    // ABUB_GPU_PNG_TYPES=1: the PNG lane also takes 16-bit, colour, grey+alpha and sub-byte files (every non-interlaced type
    // the host decoder reads; abub_png_decode_typed_dev; "PNG types on the GPU")
    bool pngTypes = false;
    // ABUB_GPU_PNG_ADAM7=1: the PNG lane also takes Adam7-interlaced files of the kinds it takes anyway (8-bit grey / palette;
    // with ABUB_GPU_PNG_TYPES=1 the 13 others too; abub_png_decode_adam7_dev; "Interlaced PNG")
    bool pngAdam7 = false;
    // ABUB_GPU_UNZIP=1: the zip layer of deflated archive entries is inflated on the GPU (abub_unzip_dev)
    bool unzip = false;

    static DecodeKnobs fromEnv()
    {
        return {envOn("ABUB_GPU_BMP"), envOn("ABUB_GPU_PNG_TYPES"), envOn("ABUB_GPU_PNG_ADAM7"), envOn("ABUB_GPU_UNZIP")};
    }
};

} // namespace abub
#endif
