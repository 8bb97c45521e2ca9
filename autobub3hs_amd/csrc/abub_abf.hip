// abub_abf.hip -- packed frames ("ABF1") decoded on the GPU: abub_abf_decode_dev (include/abub_hip.h, DESIGN section 3, "Packed frames").
//
// The format is made for this mapping.  A row is a sequence of blocks of 64 pixels, a block is its first pixel followed
// by 63 zigzagged differences at one bit width: the 64 lanes of a wave are the pixels of a block, a lane takes its
// difference out of the bit string with one or two byte loads, and "add the differences" is one wave scan.  Two blocks
// share a scan: their values sit in the two 16-bit halves of a dword, and a sum of 64 bytes never leaves its half.  A wave
// owns whole rows, so the row check needs no atomics and a clean frame touches its status word only through the memset in
// front of the launch.
//
// The input is file content.  Every wave of a frame first makes the same decisions about the descriptor and the header
// (E_DESC, E_HEADER, E_SIZE) from values it has bounds-checked against files_bytes; after those checks the header, the
// row table and the widths lie inside the file.  A row is only read when its widths are all <= 8 and its offset plus the
// size the widths give stays inside payload_bytes, which is inside the file; a block is read within the bytes its width
// gives it.  Pixels are written at dst + y * W + x with x < W, y < H, and dst + W * H <= out_bytes was checked.
#include "abub_dev.hpp"
#include <stddef.h>

namespace {

#define ABF_WAVES 4         /* waves per block, a row each at a time */
#define ABF_ROWS_PER_WAVE 8 /* rows a wave decodes (amortises the header checks), where the frame has that many */

__device__ __forceinline__ uint32_t abf_ld32(const uint8_t *p)
{
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
__device__ __forceinline__ uint32_t abf_block_bytes(int n, uint32_t b) { return 1u + (((uint32_t)(n - 1) * b + 7u) >> 3); }
__device__ __forceinline__ uint32_t abf_wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_xor(v, o);
    return v;
}
// the difference of pixel `lane` (1 .. n-1) of a block whose bit string starts at pb + 1; 0 for b = 0
__device__ __forceinline__ uint32_t abf_delta(const uint8_t *__restrict__ pb, uint32_t b, int lane)
{
    const uint32_t q = (uint32_t)(lane - 1) * b, sh = q & 7u;
    uint32_t w = pb[1 + (q >> 3)];
    if (sh + b > 8u) // (only then does the value reach into the next byte, which the block's size then covers)
        w |= (uint32_t)pb[2 + (q >> 3)] << 8;
    const uint32_t z = (w >> sh) & ((1u << b) - 1u);
    return ((z >> 1) ^ (0u - (z & 1u))) & 0xffu;
}

__global__ __launch_bounds__(64 * ABF_WAVES) void k_abf_decode(const uint8_t *__restrict__ files, uint64_t files_bytes,
                                                               const abub_abf_frame *__restrict__ frames, int W, int H,
                                                               uint8_t *__restrict__ out, uint64_t out_bytes,
                                                               int32_t *__restrict__ status)
{
    const uint32_t f = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const abub_abf_frame d = frames[f];
    const uint64_t P = (uint64_t)W * (uint64_t)H;
    const uint32_t nblk = ((uint32_t)W + 63u) >> 6;
    const uint64_t tab = 32 + 8 * (uint64_t)H, wbytes = ((uint64_t)H * nblk + 3) & ~(uint64_t)3;

    // ---- the frame's own errors: the same answer in every wave ------------------------------------------------------
    int ferr = 0;
    uint32_t payload = 0;
    const uint8_t *file = files + d.off;
    if ((uint64_t)d.off + d.len > files_bytes || d.dst > out_bytes || out_bytes - d.dst < P)
        ferr = ABUB_ABF_E_DESC;
    else if (d.len < 32 || abf_ld32(file) != 0x31464241u /* "ABF1" */ || abf_ld32(file + 4) != (uint32_t)W ||
             abf_ld32(file + 8) != (uint32_t)H || abf_ld32(file + 12) != nblk)
        ferr = ABUB_ABF_E_HEADER;
    else {
        payload = abf_ld32(file + 16);
        if (tab + wbytes + payload != (uint64_t)d.len)
            ferr = ABUB_ABF_E_SIZE;
    }
    if (ferr) {
        if (blockIdx.y == 0 && threadIdx.x == 0)
            status[f] = ferr; // (no row-level code is written for this frame: nobody reads its rows)
        return;
    }
    const uint8_t *widths = file + tab, *pay = file + tab + wbytes;
    uint8_t *dst = out + d.dst;

    for (int y = (int)blockIdx.y * ABF_WAVES + wv; y < H; y += (int)gridDim.y * ABF_WAVES) {
        const uint8_t *wrow = widths + (uint64_t)y * nblk;
        // ---- the row's widths: all <= 8, and the size they give the row -----------------------------------------------
        uint32_t rsize = 0;
        bool wide = false;
        for (uint32_t k = lane; k < nblk; k += 64) {
            const uint32_t b = wrow[k];
            const int n = min(64, W - (int)k * 64);
            wide = wide || b > 8u;
            rsize += abf_block_bytes(n, b > 8u ? 0u : b);
        }
        int rerr = 0;
        if (__any(wide))
            rerr = ABUB_ABF_E_WIDTH;
        else {
            rsize = abf_wave_sum(rsize); // (at most 1024 blocks of 64 bytes)
            const uint8_t *te = file + 32 + 8 * (uint64_t)y;
            const uint32_t off = abf_ld32(te), next = y + 1 < H ? abf_ld32(te + 8) : payload;
            if ((y == 0 && off != 0) || (uint64_t)off + rsize != (uint64_t)next || (uint64_t)off + rsize > (uint64_t)payload)
                rerr = ABUB_ABF_E_ROWS;
            else {
                const uint8_t *prow = pay + off;
                uint8_t *orow = dst + (uint64_t)y * (uint32_t)W;
                uint32_t base = 0, acc = 0;
                for (uint32_t k0 = 0; k0 < nblk; k0 += 64) {
                    // where the blocks k0 .. k0 + 63 start: a scan of their sizes
                    const uint32_t k = k0 + lane;
                    uint32_t b = 0, size = 0;
                    if (k < nblk) {
                        b = wrow[k];
                        size = abf_block_bytes(min(64, W - (int)k * 64), b);
                    }
                    uint32_t incl = size;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const uint32_t t = __shfl_up(incl, o);
                        if (lane >= o)
                            incl += t;
                    }
                    const uint32_t start = base + incl - size;
                    base += __shfl(incl, 63);
                    const int nb = (int)min(64u, nblk - k0);
                    for (int j = 0; j < nb; j += 2) { // two blocks per scan
                        const bool two = j + 1 < nb;
                        const uint32_t s0 = __builtin_amdgcn_readlane(start, j), b0 = __builtin_amdgcn_readlane(b, j);
                        const uint32_t s1 = __builtin_amdgcn_readlane(start, two ? j + 1 : j);
                        const uint32_t b1 = __builtin_amdgcn_readlane(b, two ? j + 1 : j);
                        const int x0 = (int)(k0 + j) * 64, n0 = min(64, W - x0), n1 = two ? min(64, W - x0 - 64) : 0;
                        uint32_t v = 0;
                        if (lane == 0)
                            v = prow[s0] | (two ? (uint32_t)prow[s1] << 16 : 0u);
                        else {
                            if (lane < n0 && b0)
                                v = abf_delta(prow + s0, b0, lane);
                            if (lane < n1 && b1)
                                v |= abf_delta(prow + s1, b1, lane) << 16;
                        }
#pragma unroll
                        for (int o = 1; o < 64; o <<= 1) {
                            const uint32_t t = __shfl_up(v, o);
                            if (lane >= o)
                                v += t;
                        }
                        const uint32_t p0 = v & 0xffu, p1 = (v >> 16) & 0xffu;
                        if (lane < n0) {
                            orow[x0 + lane] = (uint8_t)p0;
                            acc += (uint32_t)(x0 + lane + 1) * p0;
                        }
                        if (lane < n1) {
                            orow[x0 + 64 + lane] = (uint8_t)p1;
                            acc += (uint32_t)(x0 + 64 + lane + 1) * p1;
                        }
                    }
                }
                acc = abf_wave_sum(acc);
                if (acc != abf_ld32(te + 4))
                    rerr = ABUB_ABF_E_CHECK;
            }
        }
        if (rerr && lane == 0)
            atomicMax(&status[f], rerr); // (the launcher zeroed the word: the largest row-level code wins)
    }
}

} // namespace

extern "C" int abub_abf_decode_dev(const uint8_t *files, size_t files_bytes, const abub_abf_frame *frames, int nframes, int W,
                                   int H, uint8_t *out, size_t out_bytes, int32_t *status, void *stream)
{
    if (!files || !frames || !out || !status || nframes < 0)
        return set_err(ABUB_E_INVALID, "abub_abf_decode_dev: null pointer or negative count");
    if (W < 1 || W > 65535 || H < 1 || H > 65535)
        return set_err(ABUB_E_INVALID, "abub_abf_decode_dev: width and height must be in [1, 65535]");
    if (nframes == 0)
        return ABUB_OK;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(status, 0, (size_t)nframes * sizeof(int32_t), st));
    const int perBlock = ABF_WAVES * ABF_ROWS_PER_WAVE;
    const dim3 grid((unsigned)nframes, (unsigned)((H + perBlock - 1) / perBlock));
    k_abf_decode<<<grid, 64 * ABF_WAVES, 0, st>>>(files, (uint64_t)files_bytes, frames, W, H, out, (uint64_t)out_bytes, status);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}
