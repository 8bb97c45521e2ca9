// abub_abf_enc.hip -- packed frames ("ABF1") encoded on the GPU: abub_abf_encode_dev (include/abub_hip.h, DESIGN section 3,
// "Packed frames").  It writes the bytes cv::abfEncode (host/abf.cpp) writes: smallest width per block, zero padding bits,
// zero table padding.
//
// The mapping is the decoder's (abub_abf.hip): a wave owns a row, its 64 lanes are the pixels of a block.  Where a file
// lies depends on the sizes of all files in front of it, and where a row lies on the sizes of the rows above it, so the
// work is cut where one step needs what all workgroups of the step before wrote, and every cut is a kernel boundary: no
// workgroup ever waits for another one inside a launch.
//   measure      one wave per row: the blocks' widths, the row's size and its check -> scratch
//   place rows   one workgroup per frame: row sizes -> row offsets, the frame's payload and file length
//   place files  one workgroup: file lengths -> off, status, *total (k_enc_place_files, abub_enc.hpp: shared with the PNG encoder)
//   write        one wave per row: table entry, widths, blocks; the waves of row 0 also the header and the table padding
// Every output byte is written once by one lane, so nothing is cleared beforehand and no atomics are needed.  The string
// bytes of a block are gathered: lane i + 1 collects the residuals that reach into string byte i with ds_bpermute (at most
// 8 gathers, for blocks of 1 and 2 bits) and stores the finished byte; no LDS is allocated.
//
// Bounds.  A frame is read only when src + W * H <= pixels_bytes (E_SRC otherwise, found alike by every kernel).  A file is
// written only when off + len <= out_cap (E_CAP otherwise); within it every store lies below len: the widths come from
// measure (<= 8 by construction, clamped again where they are read), and the row offsets are sums of the sizes those widths
// give.  Every loop bound is a function of W, H and nframes.
#include "abub_enc.hpp"

namespace {

#define ABFE_WAVES 4         /* waves per block, a row each at a time */
#define ABFE_ROWS_PER_WAVE 8 /* rows a wave handles, where the frame has that many */

__device__ __forceinline__ uint32_t abfe_block_bytes(int n, uint32_t b) { return 1u + (((uint32_t)(n - 1) * b + 7u) >> 3); }
// pixel `lane` of the block at `blk` (n pixels) and its zigzagged difference to the left neighbour (0 for lane 0 and the
// lanes behind the block)
__device__ __forceinline__ void abfe_load_block(const uint8_t *__restrict__ blk, int n, int lane, uint32_t &p, uint32_t &z)
{
    p = lane < n ? (uint32_t)blk[lane] : 0u;
    const int32_t s = (int32_t)(int8_t)(uint8_t)(p - enc_left_neighbour(p));
    z = (lane >= 1 && lane < n) ? (uint32_t)((s << 1) ^ (s >> 7)) & 0xffu : 0u;
}

// rows[f * H + y] = (size of row y, its check); widths[(f * H + y) * nblk + k] = bit width of block k
__global__ __launch_bounds__(64 * ABFE_WAVES) void k_abf_enc_measure(const uint8_t *__restrict__ pixels, uint64_t pixels_bytes,
                                                                     const uint64_t *__restrict__ src, int W, int H,
                                                                     uint2 *__restrict__ rows, uint8_t *__restrict__ widths)
{
    const uint32_t f = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t P = (uint64_t)W * (uint64_t)H, s = src[f];
    if (!frame_in_range(s, pixels_bytes, P))
        return; // (nobody reads this frame's scratch)
    const uint8_t *img = pixels + s;
    const uint32_t nblk = ((uint32_t)W + 63u) >> 6;
    uint2 *frows = rows + (uint64_t)f * (uint32_t)H;
    uint8_t *fw = widths + (uint64_t)f * (uint32_t)H * nblk;

    for (int y = (int)blockIdx.y * ABFE_WAVES + wv; y < H; y += (int)gridDim.y * ABFE_WAVES) {
        const uint8_t *row = img + (uint64_t)y * (uint32_t)W;
        uint32_t rsize = 0, acc = 0;
        for (uint32_t k0 = 0; k0 < nblk; k0 += 64) {
            const int nb = (int)min(64u, nblk - k0);
            uint32_t mine = 0; // the width of block k0 + lane
            for (int j = 0; j < nb; ++j) {
                const int x0 = (int)(k0 + j) * 64, n = min(64, W - x0);
                uint32_t p, z;
                abfe_load_block(row + x0, n, lane, p, z);
                uint32_t b = 0; // the bit length of the OR of every z
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    b += __ballot((z >> i) != 0u) != 0ull;
                rsize += abfe_block_bytes(n, b);
                acc += (uint32_t)(x0 + lane + 1) * p;
                if (lane == j)
                    mine = b;
            }
            if (lane < nb)
                fw[(uint64_t)y * nblk + k0 + lane] = (uint8_t)mine;
        }
        acc = wave_sum(acc);
        if (lane == 0)
            frows[y] = make_uint2(rsize, acc);
    }
}

// rows[f * H + y].x: size -> offset of the row in the payload; flen[f] = the file's length (0 for a frame that is not read)
__global__ __launch_bounds__(ENC_SCAN) void k_abf_enc_place_rows(uint64_t pixels_bytes, const uint64_t *__restrict__ src, int W,
                                                                   int H, uint2 *__restrict__ rows, uint32_t *__restrict__ flen)
{
    __shared__ uint32_t sh[ENC_SCAN / 64];
    const uint32_t f = blockIdx.x;
    const uint64_t P = (uint64_t)W * (uint64_t)H;
    if (!frame_in_range(src[f], pixels_bytes, P)) { // (the same answer in every thread)
        if (threadIdx.x == 0)
            flen[f] = 0;
        return;
    }
    const uint32_t nblk = ((uint32_t)W + 63u) >> 6;
    uint2 *frows = rows + (uint64_t)f * (uint32_t)H;
    uint32_t base = 0; // (a file is shorter than 2^32 bytes: abub_abf_file_bound)
    for (int y0 = 0; y0 < H; y0 += ENC_SCAN) {
        const int y = y0 + (int)threadIdx.x;
        const uint32_t size = y < H ? frows[y].x : 0u;
        uint32_t all;
        const uint32_t incl = enc_block_scan(size, sh, all);
        if (y < H)
            frows[y].x = base + incl - size;
        base += all;
    }
    if (threadIdx.x == 0)
        flen[f] = 32u + 8u * (uint32_t)H + (((uint32_t)H * nblk + 3u) & ~3u) + base;
}

// ceil(32768 / b) for b = 1 .. 8, 16 bits each: t / b == (t * r) >> 15 for t <= 504 (the error t * (r - 32768 / b) / 32768
// stays below 1 / 64, the fraction of t / b at or below 1 - 1 / b)
__device__ __forceinline__ uint32_t abfe_recip(uint32_t b)
{
    const uint64_t tab = b <= 4u ? 0x20002AAB40008000ull : 0x1000124A1556199Aull;
    return (uint32_t)(tab >> (16u * ((b - 1u) & 3u))) & 0xffffu;
}

__global__ __launch_bounds__(64 * ABFE_WAVES) void k_abf_enc_write(const uint8_t *__restrict__ pixels,
                                                                   const uint64_t *__restrict__ src, int W, int H,
                                                                   const uint2 *__restrict__ rows,
                                                                   const uint8_t *__restrict__ widths,
                                                                   const abub_abf_file *__restrict__ files,
                                                                   uint8_t *__restrict__ out)
{
    const uint32_t f = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const abub_abf_file rec = files[f];
    if (rec.status != 0)
        return; // (E_SRC: nothing to read; E_CAP: no room: none of the file's bytes is written)
    const uint8_t *img = pixels + src[f];
    const uint32_t nblk = ((uint32_t)W + 63u) >> 6;
    const uint32_t tab = 32u + 8u * (uint32_t)H, wcount = (uint32_t)H * nblk, wbytes = (wcount + 3u) & ~3u;
    const uint2 *frows = rows + (uint64_t)f * (uint32_t)H;
    const uint8_t *fw = widths + (uint64_t)f * (uint32_t)H * nblk;
    uint8_t *file = out + rec.off, *pay = file + tab + wbytes;

    for (int y = (int)blockIdx.y * ABFE_WAVES + wv; y < H; y += (int)gridDim.y * ABFE_WAVES) {
        const uint2 r = frows[y]; // (offset in the payload, check)
        if (lane < 8)
            file[32u + 8u * (uint32_t)y + lane] = (uint8_t)((lane < 4 ? r.x : r.y) >> (8 * (lane & 3)));
        if (y == 0) {
            if (lane < 32) {
                const uint32_t q = (uint32_t)lane >> 2;
                const uint32_t word = q == 0 ? 0x31464241u /* "ABF1" */ : q == 1 ? (uint32_t)W : q == 2 ? (uint32_t)H
                                      : q == 3 ? nblk : q == 4 ? rec.len - tab - wbytes : 0u;
                file[lane] = (uint8_t)(word >> (8 * (lane & 3)));
            }
            if ((uint32_t)lane < wbytes - wcount)
                file[tab + wcount + lane] = 0;
        }
        const uint8_t *row = img + (uint64_t)y * (uint32_t)W;
        const uint8_t *wrow = fw + (uint64_t)y * nblk;
        uint8_t *prow = pay + r.x, *wout = file + tab + (uint64_t)y * nblk;
        uint32_t base = 0;
        for (uint32_t k0 = 0; k0 < nblk; k0 += 64) {
            // where the blocks k0 .. k0 + 63 start: a scan of their sizes
            const uint32_t k = k0 + lane;
            uint32_t b = 0, size = 0;
            if (k < nblk) {
                b = min((uint32_t)wrow[k], 8u);
                size = abfe_block_bytes(min(64, W - (int)k * 64), b);
                wout[k] = (uint8_t)b;
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
            for (int j = 0; j < nb; ++j) {
                const uint32_t s0 = __builtin_amdgcn_readlane(start, j), b0 = __builtin_amdgcn_readlane(b, j);
                const int x0 = (int)(k0 + j) * 64, n = min(64, W - x0);
                uint32_t p, z;
                abfe_load_block(row + x0, n, lane, p, z);
                // lane i + 1 makes string byte i: bits 8 i .. 8 i + 7, residual r (lane r + 1) sits at bit r * b0
                const uint32_t t0 = lane ? 8u * (uint32_t)(lane - 1) : 0u, r0 = b0 ? (t0 * abfe_recip(b0)) >> 15 : 0u;
                uint32_t bits = 0;
#pragma unroll
                for (uint32_t m = 0; m < 8; ++m) { // (residuals r0 .. r0 + m while they start within 16 bits of r0's first)
                    if (m * b0 >= 16u || (b0 == 0u && m > 0u))
                        break; // (the same in every lane)
                    const uint32_t from = r0 + m + 1u;
                    const uint32_t zz = (uint32_t)__shfl((int)z, (int)(from & 63u));
                    bits |= (lane >= 1 && from < 64u ? zz : 0u) << (m * b0);
                }
                const uint32_t v = lane == 0 ? p : (bits >> (t0 - r0 * b0)) & 0xffu;
                if ((uint32_t)lane < abfe_block_bytes(n, b0))
                    prow[s0 + lane] = (uint8_t)v;
            }
        }
    }
}

} // namespace

extern "C" size_t abub_abf_file_bound(int W, int H)
{
    if (W < 1 || W > 65535 || H < 1 || H > 65535)
        return 0;
    const uint64_t nblk = ((uint64_t)W + 63) / 64;
    const uint64_t v = 32 + 8 * (uint64_t)H + (((uint64_t)H * nblk + 3) & ~(uint64_t)3) + (uint64_t)W * (uint64_t)H;
    return v >= ((uint64_t)1 << 32) ? 0 : (size_t)v;
}

// rows (8 bytes per row), file lengths (4 per frame), widths (1 per block), each part at a multiple of 16
extern "C" size_t abub_abf_encode_scratch_bytes(int nframes, int W, int H)
{
    if (nframes < 0 || !abub_abf_file_bound(W, H))
        return 0;
    const size_t nblk = ((size_t)W + 63) / 64, n = (size_t)nframes;
    return align16z(n * (size_t)H * 8) + align16z(n * 4) + align16z(n * (size_t)H * nblk) + 16;
}

extern "C" int abub_abf_encode_dev(const uint8_t *pixels, size_t pixels_bytes, const uint64_t *src, int nframes, int W, int H,
                                   uint8_t *out, size_t out_cap, abub_abf_file *files, uint64_t *total, void *scratch,
                                   size_t scratch_bytes, void *stream)
{
    if (const int e = enc_check_args("abub_abf_encode", abub_abf_file_bound, abub_abf_encode_scratch_bytes, pixels, src, nframes, W, H, out,
                                     files, total, scratch, scratch_bytes))
        return e;
    if (nframes == 0)
        return ABUB_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)nframes;
    uint8_t *sc = (uint8_t *)scratch;
    uint2 *rows = (uint2 *)sc;
    uint32_t *flen = (uint32_t *)(sc + align16z(n * (size_t)H * 8));
    uint8_t *widths = (uint8_t *)flen + align16z(n * 4);
    const int perBlock = ABFE_WAVES * ABFE_ROWS_PER_WAVE;
    const dim3 grid((unsigned)nframes, (unsigned)((H + perBlock - 1) / perBlock));
    k_abf_enc_measure<<<grid, 64 * ABFE_WAVES, 0, st>>>(pixels, (uint64_t)pixels_bytes, src, W, H, rows, widths);
    HIPCHK(hipGetLastError());
    k_abf_enc_place_rows<<<(unsigned)nframes, ENC_SCAN, 0, st>>>((uint64_t)pixels_bytes, src, W, H, rows, flen);
    HIPCHK(hipGetLastError());
    k_enc_place_files<<<1, ENC_SCAN, 0, st>>>((uint64_t)pixels_bytes, src, nframes, (uint64_t)W * (uint64_t)H, flen, (uint32_t)sizeof *flen,
                                               (uint64_t)out_cap, files, total);
    HIPCHK(hipGetLastError());
    k_abf_enc_write<<<grid, 64 * ABFE_WAVES, 0, st>>>(pixels, src, W, H, rows, widths, files, out);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}
