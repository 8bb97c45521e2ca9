// abub_bmp.hip -- BMP frames decoded on the GPU: abub_bmp_decode_dev (include/abub_hip.h, DESIGN section 3, "BMP frames on the GPU").
//
// A BMP frame is its pixels, uncompressed: rows upside down, padded to 4 bytes, behind at most a 256-entry palette.  The
// host walks the header (host/bmpwalk.hpp) and hands over a descriptor; the kernel never reads a header and believes the
// descriptor alone.  The grid is frames x groups of 32 rows, a wave owns 8 whole rows, so nothing is shared between waves
// and a clean frame touches its status word only through the memset in front of the launch.
//
// The 8-bit route is the one real runs take.  A row is written in 16-byte pieces at 16-byte aligned addresses (bytes up
// to the first one and behind the last); the stored rows are usually not dword aligned (data_off = 1078 for the usual
// header and a full palette), so a piece is assembled from five aligned source dwords with v_alignbyte.  Such a load may
// reach up to 3 bytes in front of the row and 19 behind the piece: where that would leave [files, files + files_bytes)
// the piece is read byte by byte.  The 1, 4, 24 and 32 bit routes are a pixel per lane with byte loads.
//
// Every wave of a frame first makes the same decisions about the descriptor, in 64-bit arithmetic.  After them the file
// lies inside `files`, the H stored rows of `stride` bytes inside the file, a row holds the W pixels, and the frame's
// W * H bytes lie inside `out`: rows are read at data_off + stride * sy + [0, ceil(W * bpp / 8)) with sy < H, pixels
// written at dst + y * W + x with x < W, y < H.
#include "abub_dev.hpp"
#include <stddef.h>

namespace {

#define BMP_WAVES 4         /* waves per block */
#define BMP_ROWS_PER_WAVE 8 /* rows a wave decodes (amortises the descriptor checks) */

struct __attribute__((packed, aligned(4))) bmp_q {
    uint32_t v[4];
};

__device__ __forceinline__ uint32_t bmp_grey(uint32_t b, uint32_t g, uint32_t r)
{
    return (b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14;
}
__device__ __forceinline__ uint32_t bmp_map4(uint32_t v, const uint8_t *lut)
{
    return (uint32_t)lut[v & 255u] | (uint32_t)lut[(v >> 8) & 255u] << 8 | (uint32_t)lut[(v >> 16) & 255u] << 16 |
           (uint32_t)lut[v >> 24] << 24;
}

// one 8-bit row of W pixels: srow -> orow (any alignment each); lut: the frame's table in LDS, or nullptr
template <bool LUT>
__device__ __forceinline__ void bmp_row8(const uint8_t *__restrict__ files, uint64_t files_bytes, const uint8_t *__restrict__ srow,
                                         uint8_t *__restrict__ orow, uint32_t W, const uint8_t *lut, uint32_t lane)
{
    const uintptr_t lo = (uintptr_t)files, hi = lo + files_bytes;
    const uint32_t head = min((uint32_t)((16u - (uint32_t)((uintptr_t)orow & 15u)) & 15u), W);
    if (lane < head) {
        const uint32_t v = srow[lane];
        orow[lane] = LUT ? lut[v] : (uint8_t)v;
    }
    const uint32_t nu = (W - head) >> 4; // 16-byte pieces
    const uint8_t *s0 = srow + head;
    uint8_t *o0 = orow + head;
    const uint32_t mis = (uint32_t)((uintptr_t)s0 & 3u);
    const uintptr_t sw = (uintptr_t)s0 - mis;
    for (uint32_t k = lane; k < nu; k += 64) {
        const uintptr_t a = sw + 16u * (uintptr_t)k;
        uint32_t w0, w1, w2, w3;
        if (a >= lo && a + (mis ? 20u : 16u) <= hi) {
            const uint8_t *pa = files + (a - lo); // (the address a, still a pointer into `files`)
            const bmp_q q = *(const bmp_q *)pa;
            w0 = q.v[0];
            w1 = q.v[1];
            w2 = q.v[2];
            w3 = q.v[3];
            if (mis) {
                const uint32_t e = *(const uint32_t *)(pa + 16);
                w0 = __builtin_amdgcn_alignbyte(w1, w0, mis);
                w1 = __builtin_amdgcn_alignbyte(w2, w1, mis);
                w2 = __builtin_amdgcn_alignbyte(w3, w2, mis);
                w3 = __builtin_amdgcn_alignbyte(e, w3, mis);
            }
        } else { // (the aligned loads would leave `files`: the piece's own 16 bytes, which lie inside the row)
            const uint8_t *p = s0 + 16u * k;
            w0 = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
            w1 = (uint32_t)p[4] | (uint32_t)p[5] << 8 | (uint32_t)p[6] << 16 | (uint32_t)p[7] << 24;
            w2 = (uint32_t)p[8] | (uint32_t)p[9] << 8 | (uint32_t)p[10] << 16 | (uint32_t)p[11] << 24;
            w3 = (uint32_t)p[12] | (uint32_t)p[13] << 8 | (uint32_t)p[14] << 16 | (uint32_t)p[15] << 24;
        }
        if (LUT) {
            w0 = bmp_map4(w0, lut);
            w1 = bmp_map4(w1, lut);
            w2 = bmp_map4(w2, lut);
            w3 = bmp_map4(w3, lut);
        }
        *(uint4 *)(o0 + 16u * k) = make_uint4(w0, w1, w2, w3);
    }
    const uint32_t x = head + 16u * nu + lane; // (fewer than 16 bytes are left)
    if (x < W) {
        const uint32_t v = srow[x];
        orow[x] = LUT ? lut[v] : (uint8_t)v;
    }
}

__global__ __launch_bounds__(64 * BMP_WAVES) void k_bmp_decode(const uint8_t *__restrict__ files, uint64_t files_bytes,
                                                               const abub_bmp_frame *__restrict__ frames,
                                                               const uint8_t *__restrict__ luts, uint32_t nluts, int W, int H,
                                                               uint8_t *__restrict__ out, uint64_t out_bytes,
                                                               int32_t *__restrict__ status)
{
    __shared__ uint8_t s_lut[256];
    const uint32_t f = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const abub_bmp_frame d = frames[f];
    const uint64_t P = (uint64_t)W * (uint64_t)H;
    const uint32_t bpp = d.bpp;

    // ---- the descriptor: the same answer in every wave ------------------------------------------------------------------
    bool bad = !(bpp == 1u || bpp == 4u || bpp == 8u || bpp == 24u || bpp == 32u);
    bad = bad || (uint64_t)d.off + d.len > files_bytes;
    bad = bad || (uint64_t)d.data_off + (uint64_t)d.stride * (uint64_t)H > (uint64_t)d.len;
    bad = bad || (uint64_t)d.stride < ((uint64_t)W * bpp + 7u) / 8u;
    bad = bad || (d.lut != 0xffffffffu && d.lut >= nluts);
    bad = bad || d.dst > out_bytes || out_bytes - d.dst < P;
    if (bad) {
        if (blockIdx.y == 0 && threadIdx.x == 0)
            status[f] = ABUB_BMP_E_DESC;
        return;
    }
    const bool haveLut = bpp <= 8u && d.lut != 0xffffffffu;
    if (haveLut) { // (uniform in the block: every thread reads the same descriptor)
        s_lut[threadIdx.x] = luts[(uint64_t)d.lut * 256u + threadIdx.x];
        __syncthreads();
    }
    const uint8_t *pix = files + d.off + d.data_off;
    uint8_t *dst = out + d.dst;
    const bool topDown = (d.flags & 1u) != 0;
    const int y0 = ((int)blockIdx.y * BMP_WAVES + (int)wv) * BMP_ROWS_PER_WAVE;
    const int y1 = min(H, y0 + BMP_ROWS_PER_WAVE);

    for (int y = y0; y < y1; ++y) {
        const uint8_t *srow = pix + (uint64_t)d.stride * (uint32_t)(topDown ? y : H - 1 - y);
        uint8_t *orow = dst + (uint64_t)y * (uint32_t)W;
        if (bpp == 8u) {
            if (haveLut)
                bmp_row8<true>(files, files_bytes, srow, orow, (uint32_t)W, s_lut, lane);
            else
                bmp_row8<false>(files, files_bytes, srow, orow, (uint32_t)W, nullptr, lane);
        } else if (bpp == 1u) {
            for (uint32_t x = lane; x < (uint32_t)W; x += 64) {
                const uint32_t v = (srow[x >> 3] >> (7u - (x & 7u))) & 1u;
                orow[x] = haveLut ? s_lut[v] : (uint8_t)v;
            }
        } else if (bpp == 4u) {
            for (uint32_t x = lane; x < (uint32_t)W; x += 64) {
                const uint32_t v = (srow[x >> 1] >> ((x & 1u) ? 0u : 4u)) & 15u;
                orow[x] = haveLut ? s_lut[v] : (uint8_t)v;
            }
        } else {
            const uint32_t bytes = bpp >> 3; // 3 or 4
            for (uint32_t x = lane; x < (uint32_t)W; x += 64) {
                const uint8_t *p = srow + (uint64_t)x * bytes;
                orow[x] = (uint8_t)bmp_grey(p[0], p[1], p[2]);
            }
        }
    }
}

} // namespace

extern "C" int abub_bmp_decode_dev(const uint8_t *files, size_t files_bytes, const abub_bmp_frame *frames, int nframes,
                                   const uint8_t *luts, int nluts, int W, int H, uint8_t *out, size_t out_bytes,
                                   int32_t *status, void *stream)
{
    if (!files || !frames || !out || !status || nframes < 0 || nluts < 0 || (!luts && nluts != 0))
        return set_err(ABUB_E_INVALID, "abub_bmp_decode_dev: null pointer or negative count");
    if (W < 1 || W > 65535 || H < 1 || H > 65535)
        return set_err(ABUB_E_INVALID, "abub_bmp_decode_dev: width and height must be in [1, 65535]");
    if (nframes == 0)
        return ABUB_OK;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(status, 0, (size_t)nframes * sizeof(int32_t), st));
    const int perBlock = BMP_WAVES * BMP_ROWS_PER_WAVE;
    const dim3 grid((unsigned)nframes, (unsigned)((H + perBlock - 1) / perBlock));
    k_bmp_decode<<<grid, 64 * BMP_WAVES, 0, st>>>(files, (uint64_t)files_bytes, frames, luts, (uint32_t)nluts, W, H, out,
                                                  (uint64_t)out_bytes, status);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}
