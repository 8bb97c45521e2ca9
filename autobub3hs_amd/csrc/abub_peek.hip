// abub_peek.hip -- the two DebugPeek planes no other kernel leaves behind: abub_peek_planes_dev (include/abub_hip.h, DESIGN
// section 3, "The peek planes").  Per item the thresholded image (reference L3Localizer.cpp:252-257: 255 where D > thr, the
// mask contoursOfCurrentImage hands back for the write-out at :257) and the presentation frame (:397, :448: the trigger
// frame with cv::rectangle drawn for every bubble box), both W x H u8, for a batch of resident frames.
//
// Two launches; the only dependence between workgroups is the boundary between them.
//   k_peek_copy  grid = items x contiguous 16 KiB tiles of the plane; a block of four waves owns a tile of both planes.  A
//                lane issues FR_UNR loads of D and FR_UNR loads of the frame before it uses any, compares the D bytes
//                four to a dword and stores 16 bytes of each plane.  Block (tile 0) of an item writes its status.
//   k_peek_draw  grid = items x PEEK_DRAW_BLOCKS; a block takes every PEEK_DRAW_BLOCKS-th rectangle of its item and its
//                threads store 255 along the clipped perimeter, a byte each.  Every rectangle pixel stores the same value,
//                so rectangles that overlap, and the two blocks that draw them, need no order.
//
// Widths.  The planes start at multiples of 16 from a 16-byte-aligned `out`, so every store of k_peek_copy but the last
// P mod 16 bytes of a plane is a 16-byte store.  A source is read 16 bytes at a time where its address is a multiple of
// 16, 4 where a multiple of 4, else byte by byte; D and the frame choose independently.
//
// Bounds.  peek_item_status is evaluated alike by every block of both kernels.  It admits an item only when both sources
// lie in their buffers, both planes are multiples of 16 that lie in [0, out_bytes) and do not overlap each other, and its
// rectangle range lies in [0, nrects].  For an admitted item the copy walks [0, P) as abub_frames.hpp describes, with
// 16-byte units and no head: a load touches bytes [0, P) of its source and a store the same bytes of its plane; a draw
// store has index y * W + x with 0 <= x < W and 0 <= y < H of the presentation plane.  Nothing of a refused item is read
// or written but status[item].
#include "abub_frames.hpp"

namespace {

#define PEEK_DRAW_BLOCKS 4 /* blocks that share an item's rectangles */

// 0, or the ABUB_PEEK_E_* code that keeps the item from being touched
__device__ __forceinline__ int peek_item_status(const abub_peek_item &it, uint64_t diff_bytes, uint64_t frames_bytes, uint64_t out_bytes,
                                                int nrects, uint64_t P)
{
    if (!frame_in_range(it.diff, diff_bytes, P) || !frame_in_range(it.frame, frames_bytes, P))
        return ABUB_PEEK_E_SRC;
    if (((it.thr_out | it.pres_out) & 15u) || !frame_in_range(it.thr_out, out_bytes, P) || !frame_in_range(it.pres_out, out_bytes, P))
        return ABUB_PEEK_E_DST;
    if ((it.thr_out > it.pres_out ? it.thr_out - it.pres_out : it.pres_out - it.thr_out) < P)
        return ABUB_PEEK_E_DST; // (the two planes overlap)
    if (it.rect_begin < 0 || it.rect_count < 0 || (int64_t)it.rect_begin + it.rect_count > (int64_t)nrects)
        return ABUB_PEEK_E_RECT;
    return 0;
}

// 16 bytes from p + 16 i, by the widest loads MODE allows: 16 (p a multiple of 16), 4 (of 4), 1
template <int MODE>
__device__ __forceinline__ u32x4 peek_load(const uint8_t *p, uint32_t i)
{
    if constexpr (MODE == 16)
        return reinterpret_cast<const u32x4 *>(p)[i];
    else if constexpr (MODE == 4) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p) + (size_t)i * 4;
        return u32x4{q[0], q[1], q[2], q[3]};
    } else {
        const uint8_t *q = p + (size_t)i * 16;
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            w[k] = (uint32_t)q[4 * k] | (uint32_t)q[4 * k + 1] << 8 | (uint32_t)q[4 * k + 2] << 16 | (uint32_t)q[4 * k + 3] << 24;
        return u32x4{w[0], w[1], w[2], w[3]};
    }
}

// The threshold of an item, prepared once: byte b of cut(x) is 255 where byte b of x is > thr.  With c = thr + 1 in
// [1, 255] the test is x >= c per byte: the high bits decide where they differ, else the low seven do, and
// (xl | 0x80) - cl borrows from no neighbour because xl | 0x80 >= 0x80 > cl.
struct PeekCut {
    uint32_t cl, nch, all, keep;
    __device__ __forceinline__ explicit PeekCut(int thr)
    {
        const uint32_t c = (uint32_t)(thr < 0 ? 1 : thr > 254 ? 255 : thr + 1) * 0x01010101u;
        cl = c & 0x7f7f7f7fu;
        nch = ~c & 0x80808080u;
        all = thr < 0 ? 0xffffffffu : 0u;    // every byte is > a negative threshold
        keep = thr > 254 ? 0u : 0xffffffffu; // no byte is > 255 or more
    }
    __device__ __forceinline__ uint32_t operator()(uint32_t x) const
    {
        const uint32_t xh = x & 0x80808080u;
        const uint32_t gel = (((x & 0x7f7f7f7fu) | 0x80808080u) - cl) & 0x80808080u; // bit 7: low seven bits >= those of c
        const uint32_t same = ~(xh ^ ~nch) & 0x80808080u;                             // bit 7: the high bits agree
        const uint32_t m = ((xh & nch) | (same & gel)) >> 7;                          // 0 or 1 per byte
        return (((m << 8) - m) | all) & keep;
    }
    __device__ __forceinline__ u32x4 operator()(u32x4 v) const
    {
        return u32x4{(*this)(v.x), (*this)(v.y), (*this)(v.z), (*this)(v.w)};
    }
};

// One step of both planes: FR_THREADS * FR_UNR units from `base` on; MD, MF: the load widths of D and of the frame
template <int MD, int MF, bool FULL>
__device__ __forceinline__ void peek_step(const uint8_t *d, const uint8_t *f, u32x4 *ot, u32x4 *op, uint32_t base, uint32_t end,
                                          const PeekCut &cut)
{
    u32x4 vd[FR_UNR], vf[FR_UNR];
#pragma unroll
    for (int u = 0; u < FR_UNR; ++u) {
        const uint32_t i = base + (uint32_t)u * FR_THREADS + threadIdx.x;
        if (FULL || i < end)
            vd[u] = peek_load<MD>(d, i);
    }
#pragma unroll
    for (int u = 0; u < FR_UNR; ++u) {
        const uint32_t i = base + (uint32_t)u * FR_THREADS + threadIdx.x;
        if (FULL || i < end)
            vf[u] = peek_load<MF>(f, i);
    }
#pragma unroll
    for (int u = 0; u < FR_UNR; ++u) {
        const uint32_t i = base + (uint32_t)u * FR_THREADS + threadIdx.x;
        if (FULL || i < end) {
            ot[i] = cut(vd[u]);
            op[i] = vf[u];
        }
    }
}

// Tile `tile` of an item's two planes: this kernel's own copy of frame_walk, 16-byte units and no head (through the shared
// walk it measured up to 1.4 % slower than before, profiles/r22/frames_ab.json)
template <int MD, int MF>
__device__ __forceinline__ void peek_tile(const uint8_t *d, const uint8_t *f, uint8_t *ot, uint8_t *op, uint32_t P, uint32_t tile,
                                          const PeekCut &cut)
{
    constexpr uint32_t PER_TILE = FR_TILE / 16u, STEP = FR_THREADS * FR_UNR;
    const uint32_t nunits = P / 16u, tail = P - nunits * 16u;
    // (tile < 2^18 and PER_TILE = 2^10: the products stay below 2^32)
    const uint32_t first = tile * PER_TILE, end = min(nunits, first + PER_TILE);
    if (first < end) {
        if (end - first >= STEP) // (the same in every thread of the block; PER_TILE == STEP)
            peek_step<MD, MF, true>(d, f, reinterpret_cast<u32x4 *>(ot), reinterpret_cast<u32x4 *>(op), first, end, cut);
        else
            peek_step<MD, MF, false>(d, f, reinterpret_cast<u32x4 *>(ot), reinterpret_cast<u32x4 *>(op), first, end, cut);
    }
    if (tile == 0 && threadIdx.x < tail) { // the last P mod 16 bytes, one per lane
        const uint32_t at = nunits * 16u + threadIdx.x;
        ot[at] = (uint8_t)cut((uint32_t)d[at]);
        op[at] = f[at];
    }
}

// body(mode) with the width a source at p is read in, as a std::integral_constant: 16, 4 or 1
template <class Body>
__device__ __forceinline__ void peek_mode(const uint8_t *p, Body body)
{
    const uint32_t low = (uint32_t)(uintptr_t)p;
    if ((low & 15u) == 0u)
        body(std::integral_constant<int, 16>());
    else if ((low & 3u) == 0u)
        body(std::integral_constant<int, 4>());
    else
        body(std::integral_constant<int, 1>());
}

__global__ __launch_bounds__(FR_THREADS) void k_peek_copy(const uint8_t *diff, uint64_t diff_bytes, const uint8_t *frames,
                                                            uint64_t frames_bytes, const abub_peek_item *__restrict__ items, int nitems,
                                                            int nrects, uint32_t P, uint8_t *out, uint64_t out_bytes,
                                                            int32_t *__restrict__ status)
{
    for (uint32_t p = blockIdx.y; p < (uint32_t)nitems; p += gridDim.y) {
        const abub_peek_item it = items[p];
        const int st = peek_item_status(it, diff_bytes, frames_bytes, out_bytes, nrects, P);
        if (blockIdx.x == 0 && threadIdx.x == 0)
            status[p] = st;
        if (st)
            continue; // (the same in every thread of every block of the item)
        const uint8_t *d = diff + it.diff, *f = frames + it.frame;
        uint8_t *ot = out + it.thr_out, *op = out + it.pres_out;
        const PeekCut cut(it.thr);
        peek_mode(d, [&](auto md) { peek_mode(f, [&](auto mf) { peek_tile<md, mf>(d, f, ot, op, P, blockIdx.x, cut); }); });
    }
}

// cv::rectangle of host/cvlite.cpp, thickness 1: rows y and y + h - 1, columns x and x + w - 1, each clipped to the frame
__global__ __launch_bounds__(FR_THREADS) void k_peek_draw(uint64_t diff_bytes, uint64_t frames_bytes, const abub_peek_item *__restrict__ items,
                                                            int nitems, const abub_peek_rect *__restrict__ rects, int nrects, int W, int H,
                                                            uint8_t *out, uint64_t out_bytes)
{
    const uint32_t P = (uint32_t)W * (uint32_t)H;
    for (uint32_t p = blockIdx.y; p < (uint32_t)nitems; p += gridDim.y) {
        const abub_peek_item it = items[p];
        if (it.rect_count <= 0 || peek_item_status(it, diff_bytes, frames_bytes, out_bytes, nrects, P))
            continue;
        uint8_t *op = out + it.pres_out;
        for (int r = (int)blockIdx.x; r < it.rect_count; r += PEEK_DRAW_BLOCKS) {
            const abub_peek_rect rc = rects[it.rect_begin + r]; // (rect_begin + r < rect_begin + rect_count <= nrects)
            if (rc.w <= 0 || rc.h <= 0)
                continue;
            const int64_t x0 = rc.x, y0 = rc.y, x1 = x0 + rc.w - 1, y1 = y0 + rc.h - 1;
            const int64_t cx0 = x0 > 0 ? x0 : 0, cx1 = x1 < W - 1 ? x1 : W - 1; // columns of the two rows
            const int64_t cy0 = y0 > 0 ? y0 : 0, cy1 = y1 < H - 1 ? y1 : H - 1; // rows of the two columns
            if (cx0 > cx1 || cy0 > cy1)
                continue; // (wholly outside: no row and no column of it meets the frame)
            const uint32_t nx = (uint32_t)(cx1 - cx0 + 1), ny = (uint32_t)(cy1 - cy0 + 1); // (<= 65535 each)
            const bool top = y0 >= 0 && y0 < H, bottom = y1 >= 0 && y1 < H, left = x0 >= 0 && x0 < W, right = x1 >= 0 && x1 < W;
            for (uint32_t i = threadIdx.x; i < nx; i += FR_THREADS) {
                if (top)
                    op[(uint32_t)y0 * (uint32_t)W + (uint32_t)cx0 + i] = 255;
                if (bottom)
                    op[(uint32_t)y1 * (uint32_t)W + (uint32_t)cx0 + i] = 255;
            }
            for (uint32_t i = threadIdx.x; i < ny; i += FR_THREADS) {
                if (left)
                    op[((uint32_t)cy0 + i) * (uint32_t)W + (uint32_t)x0] = 255;
                if (right)
                    op[((uint32_t)cy0 + i) * (uint32_t)W + (uint32_t)x1] = 255;
            }
        }
    }
}

} // namespace

extern "C" int abub_peek_planes_dev(const uint8_t *diff, size_t diff_bytes, const uint8_t *frames, size_t frames_bytes,
                                    const abub_peek_item *items, int nitems, const abub_peek_rect *rects, int nrects, int W, int H,
                                    uint8_t *out, size_t out_bytes, int32_t *status, void *stream)
{
    if (!diff || !frames || !items || !out || !status || nitems < 0 || nrects < 0 || (!rects && nrects > 0))
        return set_err(ABUB_E_INVALID, "abub_peek_planes_dev: null pointer or negative count");
    if (W < 1 || W > 65535 || H < 1 || H > 65535)
        return set_err(ABUB_E_INVALID, "abub_peek_planes_dev: W and H must be in [1, 65535]");
    if (((uintptr_t)items & 7) || ((uintptr_t)rects & 3) || ((uintptr_t)status & 3) || ((uintptr_t)out & 15))
        return set_err(ABUB_E_INVALID, "abub_peek_planes_dev: items must be 8-byte, rects and status 4-byte, out 16-byte aligned");
    if (nitems == 0)
        return ABUB_OK;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t P = (uint32_t)W * (uint32_t)H; // (<= 65535^2 < 2^32)
    const dim3 grid = frame_grid(P, nitems);
    k_peek_copy<<<grid, FR_THREADS, 0, st>>>(
        diff, (uint64_t)diff_bytes, frames, (uint64_t)frames_bytes, items, nitems, nrects, P, out, (uint64_t)out_bytes, status);
    HIPCHK(hipGetLastError());
    if (nrects > 0) { // (an item cannot name a rectangle of an empty list: its rect_count is 0, or it is refused)
        k_peek_draw<<<dim3(PEEK_DRAW_BLOCKS, grid.y), FR_THREADS, 0, st>>>((uint64_t)diff_bytes, (uint64_t)frames_bytes, items, nitems, rects,
                                                                         nrects, W, H, out, (uint64_t)out_bytes);
        HIPCHK(hipGetLastError());
    }
    return ABUB_OK;
}
