// abub_zip_pack.hip -- the files a GPU encoder left in device memory packed into a segment of the canonical zip archive of
// abub3hs --archive (abub_zip_pack_dev; the contract is in include/abub_hip.h, the layout in DESIGN section 3, "A run as one
// archive").  Three launches:
//   k_zip_pack_check   one thread per item: the descriptor against the buffers, status[i], crc[i] = 0
//   k_zip_pack_tiles   over (item, tile of ABUB_ZIP_PACK_TILE bytes): every source byte is loaded once, 16 bytes per lane and
//                      load, stored to its place behind the header and fed to the CRC; the tile's register is moved over the
//                      bytes behind the tile (x^(8 * bytes), carry-less) and xor-ed into crc[i]
//   k_zip_pack_heads   one wave per item: the CRC conditioned, the local header, the name, the padding field
// A thread of the tile kernel takes the 16-byte pieces t, t + 256, t + 512, ... of its tile, so that a wave's loads and
// stores are contiguous.  Its register runs over a piece with the slice-by-4 tables and jumps the 255 pieces of the other
// threads with a second set of tables (the multiplication by the constant x^(8 * 4080) is linear, hence four lookups); at the
// end of a whole tile the register of thread t is moved to the tile's end by one multiplication with the constant
// x^(8 * 16 * (255 - t)), in a ragged tile by crc_shift.
#include "abub_crc.hpp"
#include <stddef.h>
#include <algorithm>

namespace {

#define ZP_THREADS 256
constexpr uint32_t ZP_TILE = ABUB_ZIP_PACK_TILE;
static_assert(ZP_TILE % (16u * ZP_THREADS) == 0, "a whole tile gives every thread the same number of pieces");
static_assert(sizeof(abub_zip_item) == 32, "abub_zip_item is the 32 bytes include/abub_hip.h states");

struct ZpTables {
    uint32_t skip[4][256];     // skip[b][v]: the register (v << 8 b) times x^(8 * (16 * ZP_THREADS - 16))
    uint32_t lane[ZP_THREADS]; // x^(8 * 16 * k)
};
constexpr uint32_t zp_xpow8(uint32_t nbytes)
{
    uint32_t r = 0x80000000u, base = 0x00800000u; // x^0, x^8
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1u)
            r = crc_mul(r, base);
        base = crc_mul(base, base);
    }
    return r;
}
constexpr ZpTables zp_make_tables()
{
    ZpTables T{};
    const uint32_t c = zp_xpow8(16u * ZP_THREADS - 16u);
    for (int b = 0; b < 4; ++b) {
        for (int j = 0; j < 8; ++j) // the products of the single bits, the rest by linearity
            T.skip[b][1u << j] = crc_mul((1u << j) << (8 * b), c);
        for (uint32_t v = 1; v < 256; ++v)
            if (v & (v - 1))
                T.skip[b][v] = T.skip[b][v & (v - 1)] ^ T.skip[b][v & (~v + 1u)];
    }
    const uint32_t p16 = zp_xpow8(16u);
    T.lane[0] = 0x80000000u;
    for (int k = 1; k < ZP_THREADS; ++k)
        T.lane[k] = crc_mul(T.lane[k - 1], p16);
    return T;
}
__device__ const ZpTables zp_tables = zp_make_tables();

// the bytes in front of an item's data
__device__ __forceinline__ uint64_t zp_head(const abub_zip_item &it) { return 30ull + it.name_len + it.extra_len; }

__device__ __forceinline__ bool zp_item_bad(const abub_zip_item &it, uint64_t buf_bytes, uint64_t names_bytes, uint64_t seg_bytes)
{
    const uint64_t head = zp_head(it), all = head + it.len; // (< 2^33)
    return (it.src & 15) || it.src > buf_bytes || it.len > buf_bytes - it.src || it.len == 0xffffffffu || it.name > names_bytes ||
           it.name_len > names_bytes - it.name || (it.extra_len >= 1 && it.extra_len <= 3) || it.dst > seg_bytes ||
           all > seg_bytes - it.dst || (it.len && ((it.dst + head) & 15));
}

__global__ __launch_bounds__(ZP_THREADS) void k_zip_pack_check(uint64_t buf_bytes, const abub_zip_item *__restrict__ items, int nitems,
                                                               uint64_t names_bytes, uint64_t seg_bytes, uint32_t *__restrict__ crc,
                                                               int32_t *__restrict__ status)
{
    const int i = (int)(blockIdx.x * ZP_THREADS + threadIdx.x);
    if (i >= nitems)
        return;
    status[i] = zp_item_bad(items[i], buf_bytes, names_bytes, seg_bytes) ? ABUB_ZIP_E_DESC : 0;
    crc[i] = 0;
}

// grid (nitems, tiles in flight per item): block (i, y) takes the tiles y, y + gridDim.y, ... of item i
__global__ __launch_bounds__(ZP_THREADS) void k_zip_pack_tiles(const uint8_t *__restrict__ buf, const abub_zip_item *__restrict__ items,
                                                               uint8_t *__restrict__ seg, const int32_t *__restrict__ status,
                                                               uint32_t *__restrict__ crc)
{
    __shared__ uint32_t tab[4][256], skip[4][256];
    __shared__ uint32_t acc;
    const uint32_t i = blockIdx.x, tid = threadIdx.x;
    if (status[i] != 0) // (the same for the whole workgroup)
        return;
    const abub_zip_item it = items[i];
    const uint64_t n = it.len;
    const uint64_t ntiles = (n + ZP_TILE - 1u) / ZP_TILE;
    if (blockIdx.y >= ntiles)
        return;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        tab[s][tid] = crc_tables.t[s][tid];
        skip[s][tid] = zp_tables.skip[s][tid];
    }
    const uint8_t *__restrict__ src = buf + it.src;
    uint8_t *__restrict__ dst = seg + it.dst + zp_head(it);
    for (uint64_t tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
        if (tid == 0)
            acc = 0;
        __syncthreads(); // (the tables the first time round; acc)
        const uint64_t start = tile * ZP_TILE;
        const uint32_t L = (uint32_t)min((uint64_t)ZP_TILE, n - start), q = L >> 4, rem = L & 15u;
        const uint8_t *__restrict__ s = src + start;
        uint8_t *__restrict__ d = dst + start;
        uint32_t r = tile == 0 && tid == 0 && q ? 0xffffffffu : 0u; // (the pre-conditioning, in front of the file's first byte)
        uint32_t last = tid;
#pragma unroll 4
        for (uint32_t j = tid; j < q; j += ZP_THREADS) {
            const uint4 v = *(const uint4 *)(s + 16u * j);
            *(uint4 *)(d + 16u * j) = v;
            if (j != tid) // over the other threads' pieces since this thread's last one
                r = skip[0][r & 255] ^ skip[1][(r >> 8) & 255] ^ skip[2][(r >> 16) & 255] ^ skip[3][r >> 24];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                r ^= w[k];
                r = tab[3][r & 255] ^ tab[2][(r >> 8) & 255] ^ tab[1][(r >> 16) & 255] ^ tab[0][r >> 24];
            }
            last = j;
        }
        if (tid < q) { // to the tile's end
            if (L == ZP_TILE)
                r = crc_mul(r, zp_tables.lane[ZP_THREADS - 1 - tid]);
            else
                r = crc_shift(r, 16u * (q - 1u - last) + rem);
        }
        if (tid == 0 && rem) { // the file's last bytes, fewer than 16 (only its last tile has any)
            uint32_t r2 = tile == 0 && q == 0 ? 0xffffffffu : 0u;
            for (uint32_t k = 16u * q; k < L; ++k) {
                const uint8_t b = s[k];
                d[k] = b;
                r2 = tab[0][(r2 ^ b) & 255] ^ (r2 >> 8);
            }
            r ^= r2;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            r ^= __shfl_xor(r, o);
        if ((tid & 63) == 0 && r)
            atomicXor(&acc, r);
        __syncthreads();
        if (tid == 0) {
            const uint64_t behind = n - (start + L); // (< 2^32)
            const uint32_t t = crc_shift(acc, (uint32_t)behind);
            if (t)
                atomicXor(&crc[i], t);
        }
        __syncthreads(); // (acc is cleared by the next round)
    }
}

__device__ __forceinline__ void zp_put16(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
}
__device__ __forceinline__ void zp_put32(uint8_t *p, uint32_t v)
{
    zp_put16(p, v);
    zp_put16(p + 2, v >> 16);
}

__global__ __launch_bounds__(64) void k_zip_pack_heads(const abub_zip_item *__restrict__ items, const uint8_t *__restrict__ names,
                                                       uint8_t *__restrict__ seg, const int32_t *__restrict__ status,
                                                       uint32_t *__restrict__ crc)
{
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (status[i] != 0)
        return;
    const abub_zip_item it = items[i];
    uint8_t *p = seg + it.dst;
    if (lane == 0) {
        const uint32_t c = it.len ? crc[i] ^ 0xffffffffu : 0u; // (the post-conditioning; an empty file's CRC is 0)
        crc[i] = c;
        zp_put32(p, 0x04034b50u);
        zp_put16(p + 4, 20);      // version needed
        zp_put16(p + 6, 0);       // flags
        zp_put16(p + 8, 0);       // method: stored
        zp_put16(p + 10, 0);      // time
        zp_put16(p + 12, 0x0021); // date: 1980-01-01
        zp_put32(p + 14, c);
        zp_put32(p + 18, it.len);
        zp_put32(p + 22, it.len);
        zp_put16(p + 26, it.name_len);
        zp_put16(p + 28, it.extra_len);
    }
    for (uint32_t k = lane; k < it.name_len; k += 64)
        p[30 + k] = names[(uint64_t)it.name + k];
    uint8_t *x = p + 30 + it.name_len;
    for (uint32_t k = lane; k < it.extra_len; k += 64) {
        const uint32_t field = 0x4241u | ((uint32_t)(it.extra_len - 4u) << 16);
        x[k] = k < 4 ? (uint8_t)(field >> (8 * k)) : (uint8_t)0;
    }
}

} // namespace

extern "C" int abub_zip_pack_dev(const uint8_t *buf, size_t buf_bytes, const abub_zip_item *items, int nitems, const uint8_t *names,
                                 size_t names_bytes, uint8_t *seg, size_t seg_bytes, uint32_t *crc, int32_t *status, void *stream)
{
    if (!buf || !items || !names || !seg || !crc || !status || nitems < 0)
        return set_err(ABUB_E_INVALID, "abub_zip_pack_dev: null pointer or negative count");
    if (nitems == 0)
        return ABUB_OK;
    if (((uintptr_t)buf & 15) || ((uintptr_t)seg & 15) || ((uintptr_t)items & 7) || ((uintptr_t)crc & 3) || ((uintptr_t)status & 3))
        return set_err(ABUB_E_INVALID, "abub_zip_pack_dev: buf / seg 16-byte, items 8-byte, crc / status 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    k_zip_pack_check<<<(unsigned)((nitems + ZP_THREADS - 1) / ZP_THREADS), ZP_THREADS, 0, st>>>((uint64_t)buf_bytes, items, nitems,
                                                                                                 (uint64_t)names_bytes, (uint64_t)seg_bytes,
                                                                                                 crc, status);
    // tiles in flight per item: about 4096 workgroups where the batch is small, never more than 64 per item (a file of 4 MiB)
    const unsigned perItem = (unsigned)std::min(64, std::max(1, (4096 + nitems - 1) / nitems));
    k_zip_pack_tiles<<<dim3((unsigned)nitems, perItem), ZP_THREADS, 0, st>>>(buf, items, seg, status, crc);
    k_zip_pack_heads<<<(unsigned)nitems, 64, 0, st>>>(items, names, seg, status, crc);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}
