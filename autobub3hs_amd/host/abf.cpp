// abf.cpp -- host codec of the packed frame format "ABF1" ("Packed frames"; the GPU decoder is csrc/abub_abf.hip).
// A frame is cut into rows, a row into blocks of 64 pixels; a block stores its first pixel and the zigzagged differences
// of its neighbours at one bit width per block.  No row and no block depends on another one.  The acceptance rules here
// and in the kernel are the same, rule for rule.
#ifndef ABUB_USE_OPENCV
#include "cvlite.hpp"

#include <algorithm>
#include <cstring>

namespace cv {

namespace {
inline uint32_t ld32(const uchar *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline void st32(uchar *p, uint32_t v)
{
    p[0] = (uchar)v;
    p[1] = (uchar)(v >> 8);
    p[2] = (uchar)(v >> 16);
    p[3] = (uchar)(v >> 24);
}
inline uint32_t blockBytes(int n, int b) { return 1u + (uint32_t)(((n - 1) * b + 7) >> 3); }
} // namespace

bool abfEncode(const uchar *pixels, int W, int H, std::vector<uchar> &out)
{
    out.clear();
    if (!pixels || W < 1 || H < 1 || W > 65535 || H > 65535)
        return false;
    const uint32_t nblk = ((uint32_t)W + 63) / 64;
    const size_t tab = 32 + 8 * (size_t)H, wbytes = ((size_t)H * nblk + 3) & ~(size_t)3;
    out.assign(tab + wbytes, 0);
    out.reserve(tab + wbytes + (size_t)W * H);
    std::memcpy(out.data(), "ABF1", 4);
    st32(&out[4], (uint32_t)W);
    st32(&out[8], (uint32_t)H);
    st32(&out[12], nblk);
    uchar z[64];
    for (int y = 0; y < H; ++y) {
        const uchar *row = pixels + (size_t)y * W;
        st32(&out[32 + 8 * (size_t)y], (uint32_t)(out.size() - tab - wbytes));
        uint32_t check = 0;
        for (int x = 0; x < W; ++x)
            check += (uint32_t)(x + 1) * row[x];
        st32(&out[36 + 8 * (size_t)y], check);
        for (uint32_t k = 0; k < nblk; ++k) {
            const int x0 = (int)k * 64, n = std::min(64, W - x0);
            unsigned all = 0;
            for (int j = 1; j < n; ++j) {
                const int8_t s = (int8_t)(uchar)(row[x0 + j] - row[x0 + j - 1]);
                z[j] = (uchar)(((s << 1) ^ (s >> 7)) & 0xff);
                all |= z[j];
            }
            int b = 0;
            while (all >> b)
                ++b;
            out[tab + (size_t)y * nblk + k] = (uchar)b;
            const size_t at = out.size();
            out.resize(at + blockBytes(n, b), 0);
            out[at] = row[x0];
            for (int j = 1; j < n; ++j) {
                const int q = (j - 1) * b;
                const unsigned v = (unsigned)z[j] << (q & 7);
                out[at + 1 + (q >> 3)] |= (uchar)v;
                if (v >> 8)
                    out[at + 2 + (q >> 3)] |= (uchar)(v >> 8);
            }
        }
    }
    const size_t payload = out.size() - tab - wbytes;
    if (payload > 0xffffffffu)
        return false;
    st32(&out[16], (uint32_t)payload);
    return true;
}

bool abfProbe(const uchar *data, size_t size, int *W, int *H)
{
    if (!data || size < 32 || std::memcmp(data, "ABF1", 4))
        return false;
    const uint32_t w = ld32(data + 4), h = ld32(data + 8), nblk = ld32(data + 12), payload = ld32(data + 16);
    if (w < 1 || h < 1 || w > 65535 || h > 65535 || nblk != (w + 63) / 64)
        return false;
    const uint64_t want = 32 + 8 * (uint64_t)h + (((uint64_t)h * nblk + 3) & ~(uint64_t)3) + payload;
    if (want != size)
        return false;
    if (W)
        *W = (int)w;
    if (H)
        *H = (int)h;
    return true;
}

// 0 = decoded, else the ABUB_ABF_E_* code the GPU decoder gives the same file (include/abub_hip.h): 2 header, 3 size,
// and of the row-level errors 4 (width) < 5 (row offsets) < 6 (row check) the largest; a row that fails 4 or 5 is not read
int abfDecodeStatus(const uchar *data, size_t size, uchar *dst, int W, int H)
{
    if (!data || !dst || W < 1 || H < 1 || W > 65535 || H > 65535)
        return 2;
    if (size < 32 || std::memcmp(data, "ABF1", 4))
        return 2;
    const uint32_t nblk = ((uint32_t)W + 63) / 64, payload = ld32(data + 16);
    if (ld32(data + 4) != (uint32_t)W || ld32(data + 8) != (uint32_t)H || ld32(data + 12) != nblk)
        return 2;
    const uint64_t tab = 32 + 8 * (uint64_t)H, wbytes = ((uint64_t)H * nblk + 3) & ~(uint64_t)3;
    if (tab + wbytes + payload != size)
        return 3;
    int err = 0;
    for (int y = 0; y < H; ++y) {
        const uchar *wrow = data + tab + (size_t)y * nblk;
        uint64_t rsize = 0;
        bool wide = false;
        for (uint32_t k = 0; k < nblk; ++k) {
            wide = wide || wrow[k] > 8;
            rsize += blockBytes(std::min(64, W - (int)k * 64), wrow[k]);
        }
        if (wide) {
            err = std::max(err, 4);
            continue;
        }
        const uint32_t off = ld32(data + 32 + 8 * (size_t)y), check = ld32(data + 36 + 8 * (size_t)y);
        const uint32_t next = y + 1 < H ? ld32(data + 40 + 8 * (size_t)y) : payload;
        if ((y == 0 && off != 0) || off + rsize != next || off + rsize > payload) {
            err = std::max(err, 5);
            continue;
        }
        const uchar *p = data + tab + wbytes + off;
        uchar *row = dst + (size_t)y * W;
        uint32_t sum = 0;
        for (uint32_t k = 0; k < nblk; ++k) {
            const int x0 = (int)k * 64, n = std::min(64, W - x0), b = wrow[k];
            unsigned v = p[0];
            row[x0] = (uchar)v;
            for (int j = 1; j < n; ++j) {
                const int q = (j - 1) * b;
                unsigned w = b ? p[1 + (q >> 3)] : 0u;
                if ((q & 7) + b > 8)
                    w |= (unsigned)p[2 + (q >> 3)] << 8;
                const unsigned z = (w >> (q & 7)) & ((1u << b) - 1u);
                v = (v + ((z >> 1) ^ (0u - (z & 1u)))) & 0xffu;
                row[x0 + j] = (uchar)v;
            }
            p += blockBytes(n, b);
        }
        for (int x = 0; x < W; ++x)
            sum += (uint32_t)(x + 1) * row[x];
        if (sum != check)
            err = std::max(err, 6);
    }
    return err;
}

bool abfDecodeInto(const uchar *data, size_t size, uchar *dst, int W, int H) { return abfDecodeStatus(data, size, dst, W, H) == 0; }

} // namespace cv
#endif
