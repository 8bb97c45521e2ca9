// bmpwalk.hpp -- what a host thread finds out about a BMP file before its bytes go to the GPU decoder
// (abub_bmp_decode_dev, abub_bmp.hip): where the pixel array lies, how it is stored, and the palette -> grey table.
// decodeBMP (cvlite.cpp) is the definition; this restates its acceptance rules one for one and reads no pixel.
#ifndef ABUB3HS_BMPWALK_HPP
#define ABUB3HS_BMPWALK_HPP

#include <cstddef>
#include <cstdint>

namespace abub {

struct BmpInfo {
    uint32_t dataOff = 0; // of the pixel array inside the file
    uint32_t stride = 0;  // bytes from one stored row to the next
    int bpp = 0;          // 1 | 4 | 8 | 24 | 32
    bool topDown = false;
    bool identity = true; // bpp <= 8: lut[i] == i for every i (an 8-bit frame then needs no look-up)
    uint8_t lut[256];     // bpp <= 8: index -> grey, decodeBMP's `pal`
};

// bgr2grey of cvlite.cpp
inline uint8_t bmpBgr2grey(int b, int g, int r) { return (uint8_t)((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14); }

// true exactly when decodeBMP returns a W x H image for these bytes
inline bool bmpWalk(const uint8_t *buf, size_t size, int W, int H, BmpInfo &out)
{
    auto u16 = [&](size_t o) { return (unsigned)buf[o] | ((unsigned)buf[o + 1] << 8); };
    auto u32 = [&](size_t o) { return (unsigned)buf[o] | ((unsigned)buf[o + 1] << 8) | ((unsigned)buf[o + 2] << 16) | ((unsigned)buf[o + 3] << 24); };
    if (!buf || size < 54 || buf[0] != 'B' || buf[1] != 'M')
        return false;
    const unsigned dataOff = u32(10), hdr = u32(14);
    if (hdr < 40)
        return false;
    const long long w = (int)u32(18);
    long long h = (int)u32(22); // (64 bits: -h of the most negative height stays a number no frame has)
    const unsigned bpp = u16(28), comp = u32(30);
    unsigned ncol = u32(46);
    out.topDown = h < 0;
    if (h < 0)
        h = -h;
    if (w <= 0 || h <= 0 || (comp != 0 && !(comp == 3 && bpp == 32)) ||
        !(bpp == 1 || bpp == 4 || bpp == 8 || bpp == 24 || bpp == 32))
        return false;
    if (w != W || h != H)
        return false;
    const size_t stride = ((size_t)w * bpp + 31) / 32 * 4;
    if ((size_t)dataOff + stride * (size_t)h > size || stride > 0xffffffffu)
        return false;
    out.dataOff = dataOff;
    out.stride = (uint32_t)stride;
    out.bpp = (int)bpp;
    out.identity = true;
    for (unsigned i = 0; i < 256; ++i)
        out.lut[i] = (uint8_t)i;
    if (bpp <= 8) {
        if (ncol == 0)
            ncol = 1u << bpp;
        const size_t po = 14u + hdr; // (32-bit, as decodeBMP computes it)
        for (unsigned i = 0; i < ncol && i < 256 && po + 4 * (size_t)i + 3 < size; ++i) {
            out.lut[i] = bmpBgr2grey(buf[po + 4 * i], buf[po + 4 * i + 1], buf[po + 4 * i + 2]);
            out.identity = out.identity && out.lut[i] == i;
        }
    }
    return true;
}

} // namespace abub
#endif
