// pngwalk.hpp -- what a host thread finds out about a PNG file before its bytes go to the GPU decoder
// (abub_png_decode_dev, abub_png.hip): the IDAT chunks and, for a palette image, the palette -> grey table.
#ifndef ABUB3HS_PNGWALK_HPP
#define ABUB3HS_PNGWALK_HPP

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "abub_hip.h"

namespace abub {

// What a host thread finds out about a PNG file before its bytes go to the GPU decoder: the IDAT chunks and, for a
// palette image, the palette -> grey table (the same rounding as cv::imdecode's, cvlite.cpp).  false = not an 8-bit grey
// or palette image of W x H without interlace (or not a PNG at all): such a file is decoded on the host.
// typed (ABUB_GPU_PNG_TYPES=1, abub_png_decode_typed_dev): every non-interlaced W x H file the host decoder reads (cvlite.cpp,
// decodePNGTo) is accepted -- grey at 1, 2, 4, 8, 16 bits, palette at 1, 2, 4, 8, grey+alpha, RGB and RGBA at 8 and 16 -- and
// `kind` says which: 0 for the two 8-bit ones, else colour type | bit depth << 8 (abub_png_frame.kind).
// adam7 (ABUB_GPU_PNG_ADAM7=1, abub_png_decode_adam7_dev): an Adam7-interlaced file (interlace method 1) is accepted under the
// same rules of kind as a non-interlaced one, and `kind` gets ABUB_PNG_KIND_ADAM7 or-ed in.
struct PngInfo {
    std::vector<abub_png_seg> segs; // offsets relative to the file's first byte
    bool palette = false;
    uint8_t lut[256];               // palette images: entries past the palette are 0, as the host decoder has them
    uint64_t zlen = 0;
    uint32_t kind = 0;
};
// Adam7 (interlace method 1): pass p = 0 .. 6 of a w x h image holds the pixels (y0 + r * dy, x0 + c * dx), pw x ph of them; a
// pass without pixels is not in the stream
struct Adam7Pass {
    uint64_t x0, y0, dx, dy, pw, ph;
};
inline Adam7Pass adam7Pass(int p, uint64_t w, uint64_t h)
{
    static const uint8_t x0[7] = {0, 4, 0, 2, 0, 1, 0}, y0[7] = {0, 0, 4, 0, 2, 0, 1}, dx[7] = {8, 8, 4, 4, 2, 2, 1}, dy[7] = {8, 8, 8, 4, 4, 2, 2};
    return Adam7Pass{x0[p], y0[p], dx[p], dy[p], w > x0[p] ? (w - x0[p] + dx[p] - 1) / dx[p] : 0, h > y0[p] ? (h - y0[p] + dy[p] - 1) / dy[p] : 0};
}
// bytes of the inflated stream of an Adam7 file: the scanlines (filter type + row) of the passes that have pixels
inline uint64_t pngAdam7Bytes(uint64_t w, uint64_t h, uint64_t bitsPerPixel)
{
    uint64_t n = 0;
    for (int p = 0; p < 7; ++p) {
        const Adam7Pass a = adam7Pass(p, w, h);
        if (a.pw && a.ph)
            n += a.ph * ((a.pw * bitsPerPixel + 7) / 8 + 1);
    }
    return n;
}
inline bool pngWalk(const uint8_t *buf, size_t size, int W, int H, PngInfo &out, bool typed = false, bool adam7 = false)
{
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (size < 8 + 25 || memcmp(buf, sig, 8) != 0)
        return false;
    auto be32 = [&](size_t o) { return ((uint32_t)buf[o] << 24) | ((uint32_t)buf[o + 1] << 16) | ((uint32_t)buf[o + 2] << 8) | (uint32_t)buf[o + 3]; };
    out.segs.clear();
    out.palette = false;
    out.zlen = 0;
    out.kind = 0;
    uint8_t pal[256][3];
    int npal = 0;
    bool haveHdr = false, end = false;
    size_t o = 8;
    uint32_t w = 0, h = 0, depth = 0, ctype = 0, interlace = 1;
    while (!end && o + 12 <= size) {
        const uint32_t len = be32(o);
        const uint8_t *type = buf + o + 4, *data = buf + o + 8;
        if (o + 12 + (size_t)len > size)
            return false;
        if (!memcmp(type, "IHDR", 4) && len >= 13) {
            w = be32(o + 8);
            h = be32(o + 12);
            depth = data[8];
            ctype = data[9];
            interlace = data[12];
            haveHdr = true;
        } else if (!memcmp(type, "PLTE", 4)) {
            npal = std::min<int>((int)(len / 3), 256);
            memcpy(pal, data, (size_t)npal * 3);
        } else if (!memcmp(type, "IDAT", 4)) {
            out.segs.push_back(abub_png_seg{(uint32_t)(o + 8), len});
            out.zlen += len;
        } else if (!memcmp(type, "IEND", 4))
            end = true;
        o += 12 + (size_t)len;
    }
    if (!haveHdr || (int)w != W || (int)h != H || !(interlace == 0 || (adam7 && interlace == 1)) || out.segs.empty() ||
        out.zlen >= ((uint64_t)1 << 28) || size >= ((size_t)1 << 31))
        return false;
    uint64_t bits = 8; // per pixel
    if (depth != 8 || (ctype != 0 && ctype != 3)) {
        // the combinations of decodePNGTo, and the size of the inflated scanlines inside the kernels' 32-bit arithmetic
        const bool low = depth == 1 || depth == 2 || depth == 4;
        const bool known = ctype == 0 ? (low || depth == 16) : ctype == 3 ? low : (ctype == 2 || ctype == 4 || ctype == 6) && (depth == 8 || depth == 16);
        const uint64_t samples = ctype == 2 ? 3 : ctype == 4 ? 2 : ctype == 6 ? 4 : 1;
        const uint64_t rowBytes = ((uint64_t)w * samples * depth + 7) / 8;
        if (!typed || !known || (!interlace && (uint64_t)h * (rowBytes + 1) >= ((uint64_t)1 << 31)))
            return false;
        bits = samples * depth;
        out.kind = ctype | (depth << 8);
    }
    if (interlace) {
        if (pngAdam7Bytes(w, h, bits) >= ((uint64_t)1 << 31))
            return false;
        out.kind |= ABUB_PNG_KIND_ADAM7;
    }
    if (ctype == 3) {
        out.palette = true;
        for (int v = 0; v < 256; ++v)
            out.lut[v] = v < npal ? (uint8_t)((pal[v][0] * 9797 + pal[v][1] * 19234 + pal[v][2] * 3737 + 16384) >> 15) : 0;
    }
    return true;
}


} // namespace abub
#endif
