// pnghuff.cpp -- the canonical Huffman-only PNG writer ("Unpacking a run"): cv::pngHuffEncode.  Sub filter
// on every row, one dynamic-Huffman deflate block of literals, no LZ77; every choice is fixed by rule, so this file, the GPU
// encoder (csrc/abub_png_enc.hip) and the tests' numpy restatement write the same bytes.  This one defines them.
#ifndef ABUB_USE_OPENCV
#include "cvlite.hpp"

#include <algorithm>
#include <cstring>

#include <zlib.h>

namespace cv {

namespace {

const int kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct BitWriter {
    std::vector<uchar> &out;
    uint64_t acc = 0;
    int n = 0;
    void put(uint32_t v, int bits) // the `bits` low bits of v, least significant first
    {
        acc |= (uint64_t)v << n;
        for (n += bits; n >= 8; n -= 8, acc >>= 8)
            out.push_back((uchar)acc);
    }
    void flush()
    {
        if (n)
            out.push_back((uchar)acc);
        acc = 0;
        n = 0;
    }
};

inline uint32_t reverseBits(uint32_t c, int n)
{
    uint32_t r = 0;
    for (int i = 0; i < n; ++i)
        r |= ((c >> i) & 1u) << (n - 1 - i);
    return r;
}

// RFC 1951 3.2.2, each code reversed: ready for the LSB-first bit stream
void canonicalCodes(const uchar *len, int n, uint32_t *code)
{
    int count[17] = {0};
    for (int s = 0; s < n; ++s)
        ++count[len[s]];
    count[0] = 0;
    uint32_t next[17] = {0}, c = 0;
    for (int b = 1; b <= 16; ++b)
        next[b] = c = (c + (uint32_t)count[b - 1]) << 1;
    for (int s = 0; s < n; ++s)
        code[s] = len[s] ? reverseBits(next[len[s]]++, len[s]) : 0;
}

void be32(uchar *p, uint32_t v)
{
    p[0] = (uchar)(v >> 24);
    p[1] = (uchar)(v >> 16);
    p[2] = (uchar)(v >> 8);
    p[3] = (uchar)v;
}

} // namespace

int pngHuffLengths(const uint64_t *counts, int n, int limit, uchar *lengths)
{
    std::fill(lengths, lengths + n, (uchar)0);
    if (n < 2 || n > 288 || limit < 1 || limit > 15)
        return -1;
    // 1. the used symbols ascending by (count, symbol)
    int used[288], m = 0;
    for (int s = 0; s < n; ++s)
        if (counts[s])
            used[m++] = s;
    if (m < 2)
        return -1;
    std::sort(used, used + m, [&](int a, int b) { return counts[a] != counts[b] ? counts[a] < counts[b] : a < b; });
    // 2. two queues: the leaves in that order, the internal nodes as they are made; the leaf first on equal weight
    uint64_t weight[2 * 288];
    int parent[2 * 288];
    for (int i = 0; i < m; ++i)
        weight[i] = counts[used[i]];
    int leaf = 0, inner = m;
    for (int node = m; node < 2 * m - 1; ++node) {
        uint64_t w = 0;
        for (int k = 0; k < 2; ++k) {
            const int take = leaf < m && (inner >= node || weight[leaf] <= weight[inner]) ? leaf++ : inner++;
            parent[take] = node;
            w += weight[take];
        }
        weight[node] = w;
    }
    int depth[2 * 288], deepest = 0;
    depth[2 * m - 2] = 0;
    for (int i = 2 * m - 3; i >= 0; --i)
        depth[i] = depth[parent[i]] + 1;
    // 3. leaves per depth, a depth above the limit counted as the limit
    int per[16] = {0};
    for (int i = 0; i < m; ++i) {
        deepest = std::max(deepest, depth[i]);
        ++per[std::min(depth[i], limit)];
    }
    // 4. while the Kraft sum exceeds 1: one code off the limit, one shorter code split in two
    uint64_t kraft = 0;
    for (int d = 1; d <= limit; ++d)
        kraft += (uint64_t)per[d] << (limit - d);
    for (; kraft > (uint64_t)1 << limit; --kraft) {
        --per[limit];
        int d = limit - 1;
        while (d > 0 && !per[d])
            --d;
        if (d == 0)
            return -1; // (cannot happen: m <= 2^limit for both alphabets)
        --per[d];
        per[d + 1] += 2;
    }
    // 5. shortest first to the symbols by (count descending, symbol ascending)
    std::sort(used, used + m, [&](int a, int b) { return counts[a] != counts[b] ? counts[a] > counts[b] : a < b; });
    int at = 0;
    for (int d = 1; d <= limit; ++d)
        for (int k = 0; k < per[d]; ++k)
            lengths[used[at++]] = (uchar)d;
    return deepest;
}

size_t pngHuffFileBound(int W, int H)
{
    if (W < 1 || W > 65535 || H < 1 || H > 65535)
        return 0;
    const uint64_t headerBits = 3 + 5 + 5 + 4 + 19 * 3 + 258 * 7, container = 8 + 25 + 12 + 2 + 4 + 12;
    const uint64_t v = container + (headerBits + 15 * ((uint64_t)H * ((uint64_t)W + 1) + 1) + 7) / 8;
    return v >= ((uint64_t)1 << 32) ? 0 : (size_t)v;
}

bool pngHuffEncode(const uchar *pixels, int W, int H, std::vector<uchar> &out)
{
    out.clear();
    const size_t bound = pngHuffFileBound(W, H);
    if (!pixels || !bound)
        return false;
    // ---- the filtered bytes' counts and Adler-32 ---------------------------------------------------------------------
    uint64_t counts[257] = {0};
    std::vector<uchar> line((size_t)W + 1);
    uLong adler = adler32(0L, Z_NULL, 0);
    line[0] = 1;
    for (int y = 0; y < H; ++y) {
        const uchar *row = pixels + (size_t)y * W;
        line[1] = row[0];
        for (int x = 1; x < W; ++x)
            line[x + 1] = (uchar)(row[x] - row[x - 1]);
        for (int x = 0; x <= W; ++x)
            ++counts[line[x]];
        adler = adler32(adler, line.data(), (uInt)line.size());
    }
    counts[256] = 1;
    // ---- the two codes ----------------------------------------------------------------------------------------------
    uchar len[258], clLen[19];
    uint32_t code[257], clCode[19];
    if (pngHuffLengths(counts, 257, 15, len) < 0)
        return false;
    len[257] = 0; // the one distance length
    uint64_t clCounts[19] = {0};
    for (int i = 0; i < 258; ++i)
        ++clCounts[len[i]];
    if (pngHuffLengths(clCounts, 19, 7, clLen) < 0)
        return false;
    canonicalCodes(len, 257, code);
    canonicalCodes(clLen, 19, clCode);
    // ---- the file ---------------------------------------------------------------------------------------------------
    out.reserve(bound);
    static const uchar sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    out.insert(out.end(), sig, sig + 8);
    uchar ihdr[25] = {0, 0, 0, 13, 'I', 'H', 'D', 'R'};
    be32(ihdr + 8, (uint32_t)W);
    be32(ihdr + 12, (uint32_t)H);
    ihdr[16] = 8; // bit depth; colour type, compression, filter method, interlace: 0
    be32(ihdr + 21, (uint32_t)crc32(0L, ihdr + 4, 17));
    out.insert(out.end(), ihdr, ihdr + 25);
    const size_t idat = out.size();
    static const uchar idatHead[10] = {0, 0, 0, 0, 'I', 'D', 'A', 'T', 0x78, 0x01};
    out.insert(out.end(), idatHead, idatHead + 10);
    BitWriter bw{out};
    bw.put(1, 1);  // BFINAL
    bw.put(2, 2);  // BTYPE: dynamic Huffman
    bw.put(0, 5);  // HLIT: 257 codes
    bw.put(0, 5);  // HDIST: 1 code
    bw.put(15, 4); // HCLEN: 19 lengths
    for (int i = 0; i < 19; ++i)
        bw.put(clLen[kClOrder[i]], 3);
    for (int i = 0; i < 258; ++i)
        bw.put(clCode[len[i]], clLen[len[i]]);
    for (int y = 0; y < H; ++y) {
        const uchar *row = pixels + (size_t)y * W;
        bw.put(code[1], len[1]);
        bw.put(code[row[0]], len[row[0]]);
        for (int x = 1; x < W; ++x) {
            const uchar d = (uchar)(row[x] - row[x - 1]);
            bw.put(code[d], len[d]);
        }
    }
    bw.put(code[256], len[256]);
    bw.flush();
    uchar tail[4];
    be32(tail, (uint32_t)adler);
    out.insert(out.end(), tail, tail + 4);
    const size_t dataLen = out.size() - idat - 8;
    be32(&out[idat], (uint32_t)dataLen);
    be32(tail, (uint32_t)crc32(0L, &out[idat + 4], (uInt)(dataLen + 4)));
    out.insert(out.end(), tail, tail + 4);
    static const uchar iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
    out.insert(out.end(), iend, iend + 12);
    return true;
}

} // namespace cv
#endif
