// abub_png_enc.hip -- canonical Huffman-only PNG files written on the GPU: abub_png_encode_dev (include/abub_hip.h, DESIGN
// section 3, "Unpacking a run").  It writes the bytes cv::pngHuffEncode (host/pnghuff.cpp) writes: Sub filter on every row,
// one dynamic-Huffman deflate block of literals, the code lengths by the format's rule.
//
// A wave owns a row, its lanes are 64 consecutive symbols of it (the filter byte, then the pixels' differences).  Where a
// row's bits lie depends on the code, the code on the histogram of the whole frame, a file's place on the files in front
// of it, and the IDAT's CRC on every byte of it, so the work is cut at each of these and every cut is a kernel boundary:
// no workgroup ever waits for another one inside a launch.
//   (clear)      the frames' histograms, a memset on the stream
//   histogram    one wave per row: 257 bins per workgroup in LDS, one global atomic add per non-empty bin; the row's Adler
//                partials A = sum d, B = sum (n - i) d, both mod 65521
//   codes        one wave per frame: code lengths (limit 15), canonical codes, the code-length code (limit 7), the header bits
//   measure      one wave per row: the sum of its symbols' lengths
//   place rows   one workgroup per frame: row bit counts -> 64-bit bit offsets behind the header; file length; Adler-32
//   place files  one workgroup: file lengths -> off, status, *total (k_enc_place_files, abub_enc.hpp: the ABF encoder's)
//   write        one wave per row: the bits; row 0 also the container's head and the header bits, the last row the tail
//   crc          one lane per 1 KiB segment of "IDAT" + data, table driven (the table is built in LDS)
//   fold         one lane per frame: crc = mulmod(crc, x^(8 len)) ^ crc_seg over the segments in order
// Row seams.  Rows are not byte aligned, and at W = 1 several rows share a byte.  Every byte of the deflate data has one
// owner: the row in which the byte's first bit lies.  The owner's wave also encodes the 7 symbols behind its row (they
// may belong to several rows, or be the end-of-block code), which is enough to finish its last byte; it skips the byte
// its row starts in the middle of.  So every output byte is stored once, by one lane, with a plain store: nothing is
// cleared beforehand, no global atomic touches `out`, and `out` is read (by crc) only where write has stored.
//
// Bounds.  A frame is read only when src + W * H <= pixels_bytes.  A file is written only when off + len <= out_cap; within
// it every store of the deflate data is checked against the byte count place rows derived (the lengths are clamped to 15
// where they are read, so the counts bound the positions whatever the scratch holds).  Every loop bound is a function of
// W, H and nframes, or a constant.
#include "abub_enc.hpp"

namespace {

#define PNGE_WAVES 4          /* waves per block of histogram and measure, a row each at a time */
#define PNGE_ROWS_PER_WAVE 8  /* rows a wave handles, where the frame has that many */
#define PNGE_WRITE_ROWS 8     /* rows a (one wave) block of write handles */
#define PNGE_SEG 1024u        /* bytes per CRC segment */
#define PNGE_TAB 260          /* words per frame of the histogram and of the code table (257 used; [257] = header bits) */
#define PNGE_HDR_WORDS 60     /* 3 + 14 + 57 + 258 * 7 = 1880 header bits at the most */
#define PNGE_BUF_WORDS 68     /* 7 carried bits + 64 lanes * 32 bits, and a word to spill into */
#define PNGE_HEAD 43u         /* signature 8, IHDR 25, IDAT length and type 8, zlib header 2 */
#define PNGE_FIXED 63u        /* PNGE_HEAD + Adler-32 4 + IDAT CRC 4 + IEND 12 */
#define PNGE_MOD 65521u
#define PNGE_POLY 0xedb88320u

struct PngeRow {
    uint64_t bit;  // measure: the row's bit count; place rows: where its bits start, from the first bit of the deflate block
    uint32_t A, B; // Adler partials of the row's W + 1 filtered bytes
};
struct PngeFrame {
    uint32_t flen;   // the file's length (0 for a frame that is not read)
    uint32_t adler;
    uint64_t nbytes; // of the deflate block
};

// symbol c0 + lane of a row (W + 1 symbols: the filter byte 1, the first pixel, the differences to the left neighbour)
__device__ __forceinline__ uint32_t pnge_row_symbol(const uint8_t *__restrict__ row, int W, int c0, int lane, bool &valid)
{
    const int c = c0 + lane;
    valid = c <= W;
    const uint32_t q = (c >= 1 && c <= W) ? (uint32_t)row[c - 1] : 0u;
    uint32_t prev = enc_left_neighbour(q);
    if (lane == 0)
        prev = (c >= 2 && c <= W) ? (uint32_t)row[c - 2] : 0u;
    return c == 0 ? 1u : (q - prev) & 0xffu;
}

// symbol i of the frame's H * (W + 1) symbols, by itself
__device__ __forceinline__ uint32_t pnge_symbol_at(const uint8_t *__restrict__ img, int W, uint64_t i)
{
    const uint32_t n = (uint32_t)W + 1u;
    const uint32_t y = (uint32_t)(i / n), c = (uint32_t)(i - (uint64_t)y * n);
    if (c == 0)
        return 1u;
    const uint8_t *row = img + (uint64_t)y * (uint32_t)W;
    return c == 1 ? (uint32_t)row[0] : ((uint32_t)row[c - 1] - (uint32_t)row[c - 2]) & 0xffu;
}

__global__ __launch_bounds__(64 * PNGE_WAVES) void k_png_enc_hist(const uint8_t *__restrict__ pixels, uint64_t pixels_bytes,
                                                                  const uint64_t *__restrict__ src, int W, int H,
                                                                  uint32_t *__restrict__ hist, PngeRow *__restrict__ rows)
{
    __shared__ uint32_t sh[257];
    const uint32_t f = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t P = (uint64_t)W * (uint64_t)H, s = src[f];
    if (!frame_in_range(s, pixels_bytes, P))
        return; // (the same in every thread; nobody reads this frame's scratch)
    for (int b = threadIdx.x; b < 257; b += 64 * PNGE_WAVES)
        sh[b] = 0;
    __syncthreads();
    const uint8_t *img = pixels + s;
    PngeRow *frows = rows + (uint64_t)f * (uint32_t)H;
    const uint32_t n = (uint32_t)W + 1u;
    for (int y = (int)blockIdx.y * PNGE_WAVES + wv; y < H; y += (int)gridDim.y * PNGE_WAVES) {
        const uint8_t *row = img + (uint64_t)y * (uint32_t)W;
        uint32_t A = 0, B = 0; // (A: at most 1024 terms of 255 per lane; B: reduced every term, each below 2^24)
        for (int c0 = 0; c0 <= W; c0 += 64) {
            bool valid;
            const uint32_t d = pnge_row_symbol(row, W, c0, lane, valid);
            if (valid) {
                atomicAdd(&sh[d], 1u);
                A += d;
                B = (B + ((n - (uint32_t)(c0 + lane)) % PNGE_MOD) * d) % PNGE_MOD;
            }
        }
        A = wave_sum(A % PNGE_MOD);
        B = wave_sum(B);
        if (lane == 0) {
            frows[y].A = A % PNGE_MOD;
            frows[y].B = B % PNGE_MOD;
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < 257; b += 64 * PNGE_WAVES)
        if (sh[b])
            atomicAdd(&hist[(uint64_t)f * PNGE_TAB + b], sh[b]);
}

// The format's code lengths of cnt[0 .. n) (n <= 257, at least two nonzero, their sum below 2^32) under `limit`; every
// lane of the one wave calls it.  Work arrays in LDS: ordA, ordD [n]; weight, parent [2 n].
__device__ void pnge_lengths(const uint32_t *cnt, int n, int limit, uint8_t *len, uint16_t *ordA, uint16_t *ordD, uint32_t *weight,
                             uint16_t *parent)
{
    const int lane = threadIdx.x;
    // the used symbols ascending by (count, symbol), and by (count descending, symbol): every symbol finds its two ranks
    for (int s = lane; s < n; s += 64) {
        len[s] = 0;
        const uint32_t c = cnt[s];
        if (!c)
            continue;
        int ra = 0, rd = 0;
        for (int t = 0; t < n; ++t) {
            const uint32_t ct = cnt[t];
            if (!ct || t == s)
                continue;
            ra += ct < c || (ct == c && t < s);
            rd += ct > c || (ct == c && t < s);
        }
        ordA[ra] = (uint16_t)s;
        ordD[rd] = (uint16_t)s;
    }
    __syncthreads();
    if (lane == 0) {
        int m = 0;
        for (int s = 0; s < n; ++s)
            m += cnt[s] != 0u;
        if (m >= 2) {
            for (int i = 0; i < m; ++i)
                weight[i] = cnt[ordA[i]];
            // two queues: the leaves in order, the internal nodes as they are made; the leaf first on equal weight
            int leaf = 0, inner = m;
            for (int node = m; node < 2 * m - 1; ++node) {
                uint32_t w = 0;
                for (int k = 0; k < 2; ++k) {
                    const int take = leaf < m && (inner >= node || weight[leaf] <= weight[inner]) ? leaf++ : inner++;
                    parent[take] = (uint16_t)node;
                    w += weight[take];
                }
                weight[node] = w;
            }
            // depths, from the root down (weight is free now: it takes them)
            weight[2 * m - 2] = 0;
            for (int i = 2 * m - 3; i >= 0; --i)
                weight[i] = weight[parent[i]] + 1u;
            int per[16];
            for (int d = 0; d < 16; ++d)
                per[d] = 0;
            for (int i = 0; i < m; ++i)
                ++per[min((int)weight[i], limit)];
            uint32_t kraft = 0; // in units of 2^-limit (m <= 257 codes of at most 2^15 units)
            for (int d = 1; d <= limit; ++d)
                kraft += (uint32_t)per[d] << (limit - d);
            for (; kraft > (1u << limit); --kraft) {
                int d = limit - 1;
                while (d > 0 && !per[d])
                    --d;
                if (d == 0)
                    break; // (cannot happen: m <= 2^limit)
                --per[limit];
                --per[d];
                per[d + 1] += 2;
            }
            int at = 0;
            for (int d = 1; d <= limit; ++d)
                for (int k = 0; k < per[d] && at < m; ++k)
                    len[ordD[at++]] = (uint8_t)d;
        }
    }
    __syncthreads();
}

// RFC 1951 3.2.2 with every code reversed (the bit stream is filled from the least significant bit); lane 0 calls it
__device__ void pnge_canonical(const uint8_t *len, int n, uint32_t *code)
{
    uint32_t count[16], next[16];
    for (int b = 0; b < 16; ++b)
        count[b] = 0;
    for (int s = 0; s < n; ++s)
        ++count[len[s] & 15];
    count[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (int b = 1; b < 16; ++b)
        next[b] = c = (c + count[b - 1]) << 1;
    for (int s = 0; s < n; ++s) {
        const uint32_t l = len[s] & 15u;
        code[s] = l ? (__brev(next[l]++) >> (32u - l)) | l << 16 : 0u;
    }
}

// codes[f * PNGE_TAB + s] = reversed code | length << 16 of symbol s <= 256; [257] = the header's bit count;
// hdr[f * PNGE_HDR_WORDS ..] = the header bits (BFINAL ... the 258 lengths), zero behind them
__global__ __launch_bounds__(64) void k_png_enc_codes(uint64_t pixels_bytes, const uint64_t *__restrict__ src, int W, int H,
                                                      const uint32_t *__restrict__ hist, uint32_t *__restrict__ codes,
                                                      uint32_t *__restrict__ hdr)
{
    __shared__ uint32_t cnt[257], code[257], weight[2 * 257], hbits[PNGE_HDR_WORDS], clcnt[19], clcode[19];
    __shared__ uint16_t ordA[257], ordD[257], parent[2 * 257];
    __shared__ uint8_t len[258], cllen[19];
    const uint32_t f = blockIdx.x;
    const int lane = threadIdx.x;
    if (!frame_in_range(src[f], pixels_bytes, (uint64_t)W * (uint64_t)H))
        return;
    for (int s = lane; s < 257; s += 64)
        cnt[s] = s == 256 ? 1u : hist[(uint64_t)f * PNGE_TAB + s];
    for (int s = lane; s < PNGE_HDR_WORDS; s += 64)
        hbits[s] = 0;
    __syncthreads();
    pnge_lengths(cnt, 257, 15, len, ordA, ordD, weight, parent);
    if (lane == 0) {
        len[257] = 0; // the one distance length
        for (int s = 0; s < 19; ++s)
            clcnt[s] = 0;
        for (int s = 0; s < 258; ++s)
            ++clcnt[len[s] & 15];
    }
    __syncthreads();
    pnge_lengths(clcnt, 19, 7, cllen, ordA, ordD, weight, parent);
    uint32_t nbits = 0;
    if (lane == 0) {
        pnge_canonical(len, 257, code);
        pnge_canonical(cllen, 19, clcode);
        auto put = [&](uint32_t v, uint32_t n) { // (n <= 7; the words are zero)
            if (n && (nbits + n) <= 32u * PNGE_HDR_WORDS) {
                hbits[nbits >> 5] |= v << (nbits & 31u);
                if ((nbits & 31u) + n > 32u)
                    hbits[(nbits >> 5) + 1u] |= v >> (32u - (nbits & 31u));
                nbits += n;
            }
        };
        put(1u, 1);  // BFINAL
        put(2u, 2);  // BTYPE: dynamic Huffman
        put(0u, 5);  // HLIT: 257 codes
        put(0u, 5);  // HDIST: 1 code
        put(15u, 4); // HCLEN: 19 lengths
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        for (int i = 0; i < 19; ++i)
            put(cllen[order[i]] & 7u, 3);
        for (int s = 0; s < 258; ++s) {
            const uint32_t e = clcode[len[s] & 15];
            put(e & 0xffffu, e >> 16);
        }
    }
    __syncthreads();
    nbits = (uint32_t)__shfl((int)nbits, 0);
    for (int s = lane; s < 257; s += 64)
        codes[(uint64_t)f * PNGE_TAB + s] = code[s];
    if (lane == 0)
        codes[(uint64_t)f * PNGE_TAB + 257] = nbits;
    for (int s = lane; s < PNGE_HDR_WORDS; s += 64)
        hdr[(uint64_t)f * PNGE_HDR_WORDS + s] = hbits[s];
}

// rows[f * H + y].bit = the bits of row y's W + 1 symbols
__global__ __launch_bounds__(64 * PNGE_WAVES) void k_png_enc_measure(const uint8_t *__restrict__ pixels, uint64_t pixels_bytes,
                                                                     const uint64_t *__restrict__ src, int W, int H,
                                                                     const uint32_t *__restrict__ codes, PngeRow *__restrict__ rows)
{
    __shared__ uint8_t len[257];
    const uint32_t f = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t P = (uint64_t)W * (uint64_t)H, s = src[f];
    if (!frame_in_range(s, pixels_bytes, P))
        return;
    for (int b = threadIdx.x; b < 257; b += 64 * PNGE_WAVES)
        len[b] = (uint8_t)min(codes[(uint64_t)f * PNGE_TAB + b] >> 16, 15u);
    __syncthreads();
    const uint8_t *img = pixels + s;
    PngeRow *frows = rows + (uint64_t)f * (uint32_t)H;
    for (int y = (int)blockIdx.y * PNGE_WAVES + wv; y < H; y += (int)gridDim.y * PNGE_WAVES) {
        const uint8_t *row = img + (uint64_t)y * (uint32_t)W;
        uint32_t bits = 0; // (at most 65536 * 15)
        for (int c0 = 0; c0 <= W; c0 += 64) {
            bool valid;
            const uint32_t d = pnge_row_symbol(row, W, c0, lane, valid);
            bits += valid ? (uint32_t)len[d] : 0u;
        }
        bits = wave_sum(bits);
        if (lane == 0)
            frows[y].bit = bits;
    }
}

// rows[f * H + y].bit: count -> offset; info[f] = file length, Adler-32, bytes of the deflate block
__global__ __launch_bounds__(ENC_SCAN) void k_png_enc_place_rows(uint64_t pixels_bytes, const uint64_t *__restrict__ src, int W,
                                                                   int H, const uint32_t *__restrict__ codes,
                                                                   PngeRow *__restrict__ rows, PngeFrame *__restrict__ info)
{
    __shared__ unsigned long long sh64[ENC_SCAN / 64];
    __shared__ uint32_t sh32[ENC_SCAN / 64];
    const uint32_t f = blockIdx.x;
    if (!frame_in_range(src[f], pixels_bytes, (uint64_t)W * (uint64_t)H)) { // (the same answer in every thread)
        if (threadIdx.x == 0) {
            PngeFrame z;
            z.flen = 0;
            z.adler = 0;
            z.nbytes = 0;
            info[f] = z;
        }
        return;
    }
    const uint32_t *tab = codes + (uint64_t)f * PNGE_TAB;
    PngeRow *frows = rows + (uint64_t)f * (uint32_t)H;
    const uint32_t nmod = ((uint32_t)W + 1u) % PNGE_MOD;
    unsigned long long base = min(tab[257], 32u * PNGE_HDR_WORDS); // the rows start behind the header bits
    uint32_t a = 1, b = 0;                                          // Adler-32 in front of the rows of this round
    for (int y0 = 0; y0 < H; y0 += ENC_SCAN) {
        const int y = y0 + (int)threadIdx.x;
        PngeRow r;
        r.bit = 0;
        r.A = r.B = 0;
        if (y < H)
            r = frows[y];
        unsigned long long all;
        const unsigned long long incl = enc_block_scan((unsigned long long)r.bit, sh64, all);
        if (y < H)
            frows[y].bit = base + incl - r.bit;
        base += all;
        // a row of n bytes takes (a, b) to (a + A, b + n a + B): a in front of each row by a scan, b by a sum
        uint32_t allA, allT;
        const uint32_t inclA = enc_block_scan(r.A, sh32, allA); // (256 values below 65521)
        const uint32_t a0 = (a + inclA - r.A) % PNGE_MOD;
        const uint32_t term = y < H ? (uint32_t)(((unsigned long long)nmod * a0 + r.B) % PNGE_MOD) : 0u;
        enc_block_scan(term, sh32, allT);
        a = (a + allA) % PNGE_MOD;
        b = (b + allT) % PNGE_MOD;
    }
    if (threadIdx.x == 0) {
        const unsigned long long bits = base + min(tab[256] >> 16, 15u); // (the end-of-block code)
        PngeFrame z;
        z.nbytes = (bits + 7ull) >> 3;
        z.flen = (uint32_t)(PNGE_FIXED + z.nbytes); // (below 2^32: abub_png_file_bound)
        z.adler = b << 16 | a;
        info[f] = z;
    }
}

// The bit writer of one wave (a block of 64 threads): lanes hand in up to 32 bits each, in lane order; whole bytes go
// out with plain stores, the rest is carried.  A byte is stored only when its first bit lies in [ownStart, ownEnd).
struct PngeBits {
    uint64_t cur;               // bits handed in so far, counted from the first bit of the deflate block
    uint64_t ownStart, ownEnd;
    uint64_t nbytes;            // of the deflate block: nothing is stored at or behind it
    uint8_t *data;              // the deflate block
    uint32_t *buf;              // PNGE_BUF_WORDS words of LDS, zero but for the carried bits
};
__device__ __forceinline__ void pnge_store_byte(const PngeBits &s, uint64_t B, uint32_t v)
{
    if (8ull * B >= s.ownStart && 8ull * B < s.ownEnd && B < s.nbytes)
        s.data[B] = (uint8_t)v;
}
__device__ __forceinline__ void pnge_emit(PngeBits &s, uint32_t val, uint32_t len)
{
    const int lane = threadIdx.x;
    uint32_t incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o);
        if (lane >= o)
            incl += t;
    }
    const uint32_t sum = (uint32_t)__shfl((int)incl, 63);
    const uint32_t pos = (uint32_t)(s.cur & 7u) + incl - len;
    if (len) {
        atomicOr(&s.buf[pos >> 5], val << (pos & 31u));
        if ((pos & 31u) + len > 32u)
            atomicOr(&s.buf[(pos >> 5) + 1u], val >> (32u - (pos & 31u)));
    }
    __syncthreads();
    const uint32_t have = (uint32_t)(s.cur & 7u) + sum, nfull = have >> 3; // (at most 7 + 2048 bits)
    const uint64_t B0 = s.cur >> 3;
    for (uint32_t j = lane; j < nfull; j += 64)
        pnge_store_byte(s, B0 + j, (s.buf[j >> 2] >> (8u * (j & 3u))) & 0xffu);
    const uint32_t carry = (s.buf[nfull >> 2] >> (8u * (nfull & 3u))) & 0xffu;
    __syncthreads();
    for (int j = lane; j < PNGE_BUF_WORDS; j += 64)
        s.buf[j] = j == 0 ? carry : 0u;
    __syncthreads();
    s.cur += sum;
}

__global__ __launch_bounds__(64) void k_png_enc_write(const uint8_t *__restrict__ pixels, const uint64_t *__restrict__ src, int W,
                                                      int H, const PngeRow *__restrict__ rows, const PngeFrame *__restrict__ info,
                                                      const uint32_t *__restrict__ codes, const uint32_t *__restrict__ hdr,
                                                      const abub_abf_file *__restrict__ files, uint32_t crcIhdr,
                                                      uint8_t *__restrict__ out)
{
    __shared__ uint32_t tab[257], buf[PNGE_BUF_WORDS];
    const uint32_t f = blockIdx.x;
    const int lane = threadIdx.x;
    const abub_abf_file rec = files[f];
    if (rec.status != 0)
        return; // (E_SRC: nothing to read; E_CAP: no room: none of the file's bytes is written)
    const PngeFrame fi = info[f];
    if ((uint64_t)rec.len != PNGE_FIXED + fi.nbytes)
        return; // (cannot happen: place files copied the length from there)
    for (int b = lane; b < 257; b += 64) {
        const uint32_t e = codes[(uint64_t)f * PNGE_TAB + b];
        tab[b] = (e & 0x7fffu) | min(e >> 16, 15u) << 16;
    }
    for (int j = lane; j < PNGE_BUF_WORDS; j += 64)
        buf[j] = 0;
    __syncthreads();
    const uint32_t hbits = min(codes[(uint64_t)f * PNGE_TAB + 257], 32u * PNGE_HDR_WORDS);
    const uint8_t *img = pixels + src[f];
    const PngeRow *frows = rows + (uint64_t)f * (uint32_t)H;
    uint8_t *file = out + rec.off;
    const uint64_t nsym = (uint64_t)H * ((uint64_t)W + 1u);
    const uint32_t dataLen = (uint32_t)(fi.nbytes + 6u);

    const int yEnd = min(H, ((int)blockIdx.y + 1) * PNGE_WRITE_ROWS);
    for (int y = (int)blockIdx.y * PNGE_WRITE_ROWS; y < yEnd; ++y) {
        PngeBits s;
        s.cur = y == 0 ? 0ull : frows[y].bit;
        s.ownStart = s.cur;
        s.ownEnd = y == H - 1 ? ~0ull : frows[y + 1].bit;
        s.nbytes = fi.nbytes;
        s.data = file + PNGE_HEAD;
        s.buf = buf;
        if (y == 0) {
            // the container in front of the deflate block
            if (lane < (int)PNGE_HEAD) {
                const uint32_t at = (uint32_t)lane;
                uint32_t v;
                if (at < 8u)
                    v = (uint32_t)(0x0a1a0a0d474e5089ull >> (8u * at));
                else if (at < 12u)
                    v = at == 11u ? 13u : 0u;
                else if (at < 16u)
                    v = 0x52444849u >> (8u * (at - 12u)); // "IHDR"
                else if (at < 20u)
                    v = (uint32_t)W >> (8u * (19u - at));
                else if (at < 24u)
                    v = (uint32_t)H >> (8u * (23u - at));
                else if (at < 29u)
                    v = at == 24u ? 8u : 0u;
                else if (at < 33u)
                    v = crcIhdr >> (8u * (32u - at));
                else if (at < 37u)
                    v = dataLen >> (8u * (36u - at));
                else if (at < 41u)
                    v = 0x54414449u >> (8u * (at - 37u)); // "IDAT"
                else
                    v = at == 41u ? 0x78u : 0x01u;
                file[at] = (uint8_t)v;
            }
            const uint32_t w = (uint32_t)lane;
            const uint32_t n = 32u * w < hbits ? min(32u, hbits - 32u * w) : 0u;
            pnge_emit(s, n ? hdr[(uint64_t)f * PNGE_HDR_WORDS + w] & (n == 32u ? ~0u : (1u << n) - 1u) : 0u, n);
        }
        const uint8_t *row = img + (uint64_t)y * (uint32_t)W;
        for (int c0 = 0; c0 <= W; c0 += 64) {
            bool valid;
            const uint32_t d = pnge_row_symbol(row, W, c0, lane, valid);
            const uint32_t e = tab[d];
            pnge_emit(s, e & 0xffffu, valid ? e >> 16 : 0u);
        }
        // the 7 symbols behind the row finish the last byte this row owns; behind the last symbol comes the end-of-block code
        {
            const uint64_t i = (uint64_t)(y + 1) * ((uint64_t)W + 1u) + (uint64_t)lane;
            uint32_t e = 0;
            if (lane < 7 && i <= nsym)
                e = tab[i == nsym ? 256u : pnge_symbol_at(img, W, i)];
            pnge_emit(s, e & 0xffffu, e >> 16);
        }
        // what is left is the block's last byte, zero bits behind the end-of-block code (stored if this row owns it)
        if ((s.cur & 7u) && lane == 0)
            pnge_store_byte(s, s.cur >> 3, buf[0] & 0xffu);
        __syncthreads();
        if (lane == 0)
            buf[0] = 0;
        __syncthreads();
        if (y == H - 1) {
            uint8_t *tail = file + PNGE_HEAD + fi.nbytes; // Adler-32, (the IDAT's CRC: k_png_enc_fold), IEND
            if (lane < 4)
                tail[lane] = (uint8_t)(fi.adler >> (8 * (3 - lane)));
            else if (lane >= 8 && lane < 20) {
                const uint64_t lo = 0x444e454900000000ull; // 0, 0, 0, 0, "IEND"
                const uint32_t hi = 0x826042aeu;           // its CRC, ae 42 60 82
                const int k = lane - 8;
                tail[lane] = (uint8_t)(k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8)));
            }
        }
    }
}

// seg[f * nsegMax + g] = CRC-32 of bytes [g * PNGE_SEG, ...) of the file's "IDAT" + data
__global__ __launch_bounds__(256) void k_png_enc_crc(const PngeFrame *__restrict__ info, const abub_abf_file *__restrict__ files,
                                                     const uint8_t *__restrict__ out, uint32_t nsegMax, uint32_t *__restrict__ seg)
{
    __shared__ uint32_t table[256];
    {
        uint32_t c = threadIdx.x;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            c = (c >> 1) ^ ((c & 1u) ? PNGE_POLY : 0u);
        table[threadIdx.x] = c;
    }
    __syncthreads();
    const uint32_t f = blockIdx.x;
    const abub_abf_file rec = files[f];
    if (rec.status != 0)
        return;
    const uint64_t L = info[f].nbytes + 10u; // type 4, zlib header 2, the block, Adler-32 4
    if (PNGE_FIXED - 10u + L != (uint64_t)rec.len)
        return; // (cannot happen)
    const uint32_t g = blockIdx.y * 256u + threadIdx.x;
    const uint64_t from = (uint64_t)g * PNGE_SEG;
    if (g >= nsegMax || from >= L)
        return;
    const uint32_t n = (uint32_t)min((uint64_t)PNGE_SEG, L - from);
    const uint8_t *p = out + rec.off + 37u + from;
    uint32_t c = ~0u;
    for (uint32_t i = 0; i < n; ++i)
        c = table[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    seg[(uint64_t)f * nsegMax + g] = ~c;
}

// a * b mod the CRC polynomial, both in the CRC's reflected bit order (x^0 is bit 31)
__device__ __forceinline__ uint32_t pnge_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i))
            p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? PNGE_POLY : 0u);
    }
    return p;
}
// x^(8 n)
__device__ __forceinline__ uint32_t pnge_xpow8(uint32_t n)
{
    uint32_t r = 0x80000000u, base = 0x00800000u;
    for (; n; n >>= 1) {
        if (n & 1u)
            r = pnge_mulmod(r, base);
        base = pnge_mulmod(base, base);
    }
    return r;
}

// crc(A || B) = crc(A) * x^(8 |B|) ^ crc(B): the segments folded in order, the four bytes stored behind the data.
// Untuned: a lane computes x^(8 PNGE_SEG) for itself and folds its frame's segments one after the other, a 32-step
// bitwise mulmod each, so the launch costs O(segments x 32) dependent steps per frame (about 600 segments for a 1280 x
// 1024 frame; 0.41 ms of the encoder's 11.4 for 1024 of them).  A wave per frame folding pairs of segments in a tree, or
// larger segments, is where that time would go.
__global__ __launch_bounds__(64) void k_png_enc_fold(int nframes, const PngeFrame *__restrict__ info,
                                                     const abub_abf_file *__restrict__ files, uint32_t nsegMax,
                                                     const uint32_t *__restrict__ seg, uint8_t *__restrict__ out)
{
    const int f = (int)(blockIdx.x * 64u + threadIdx.x);
    if (f >= nframes)
        return;
    const abub_abf_file rec = files[f];
    if (rec.status != 0)
        return;
    const uint64_t L = info[f].nbytes + 10u;
    if (PNGE_FIXED - 10u + L != (uint64_t)rec.len)
        return; // (cannot happen)
    const uint32_t nseg = (uint32_t)min((uint64_t)nsegMax, (L + PNGE_SEG - 1u) / PNGE_SEG);
    const uint32_t *s = seg + (uint64_t)f * nsegMax;
    const uint32_t whole = pnge_xpow8(PNGE_SEG);
    uint32_t crc = s[0];
    for (uint32_t g = 1; g < nseg; ++g) {
        const uint64_t left = L - (uint64_t)g * PNGE_SEG;
        const uint32_t m = left >= PNGE_SEG ? whole : pnge_xpow8((uint32_t)left);
        crc = pnge_mulmod(m, crc) ^ s[g];
    }
    uint8_t *p = out + rec.off + 37u + L;
    p[0] = (uint8_t)(crc >> 24);
    p[1] = (uint8_t)(crc >> 16);
    p[2] = (uint8_t)(crc >> 8);
    p[3] = (uint8_t)crc;
}

inline size_t pnge_nseg_max(int W, int H) { return (abub_png_file_bound(W, H) - (PNGE_FIXED - 10u) + PNGE_SEG - 1u) / PNGE_SEG; }

// CRC-32 of a few bytes on the host (IHDR's depends on W and H only)
uint32_t host_crc32(const uint8_t *p, size_t n)
{
    uint32_t c = ~0u;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k)
            c = (c >> 1) ^ ((c & 1u) ? PNGE_POLY : 0u);
    }
    return ~c;
}

} // namespace

extern "C" size_t abub_png_file_bound(int W, int H)
{
    if (W < 1 || W > 65535 || H < 1 || H > 65535)
        return 0;
    const uint64_t v = PNGE_FIXED + (1880u + 15u * ((uint64_t)H * ((uint64_t)W + 1u) + 1u) + 7u) / 8u;
    return v >= ((uint64_t)1 << 32) ? 0 : (size_t)v;
}

// histograms, code tables, header bits, rows (16 bytes each), frame records, CRC segments: each part at a multiple of 16
extern "C" size_t abub_png_encode_scratch_bytes(int nframes, int W, int H)
{
    if (nframes < 0 || !abub_png_file_bound(W, H))
        return 0;
    const size_t n = (size_t)nframes;
    return 2 * align16z(n * PNGE_TAB * 4) + align16z(n * PNGE_HDR_WORDS * 4) + align16z(n * (size_t)H * sizeof(PngeRow)) +
           align16z(n * sizeof(PngeFrame)) + align16z(n * pnge_nseg_max(W, H) * 4) + 16;
}

extern "C" int abub_png_encode_dev(const uint8_t *pixels, size_t pixels_bytes, const uint64_t *src, int nframes, int W, int H,
                                   uint8_t *out, size_t out_cap, abub_abf_file *files, uint64_t *total, void *scratch,
                                   size_t scratch_bytes, void *stream)
{
    if (const int e = enc_check_args("abub_png_encode", abub_png_file_bound, abub_png_encode_scratch_bytes, pixels, src, nframes, W, H, out,
                                     files, total, scratch, scratch_bytes))
        return e;
    if (nframes == 0)
        return ABUB_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)nframes;
    const uint32_t nsegMax = (uint32_t)pnge_nseg_max(W, H);
    uint8_t *sc = (uint8_t *)scratch;
    uint32_t *hist = (uint32_t *)sc;
    sc += align16z(n * PNGE_TAB * 4);
    uint32_t *codes = (uint32_t *)sc;
    sc += align16z(n * PNGE_TAB * 4);
    uint32_t *hdr = (uint32_t *)sc;
    sc += align16z(n * PNGE_HDR_WORDS * 4);
    PngeRow *rows = (PngeRow *)sc;
    sc += align16z(n * (size_t)H * sizeof(PngeRow));
    PngeFrame *info = (PngeFrame *)sc;
    sc += align16z(n * sizeof(PngeFrame));
    uint32_t *seg = (uint32_t *)sc;
    uint8_t ihdr[17] = {'I', 'H', 'D', 'R', (uint8_t)(W >> 24), (uint8_t)(W >> 16), (uint8_t)(W >> 8), (uint8_t)W,
                        (uint8_t)(H >> 24), (uint8_t)(H >> 16), (uint8_t)(H >> 8), (uint8_t)H, 8, 0, 0, 0, 0};
    const uint32_t crcIhdr = host_crc32(ihdr, sizeof ihdr);

    const int perBlock = PNGE_WAVES * PNGE_ROWS_PER_WAVE;
    const dim3 grid((unsigned)nframes, (unsigned)((H + perBlock - 1) / perBlock));
    HIPCHK(hipMemsetAsync(hist, 0, n * PNGE_TAB * 4, st));
    k_png_enc_hist<<<grid, 64 * PNGE_WAVES, 0, st>>>(pixels, (uint64_t)pixels_bytes, src, W, H, hist, rows);
    HIPCHK(hipGetLastError());
    k_png_enc_codes<<<(unsigned)nframes, 64, 0, st>>>((uint64_t)pixels_bytes, src, W, H, hist, codes, hdr);
    HIPCHK(hipGetLastError());
    k_png_enc_measure<<<grid, 64 * PNGE_WAVES, 0, st>>>(pixels, (uint64_t)pixels_bytes, src, W, H, codes, rows);
    HIPCHK(hipGetLastError());
    k_png_enc_place_rows<<<(unsigned)nframes, ENC_SCAN, 0, st>>>((uint64_t)pixels_bytes, src, W, H, codes, rows, info);
    HIPCHK(hipGetLastError());
    k_enc_place_files<<<1, ENC_SCAN, 0, st>>>((uint64_t)pixels_bytes, src, nframes, (uint64_t)W * (uint64_t)H, &info->flen,
                                               (uint32_t)sizeof(PngeFrame), (uint64_t)out_cap, files, total);
    HIPCHK(hipGetLastError());
    const dim3 wgrid((unsigned)nframes, (unsigned)((H + PNGE_WRITE_ROWS - 1) / PNGE_WRITE_ROWS));
    k_png_enc_write<<<wgrid, 64, 0, st>>>(pixels, src, W, H, rows, info, codes, hdr, files, crcIhdr, out);
    HIPCHK(hipGetLastError());
    const dim3 cgrid((unsigned)nframes, (nsegMax + 255u) / 256u);
    k_png_enc_crc<<<cgrid, 256, 0, st>>>(info, files, out, nsegMax, seg);
    HIPCHK(hipGetLastError());
    k_png_enc_fold<<<(unsigned)((nframes + 63) / 64), 64, 0, st>>>(nframes, info, files, nsegMax, seg, out);
    HIPCHK(hipGetLastError());
    return ABUB_OK;
}
