// abub_crc.hpp -- the CRC-32 of zip and PNG (IEEE, reflected, polynomial 0xEDB88320) as the kernels compute it: the
// slice-by-4 tables, the carry-less multiplication modulo the polynomial and the powers x^(8 * 2^k) with which a register is
// moved over the bytes behind it.  One copy for k_zip_crc (abub_png.hip) and the archive packer (abub_zip_pack.hip); each
// translation unit that includes it gets its own tables.
#ifndef ABUB_CRC_HPP
#define ABUB_CRC_HPP

#include "abub_dev.hpp"

namespace {

constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr uint32_t crc_mul(uint32_t a, uint32_t b) // a * b mod P (bit 31 is x^0)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i))
            p ^= b;
        b = (b >> 1) ^ ((b & 1) ? CRC_POLY : 0u);
    }
    return p;
}
struct CrcTables {
    uint32_t t[4][256];
    uint32_t pw[32]; // x^(8 * 2^k) mod P
};
constexpr CrcTables crc_make_tables()
{
    CrcTables T{};
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k)
            c = (c >> 1) ^ ((c & 1) ? CRC_POLY : 0u);
        T.t[0][i] = c;
    }
    for (int s = 1; s < 4; ++s)
        for (uint32_t i = 0; i < 256; ++i)
            T.t[s][i] = (T.t[s - 1][i] >> 8) ^ T.t[0][T.t[s - 1][i] & 255];
    T.pw[0] = 0x00800000u; // x^8
    for (int k = 1; k < 32; ++k)
        T.pw[k] = crc_mul(T.pw[k - 1], T.pw[k - 1]);
    return T;
}
__device__ const CrcTables crc_tables = crc_make_tables();

// r moved over `nbytes` bytes of zeros: r * x^(8 * nbytes) mod P, one 32-step multiplication per set bit of nbytes
__device__ __forceinline__ uint32_t crc_shift(uint32_t r, uint32_t nbytes)
{
    if (r)
        for (int b = 0; b < 32 && (nbytes >> b); ++b)
            if ((nbytes >> b) & 1)
                r = crc_mul(r, crc_tables.pw[b]);
    return r;
}

} // namespace
#endif
