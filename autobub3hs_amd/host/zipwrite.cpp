// zipwrite.cpp -- the host writer of the canonical archive (zipwrite.hpp): it is the definition of the bytes that
// abub_zip_pack_dev and tests/zipref.py restate.
#include "zipwrite.hpp"

#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include <unistd.h>
#include <zlib.h>

namespace abub {

namespace {

inline void put16(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
}
inline void put32(uint8_t *p, uint32_t v)
{
    put16(p, v);
    put16(p + 2, v >> 16);
}
inline void put64(uint8_t *p, uint64_t v)
{
    put32(p, (uint32_t)v);
    put32(p + 4, (uint32_t)(v >> 32));
}
// what the local header and the central record share, 26 bytes from "version needed" to the length of the extra field
// (whose value the caller sets)
void putCommon(uint8_t *p, unsigned versionNeeded, const ZipWriter::Entry &e)
{
    put16(p, versionNeeded);
    put16(p + 2, 0);       // flags
    put16(p + 4, 0);       // method: stored
    put16(p + 6, 0);       // time
    put16(p + 8, 0x0021);  // date: 1980-01-01
    put32(p + 10, e.crc);
    put32(p + 14, e.at.len);
    put32(p + 18, e.at.len);
    put16(p + 22, e.at.nameLen);
}

} // namespace

std::string zipPathOf(const std::string &folder)
{
    std::string p = folder;
    while (p.size() > 1 && p.back() == '/')
        p.pop_back();
    const size_t slash = p.find_last_of('/'), dot = p.find_last_of('.');
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash))
        p += ".zip";
    return p;
}

ZipWriter::ZipWriter(const std::string &path) : path_(path), part_(path + ".part")
{
    const char *f = getenv("ABUB_ZIP64_FORCE");
    force64_ = f && atoi(f) != 0;
    fp_ = fopen(part_.c_str(), "wb");
    if (!fp_)
        throw std::runtime_error("cannot write " + part_ + ": " + strerror(errno));
}

ZipWriter::~ZipWriter()
{
    if (fp_) { // not finished
        fclose(fp_);
        remove(part_.c_str());
    }
}

size_t ZipWriter::plan(const std::string &name, uint64_t len)
{
    if (name.size() > 65535 || len >= 0xffffffffull)
        throw std::runtime_error("archive entry " + name + ": the name or the file is too long for a zip entry");
    Entry e;
    e.name = name;
    e.at = zipLayout(planned_, name.size(), len);
    planned_ = e.at.end();
    entries_.push_back(std::move(e));
    return entries_.size() - 1;
}

void ZipWriter::putHead(size_t i, uint8_t *dst) const
{
    const Entry &e = entries_[i];
    put32(dst, 0x04034b50u);
    putCommon(dst + 4, 20, e);
    put16(dst + 28, e.at.extraLen);
    std::memcpy(dst + 30, e.name.data(), e.name.size());
    if (e.at.extraLen) {
        uint8_t *x = dst + 30 + e.name.size();
        std::memset(x, 0, e.at.extraLen);
        put16(x, 0x4241);
        put16(x + 2, e.at.extraLen - 4u);
    }
}

void ZipWriter::putEntry(size_t i, const uint8_t *data, uint8_t *dst)
{
    Entry &e = entries_[i];
    e.crc = e.at.len ? (uint32_t)crc32(crc32(0L, Z_NULL, 0), data, e.at.len) : 0u;
    putHead(i, dst);
    if (e.at.len)
        std::memcpy(dst + e.at.head(), data, e.at.len);
}

void ZipWriter::write(const uint8_t *bytes, size_t n)
{
    if (!fp_ || written_ + n > planned_)
        throw std::runtime_error("archive " + path_ + ": bytes written out of turn");
    if (n && fwrite(bytes, 1, n, fp_) != n)
        throw std::runtime_error("cannot write " + part_ + ": " + strerror(errno));
    written_ += n;
}

void ZipWriter::add(const std::string &name, const uint8_t *data, size_t len)
{
    const size_t i = plan(name, len);
    std::vector<uint8_t> whole(entries_[i].at.end() - entries_[i].at.off);
    putEntry(i, data, whole.data());
    write(whole.data(), whole.size());
}

void ZipWriter::finish()
{
    if (!fp_ || written_ != planned_)
        throw std::runtime_error("archive " + path_ + ": finished before all of its entries were written");
    const uint64_t cdOff = written_, count = entries_.size();
    std::vector<uint8_t> cd;
    for (const Entry &e : entries_) {
        const bool wide = force64_ || e.at.off >= 0xffffffffull;
        const size_t at = cd.size();
        cd.resize(at + 46 + e.name.size() + (wide ? 12 : 0));
        uint8_t *p = cd.data() + at;
        put32(p, 0x02014b50u);
        put16(p + 4, 45); // version made by
        putCommon(p + 6, wide ? 45 : 20, e);
        put16(p + 30, wide ? 12 : 0); // extra field
        put16(p + 32, 0);             // comment
        put16(p + 34, 0);             // disk
        put16(p + 36, 0);             // internal attributes
        put32(p + 38, !e.name.empty() && e.name.back() == '/' ? 0x10u : 0u);
        put32(p + 42, wide ? 0xffffffffu : (uint32_t)e.at.off);
        std::memcpy(p + 46, e.name.data(), e.name.size());
        if (wide) {
            uint8_t *x = p + 46 + e.name.size();
            put16(x, 0x0001);
            put16(x + 2, 8);
            put64(x + 4, e.at.off);
        }
    }
    const uint64_t cdSize = cd.size();
    const bool z64 = force64_ || count >= 0xffff || cdOff >= 0xffffffffull || cdSize >= 0xffffffffull;
    const size_t at = cd.size();
    cd.resize(at + (z64 ? 56 + 20 : 0) + 22);
    uint8_t *p = cd.data() + at;
    if (z64) {
        put32(p, 0x06064b50u);
        put64(p + 4, 44);
        put16(p + 12, 45);
        put16(p + 14, 45);
        put32(p + 16, 0);
        put32(p + 20, 0);
        put64(p + 24, count);
        put64(p + 32, count);
        put64(p + 40, cdSize);
        put64(p + 48, cdOff);
        p += 56;
        put32(p, 0x07064b50u);
        put32(p + 4, 0);
        put64(p + 8, cdOff + cdSize);
        put32(p + 16, 1);
        p += 20;
    }
    put32(p, 0x06054b50u);
    put16(p + 4, 0);
    put16(p + 6, 0);
    put16(p + 8, z64 ? 0xffffu : (uint32_t)count);
    put16(p + 10, z64 ? 0xffffu : (uint32_t)count);
    put32(p + 12, z64 ? 0xffffffffu : (uint32_t)cdSize);
    put32(p + 16, z64 ? 0xffffffffu : (uint32_t)cdOff);
    put16(p + 20, 0);
    planned_ += cd.size();
    write(cd.data(), cd.size());
    FILE *fp = fp_;
    fp_ = nullptr; // (from here on the destructor has nothing to close)
    const bool ok = fflush(fp) == 0 && fsync(fileno(fp)) == 0;
    if (fclose(fp) != 0 || !ok || rename(part_.c_str(), path_.c_str()) != 0) {
        const std::string why = strerror(errno);
        remove(part_.c_str());
        throw std::runtime_error("cannot write " + path_ + ": " + why);
    }
}

} // namespace abub
