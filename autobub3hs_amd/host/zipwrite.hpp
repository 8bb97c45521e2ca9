// zipwrite.hpp -- the canonical zip archive of abub3hs --archive ("A run as one archive"): stored entries,
// the data of every entry that has any at a multiple of 16, every byte fixed by rule, so that the host route, the device
// route (abub_zip_pack_dev forms the entries whose files are resident on the device) and the tests' restatement
// (tests/zipref.py) write the same file.  zipLayout is the one layout function: the host route, the device route's planning
// and the central directory take an entry's place from it.  The archive is written as <path>.part and renamed once its end
// record is on disk; a writer that is destroyed before finish() removes the .part file and leaves an older <path> alone.
// Internal to the host library.
#ifndef ABUB3HS_ZIPWRITE_HPP
#define ABUB3HS_ZIPWRITE_HPP

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace abub {

// Where an entry lies: its local header at `off`, then the name, the padding field, the data
struct ZipLayout {
    uint64_t off = 0;
    uint16_t nameLen = 0, extraLen = 0;
    uint32_t len = 0;
    uint64_t head() const { return 30ull + nameLen + extraLen; }
    uint64_t data() const { return off + head(); }
    uint64_t end() const { return data() + len; }
};
// The entry of `len` bytes named with nameLen bytes whose local header starts at archive offset `off`: data of length > 0
// starts at a multiple of 16.  p = (-(off + 30 + nameLen)) mod 16 bytes are missing; the padding field (u16 0x4241, u16
// size, zeros) takes p bytes, or p + 16 where p is 1, 2 or 3 (a field has four bytes at least); none where p is 0 or the
// entry is empty
inline ZipLayout zipLayout(uint64_t off, size_t nameLen, uint64_t len)
{
    ZipLayout l;
    l.off = off;
    l.nameLen = (uint16_t)nameLen;
    l.len = (uint32_t)len;
    const unsigned p = (unsigned)((0 - (off + 30 + nameLen)) & 15);
    l.extraLen = (uint16_t)(len == 0 || p == 0 ? 0 : p >= 4 ? p : p + 16);
    return l;
}

class ZipWriter {
public:
    struct Entry {
        std::string name;
        ZipLayout at;
        uint32_t crc = 0;
    };
    // opens <path>.part; throws std::runtime_error where that cannot be written.  ABUB_ZIP64_FORCE=1 (a test knob): every
    // central record carries the zip64 offset field, and the zip64 end record and its locator are present
    explicit ZipWriter(const std::string &path);
    ~ZipWriter();
    ZipWriter(const ZipWriter &) = delete;
    ZipWriter &operator=(const ZipWriter &) = delete;

    // The next entry gets its place behind the last planned one; returns its index.  Throws on a name of more than 65535
    // bytes or a length of 2^32 - 1 and more
    size_t plan(const std::string &name, uint64_t len);
    const Entry &entry(size_t i) const { return entries_[i]; }
    uint64_t planned() const { return planned_; } // the archive offset behind the last planned entry
    void setCrc(size_t i, uint32_t crc) { entries_[i].crc = crc; }
    // entry i's local header with its CRC, its name and its padding field: entry(i).at.head() bytes
    void putHead(size_t i, uint8_t *dst) const;
    // entry i whole from the host's bytes: its CRC is taken (zlib) and kept, head and data go to dst (room up to at.end() - at.off)
    void putEntry(size_t i, const uint8_t *data, uint8_t *dst);
    // the next n bytes of the archive (whole planned entries, in order); throws on an IO failure
    void write(const uint8_t *bytes, size_t n);
    // plan + putEntry + write of one entry
    void add(const std::string &name, const uint8_t *data, size_t len);
    // the central directory and the end records behind the last entry (all planned bytes must have been written), the
    // file on disk, the rename
    void finish();
    uint64_t bytes() const { return written_; } // of the archive so far (after finish(): its size)
    size_t entries() const { return entries_.size(); }
    const std::string &path() const { return path_; }

private:
    std::string path_, part_;
    FILE *fp_ = nullptr;
    bool force64_ = false;
    uint64_t planned_ = 0, written_ = 0;
    std::vector<Entry> entries_;
};

// the archive a ZipParser opens for the run folder `folder` (its rule: trailing separators go, ".zip" is added where the
// last component has no extension)
std::string zipPathOf(const std::string &folder);

} // namespace abub
#endif
