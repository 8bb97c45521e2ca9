"""The canonical zip archive of abub3hs --archive restated with struct and zlib.crc32 (the rules: DESIGN section 3, "A run as
one archive"; the definition: autobub3hs_amd/host/zipwrite.cpp).  Stored entries, every byte fixed by rule; the data of an
entry with any starts at an archive offset that is a multiple of 16."""
import struct
import zlib

DATE = 0x0021  # 1980-01-01; the time is 0


def extra_len(off, name_len, length):
    """of the padding field of the entry whose local header starts at `off`"""
    p = -(off + 30 + name_len) % 16
    if length == 0 or p == 0:
        return 0
    return p if p >= 4 else p + 16


def extra_field(xl):
    return b"" if xl == 0 else struct.pack("<HH", 0x4241, xl - 4) + bytes(xl - 4)


def local_entry(off, name, data):
    """local header, name, padding field, data of one entry at archive offset `off`"""
    xl = extra_len(off, len(name), len(data))
    head = struct.pack("<IHHHHHIIIHH", 0x04034B50, 20, 0, 0, 0, DATE, zlib.crc32(data), len(data), len(data), len(name), xl)
    return head + name + extra_field(xl) + data


def layout(entries, start=0):
    """[(offset of the local header, extra_len)] of (name, data) entries laid out from archive offset `start`"""
    out, off = [], start
    for name, data in entries:
        xl = extra_len(off, len(name), len(data))
        out.append((off, xl))
        off += 30 + len(name) + xl + len(data)
    return out


def archive(entries, force64=False):
    """the whole archive of [(name bytes, data bytes)]"""
    body, offs = bytearray(), []
    for name, data in entries:
        offs.append(len(body))
        body += local_entry(len(body), name, data)
    cd = bytearray()
    for (name, data), off in zip(entries, offs):
        wide = force64 or off >= 0xFFFFFFFF
        extra = struct.pack("<HHQ", 1, 8, off) if wide else b""
        cd += struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 45, 45 if wide else 20, 0, 0, 0, DATE, zlib.crc32(data), len(data),
                          len(data), len(name), len(extra), 0, 0, 0, 0x10 if name.endswith(b"/") else 0,
                          0xFFFFFFFF if wide else off)
        cd += name + extra
    n, cd_off, cd_size = len(entries), len(body), len(cd)
    z64 = force64 or n >= 0xFFFF or cd_off >= 0xFFFFFFFF or cd_size >= 0xFFFFFFFF
    end = b""
    if z64:
        end += struct.pack("<IQHHIIQQQQ", 0x06064B50, 44, 45, 45, 0, 0, n, n, cd_size, cd_off)
        end += struct.pack("<IIQI", 0x07064B50, 0, cd_off + cd_size, 1)
        end += struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, 0xFFFF, 0xFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0)
    else:
        end += struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, n, n, cd_size, cd_off, 0)
    return bytes(body) + bytes(cd) + end


def run_entries(run_id, event_text, events, image_folder="Images"):
    """the entries of a run's archive in canonical order: events = [(event, [(frame name, bytes)])] in sorted-event order,
    the frames in task order; event_text: the event file's bytes (b"" = no entry)"""
    rid = run_id.encode()
    out = [(rid + b"/", b"")]
    if event_text:
        out.append((rid + b"/" + rid + b".txt", event_text))
    for ev, frames in events:
        d = rid + b"/" + str(ev).encode() + b"/"
        out.append((d, b""))
        for level in [x for x in image_folder.split("/") if x]:
            d += level.encode() + b"/"
            out.append((d, b""))
        out += [(d + name.encode(), data) for name, data in frames]
    return out
