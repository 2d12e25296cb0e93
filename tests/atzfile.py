"""The tests' one reader of an ATZ file (versions 1-6).  It trusts the file: sizes are not checked
beyond the total length, which is what the tests' writers and the library's own output need.  The product's reader
is antiz_amd/csrc/atz_format.h; tests/test_format_cpu.py compares the two on every file that one accepts."""
import struct


def parse(atz):
    """-> (version, origlen, descriptors, residue bytes).  A descriptor: dict(off, cl, il, c, w, m, nd, first_diff,
    pos, val, raw, pieces) -- first_diff -1 and pos [] without diffs, else pos the absolute diff positions in the
    stream (first_diff plus the deltas' prefix sums, as Python integers: no wrap) and val their bytes; raw: the
    descriptor's own bytes, payload and piece list included; pieces: a stitched descriptor's lengths, else None
    (read whenever bit 7 of c is set and the version is at least 4)."""
    assert atz[:3] == b"ATZ"
    total, origlen, ns = struct.unpack_from("<QQQ", atz, 4)
    assert total == len(atz)
    at, out = 28, []
    for _ in range(ns):
        off, cl, il, c, w, m, nd = struct.unpack_from("<QQQBBBQ", atz, at)
        end = at + 35
        first_diff, pos, val = -1, [], b""
        if nd:
            first_diff, = struct.unpack_from("<Q", atz, end)
            p = first_diff
            for d in struct.unpack_from("<%dQ" % nd, atz, end + 8):
                p += d
                pos.append(p)
            val = atz[end + 8 + 8 * nd:end + 8 + 9 * nd]
            end += 8 + 9 * nd
        end += il
        pieces = None
        if atz[3] >= 4 and c & 0x80:
            k, = struct.unpack_from("<I", atz, end)
            pieces = list(struct.unpack_from("<%dI" % k, atz, end + 4))
            end += 4 + 4 * k
        out.append(dict(off=off, cl=cl, il=il, c=c, w=w, m=m, nd=nd, first_diff=first_diff, pos=pos, val=val,
                        raw=atz[at:end], pieces=pieces))
        at = end
    return atz[3], origlen, out, atz[at:]
