"""The stitch extension restated in Python: hand-built PNG files whose IDAT split a test states
chunk by chunk, the anchor kernel's list, the cursor walk over the anchors, the candidate, acceptance and hull
rules, a record's piece list, the ATZ4 descriptor and the residue.  The model's inflate is Python's
zlib.decompressobj(); expected deflate bytes come from zstrat (the reference's zlib 1.2.8).
"""
import struct
import zlib

import atzfile

SIG = b"\x89PNG\r\n\x1a\n"
FRAMING = 12   # between two payloads: the chunk's CRC, the next chunk's length, "IDAT"


# ---- builders ------------------------------------------------------------------------------------
def chunk(typ, payload, length=None, crc=None):
    """One PNG chunk; `length` and `crc` as given when a test wants wrong ones."""
    if length is None:
        length = len(payload)
    if crc is None:
        crc = zlib.crc32(typ + payload)
    return struct.pack(">I", length) + typ + payload + struct.pack(">I", crc)


def idat_chain(payload, lens):
    """`payload` cut into consecutive IDAT chunks of the lengths `lens` (which sum to its length)."""
    assert sum(lens) == len(payload), (sum(lens), len(payload))
    out, at = [], 0
    for n in lens:
        out.append(chunk(b"IDAT", payload[at:at + n]))
        at += n
    return b"".join(out)


def png(payload, lens, width=16, height=16):
    """A PNG file: signature, IHDR, `payload` (a zlib stream, with whatever follows it) in IDAT chunks of the
    lengths `lens`, IEND.  -> (bytes, offset of the first payload byte)"""
    head = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0))
    return head + idat_chain(payload, lens) + chunk(b"IEND", b""), len(head) + 8


def split(n, size):
    """Chunk lengths that cut n bytes every `size` bytes, as a PNG writer does."""
    return [size] * (n // size) + ([n % size] if n % size else [])


# ---- the anchor kernel -----------------------------------------------------------------------------
def anchors(data):
    """Ascending positions a of the 'I' of a chunk type field "IDAT": a >= 4, the big-endian length L at a - 4
    is below 2^31, and payload and CRC lie inside the file, a + 8 + L <= n."""
    n, out = len(data), []
    a = data.find(b"IDAT")
    while a >= 0:
        if a >= 4:
            L, = struct.unpack_from(">I", data, a - 4)
            if L < 1 << 31 and a + 8 + L <= n:
                out.append(a)
        a = data.find(b"IDAT", a + 1)
    return out


# ---- chains and candidates ---------------------------------------------------------------------------
def chains(data, anch=None):
    """The cursor walk: [[(payload offset, length), ...], ...].  An anchor below the cursor belongs to no chain;
    a chain follows a' = a + L + 12 while a' is an anchor; the cursor then stands behind the last chunk's CRC."""
    anch = anchors(data) if anch is None else anch
    known, cursor, out = set(anch), 0, []
    for a in anch:
        if a < cursor:
            continue
        ch = []
        while True:
            L, = struct.unpack_from(">I", data, a - 4)
            ch.append((a + 4, L))
            cursor = a + 8 + L
            if a + L + 12 not in known:
                break
            a += L + 12
        out.append(ch)
    return out


def header_type(b0, b1):
    """The reference's offsetType 0..23 of a two-byte zlib header, -1 for any other pair."""
    if b0 & 15 != 8 or not 2 <= b0 >> 4 <= 7 or b1 & 0x20 or ((b0 << 8) | b1) % 31:
        return -1
    return ((b0 >> 4) - 2) * 4 + (b1 >> 6)


def candidates(data, anch=None):
    """[(pieces, type)]: each chain without its leading empty chunks, if two chunks or more remain and the
    concatenated payloads start with a zlib header."""
    out = []
    for ch in chains(data, anch):
        while ch and ch[0][1] == 0:
            ch = ch[1:]
        if len(ch) < 2:
            continue
        head = b"".join(data[o:o + n] for o, n in ch)[:2]
        t = header_type(head[0], head[1]) if len(head) == 2 else -1
        if t >= 0:
            out.append((ch, t))
    return out


def gathered_bytes(data, anch=None):
    """Payload bytes the stitch buffer receives (without alignment): never more than len(data)."""
    return sum(n for ch, _ in candidates(data, anch) for _, n in ch)


# ---- acceptance, pieces, hull ------------------------------------------------------------------------
def inflate(buf):
    """-> None unless `buf` starts with a complete zlib stream (Adler-32 checked), else (consumed, output)."""
    z = zlib.decompressobj()
    try:
        out = z.decompress(buf)
    except zlib.error:
        return None
    if not z.eof:
        return None
    return len(buf) - len(z.unused_data), out


def pieces_of(ch, consumed):
    """The pieces the first `consumed` stream bytes touch: the last one ends where the stream does."""
    out, total = [], 0
    for o, n in ch:
        if total >= consumed:
            break
        take = min(n, consumed - total)
        out.append((o, take))
        total += take
    assert total == consumed
    return out


def hull(pieces):
    return sum(n for _, n in pieces) + FRAMING * (len(pieces) - 1)


def stitched_records(data, prior=()):
    """The stitched records the scan adds to the records made before, prior = [(offset, length in the file)]:
    [dict(offset, comp_len, infl_len, type, pieces, stream, payload)] ascending, and the accepted candidates
    the hull rule dropped (same dicts)."""
    kept, dropped = [], []
    for ch, t in candidates(data):
        joined = b"".join(data[o:o + n] for o, n in ch)
        r = inflate(joined)
        if r is None:
            continue
        consumed, out = r
        if not 1 <= len(out) < 1 << 31 or consumed <= ch[0][1]:
            continue
        pcs = pieces_of(ch, consumed)
        rec = dict(offset=pcs[0][0], comp_len=consumed, infl_len=len(out), type=t, pieces=pcs,
                   stream=joined[:consumed], payload=out)
        lo, hi = rec["offset"], rec["offset"] + hull(pcs)
        (dropped if any(o < hi and lo < o + n for o, n in prior) else kept).append(rec)
    return kept, dropped


# ---- the flat twin -----------------------------------------------------------------------------------
def flat_twin(data):
    """`data` with every chain of two chunks or more rewritten as one IDAT chunk that holds the same payload
    bytes.  -> (twin, {payload offset of the chain's first non-empty chunk in data: payload offset in the twin})"""
    out, at, where = [], 0, {}
    for ch in chains(data):
        if len(ch) < 2:
            continue
        first, last = ch[0], ch[-1]
        out.append(data[at:first[0] - 8])
        pos = sum(len(x) for x in out) + 8
        lead = [c for c in ch if c[1]]
        if lead:
            where[lead[0][0]] = pos
        out.append(chunk(b"IDAT", b"".join(data[o:o + n] for o, n in ch)))
        at = last[0] + last[1] + 4
    out.append(data[at:])
    return b"".join(out), where


# ---- the ATZ4 file -----------------------------------------------------------------------------------
def descriptor(rec, clevel, window, memlevel, diff_pos=(), diff_val=b""):
    """The ATZ4 descriptor of stitched record `rec`: the version 1 layout (writeStreamdesc) with bit 7 of the
    clevel byte set, then the inflated payload, then u32 k and k x u32 piece lengths."""
    out = struct.pack("<QQQBBBQ", rec["offset"], rec["comp_len"], rec["infl_len"], 0x80 | clevel, window, memlevel,
                      len(diff_pos))
    if diff_pos:
        out += struct.pack("<Q", diff_pos[0])
        out += b"".join(struct.pack("<Q", 0 if k == 0 else diff_pos[k] - diff_pos[k - 1]) for k in range(len(diff_pos)))
        out += bytes(diff_val)
    out += rec["payload"]
    out += struct.pack("<I", len(rec["pieces"])) + b"".join(struct.pack("<I", n) for _, n in rec["pieces"])
    return out


def parse_atz(atz):
    """-> (version, origlen, [dict(off, cl, il, c, w, m, nd, raw, pieces)], residue bytes) of an ATZ file
    (atzfile.parse's fields of these names); pieces: a stitched descriptor's lengths, else None."""
    ver, origlen, descs, res = atzfile.parse(atz)
    return ver, origlen, [{k: d[k] for k in ("off", "cl", "il", "c", "w", "m", "nd", "raw", "pieces")} for d in descs], res


def residue(data, ranges):
    """Every byte of `data` outside the recorded ranges [(offset, length)] (one per piece of a stitched record)."""
    out, at = [], 0
    for o, n in sorted(ranges):
        out.append(data[at:o])
        at = o + n
    out.append(data[at:])
    return b"".join(out)
