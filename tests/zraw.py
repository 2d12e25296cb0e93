"""The container extension restated in Python: hand-built ZIP entries and gzip members,
the anchor kernel's list, the host's parse / acceptance / overlap rule, the raw walk's candidate list and its
rule.  Expected deflate bytes come from the reference's zlib 1.2.8 (zstrat.deflate with a negative window);
the model's inflate is Python's zlib.decompressobj(-15).
"""
import struct
import zlib

import zstrat

ZIP, GZIP = 0, 1
HINT_NONE, HINT_FAST, HINT_MAX = 0, 1, 2
MEMLEVELS = (8, 9, 7, 6, 5, 4, 3, 2, 1)
LEVELS = {HINT_NONE: (6, 9, 1, 5, 7, 8, 4, 3, 2, 0), HINT_FAST: (1, 2, 3, 4, 5, 6, 7, 8, 9, 0),
          HINT_MAX: (9, 8, 7, 6, 5, 4, 3, 2, 1, 0)}
ZIP_HINT_BITS = {HINT_NONE: 0, HINT_MAX: 1 << 1, HINT_FAST: 2 << 1}   # general purpose bits 2-1
GZIP_XFL = {HINT_NONE: 0, HINT_MAX: 2, HINT_FAST: 4}


def raw_deflate(data, level, memlevel, window=15, strategy=0):
    """The raw deflate body zlib 1.2.8 writes (deflateInit2 with -window)."""
    return zstrat.deflate(data, level, -window, memlevel, strategy)


# ---- builders ------------------------------------------------------------------------------------
def zip_entry(body, usize, name=b"", extra=b"", flags=0, method=8, csize=None, crc=0, descriptor=False):
    """A ZIP local file header, `body`, and with `descriptor` a data descriptor (flag bit 3, sizes 0 in the
    header).  csize / usize as given (csize None: len(body)), so a test can state wrong ones."""
    if csize is None:
        csize = len(body)
    if descriptor:
        flags |= 8
        hc, hu = 0, 0
    else:
        hc, hu = csize, usize
    hdr = struct.pack("<4sHHHHHIIIHH", b"PK\3\4", 20, flags, method, 0x6000, 0x5521, crc, hc, hu, len(name),
                      len(extra))
    out = hdr + name + extra + body
    if descriptor:
        out += struct.pack("<4sIII", b"PK\7\x08", crc, csize, usize)
    return out


def gzip_member(body, payload, extra=None, name=None, comment=None, hcrc=False, xfl=0, isize=None, flg_more=0):
    """A gzip member around `body`: the 10 fixed bytes, the optional fields FLG names, CRC-32 and ISIZE."""
    flg = flg_more | (4 if extra is not None else 0) | (8 if name is not None else 0) | \
        (16 if comment is not None else 0) | (2 if hcrc else 0)
    out = struct.pack("<3sBIBB", b"\x1f\x8b\x08", flg, 0x5f000000, xfl, 3)
    if extra is not None:
        out += struct.pack("<H", len(extra)) + extra
    if name is not None:
        out += name + b"\0"
    if comment is not None:
        out += comment + b"\0"
    if hcrc:
        out += struct.pack("<H", zlib.crc32(out) & 0xffff)
    if isize is None:
        isize = len(payload) & 0xffffffff
    return out + body + struct.pack("<II", zlib.crc32(payload), isize)


# ---- the anchor kernel -----------------------------------------------------------------------------
def anchors(data, mask):
    """[(position, kind)] ascending: what k_anchors_ordered reports."""
    n, out = len(data), []
    if mask & 1:
        at = data.find(b"PK\3\4")
        while at >= 0:
            if at + 30 <= n and data[at + 8] == 8 and data[at + 9] == 0 and not data[at + 6] & 1:
                out.append((at, ZIP))
            at = data.find(b"PK\3\4", at + 1)
    if mask & 2:
        at = data.find(b"\x1f\x8b\x08")
        while at >= 0:
            if at + 18 <= n and not data[at + 3] & 0xe0:
                out.append((at, GZIP))
            at = data.find(b"\x1f\x8b\x08", at + 1)
    return sorted(out)


# ---- the host's parse, acceptance and overlap rule -------------------------------------------------------
def parse(data, p, kind):
    """-> None (dropped) or dict(d, limit, hint, csize, usize) with csize / usize None when not stated."""
    n = len(data)
    if kind == ZIP:
        flag, = struct.unpack_from("<H", data, p + 6)
        csize, usize, nlen, xlen = struct.unpack_from("<IIHH", data, p + 18)
        d = p + 30 + nlen + xlen
        if d >= n:
            return None
        dd = bool(flag & 8)
        know_c = not dd and csize not in (0, 0xffffffff)
        know_u = not dd and usize != 0xffffffff
        if know_c and d + csize > n:
            return None
        lv = (flag >> 1) & 3
        return dict(d=d, limit=csize if know_c else n - d, hint=HINT_MAX if lv == 1 else HINT_FAST if lv else HINT_NONE,
                    csize=csize if know_c else None, usize=usize if know_u else None)
    flg, xfl = data[p + 3], data[p + 8]
    at = p + 10
    if flg & 4:
        if at + 2 > n:
            return None
        at += 2 + struct.unpack_from("<H", data, at)[0]
        if at > n:
            return None
    for bit in (8, 16):
        if flg & bit:
            z = data.find(b"\0", at)
            if z < 0:
                return None
            at = z + 1
    if flg & 2:
        at += 2
        if at > n:
            return None
    if at + 8 >= n:
        return None
    return dict(d=at, limit=n - at - 8, hint=HINT_MAX if xfl == 2 else HINT_FAST if xfl == 4 else HINT_NONE)


def inflate_raw(buf):
    """-> None unless `buf` starts with a complete raw deflate stream, else (consumed, output)."""
    z = zlib.decompressobj(-15)
    try:
        out = z.decompress(buf)
    except zlib.error:
        return None
    if not z.eof:
        return None
    return len(buf) - len(z.unused_data), out


def raw_records(data, mask, ref_records):
    """The raw records the scan adds to the reference's ref_records [(offset, comp_len)]:
    [(offset, comp_len, infl_len, type)] ascending, type = 24 + hint."""
    acc = []
    for p, kind in anchors(data, mask):
        c = parse(data, p, kind)
        if c is None:
            continue
        r = inflate_raw(data[c["d"]:c["d"] + c["limit"]])
        if r is None:
            continue
        consumed, out = r
        if not 1 <= len(out) < 1 << 31:
            continue
        if kind == ZIP:
            if c["csize"] is not None and consumed != c["csize"]:
                continue
            if c["usize"] is not None and len(out) != c["usize"]:
                continue
        elif struct.unpack_from("<I", data, c["d"] + consumed + 4)[0] != len(out) & 0xffffffff:
            continue
        lo, hi = c["d"], c["d"] + consumed
        if any(o < hi and lo < o + cl for o, cl in ref_records):
            continue
        acc.append((lo, p, consumed, len(out), 24 + c["hint"]))
    out, end = [], 0
    for lo, _, consumed, produced, typ in sorted(acc):
        if lo < end:
            continue
        end = lo + consumed
        out.append((lo, consumed, produced, typ))
    return out


# ---- the raw walk ----------------------------------------------------------------------------------
def candidates(hint):
    """(level, window, memlevel) in the raw walk's order."""
    return [(lv, 15, m) for m in MEMLEVELS for lv in LEVELS[hint]]


def rule(body, inflated, hint, recomp_tresh=128, sizediff_tresh=128, mismatch_tol=2, shortcut_len=512):
    """zstrat.rule over candidates(hint) with raw outputs: testDeflateParams and the stop rule (main.cpp:616-700)
    restarted with identBytes = 0 on the body.  -> None if the body is not recorded, else dict(level, window,
    memlevel, ident, diff_pos, diff_val)."""
    C_ = len(body)
    best, ident = None, 0
    for cand in candidates(hint):
        lv, w, m = cand
        out = raw_deflate(inflated, lv, m, w)
        if C_ > shortcut_len:
            head = out[:shortcut_len]
            if sum(1 for x, y in zip(head, body) if x == y) < (shortcut_len - recomp_tresh) % (1 << 64):
                continue
        if abs(len(out) - C_) > sizediff_tresh:
            continue
        k = min(len(out), C_)
        same = sum(1 for a, b in zip(out[:k], body[:k]) if a == b)
        if same > ident:
            ident, best = same, (cand, out)
            if same == C_ or same + mismatch_tol >= C_:
                break
    if best is None or not (C_ - ident <= recomp_tresh and ident > 0):
        return None
    (lv, w, m), out = best
    pos = [i for i in range(C_) if i >= len(out) or out[i] != body[i]]
    return dict(level=lv, window=w, memlevel=m, ident=ident, diff_pos=pos, diff_val=bytes(body[i] for i in pos))
