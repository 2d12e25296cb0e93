"""The segment extension restated in Python: streams written with deflate(Z_FULL_FLUSH) by the
reference's zlib 1.2.8 (zstrat.z128), the marker list, a bit-level decoder of one segment, the chain rule with
the replacement of a record by its segments, and the raw walk's rule on a segment.
"""
import ctypes as C

import zgnu
import zraw
import zstrat

Z_SYNC_FLUSH, Z_FULL_FLUSH, Z_FINISH = 2, 3, 4
MARKER = b"\x00\x00\xff\xff"
END, ERROR, NEED = 0, 1, 2   # atz_inflate_batch's status values
FLAG_FLUSH = 128             # atz_cand_t.flags bit 7


# ---- zlib 1.2.8 with flushes -----------------------------------------------------------------------
def flush_stream(segments, level, memlevel, window=15, how=Z_FULL_FLUSH, finish=True):
    """One deflateInit2 (window < 0: raw), then each segment followed by deflate(how), the last one by
    deflate(Z_FINISH) when `finish` -> (stream, [output length after each call])."""
    L = zstrat.z128()
    zs = zstrat.ZStream()
    r = L.deflateInit2_(C.byref(zs), level, zstrat.Z_DEFLATED, window, memlevel, 0, b"1.2.8", C.sizeof(zstrat.ZStream))
    assert r == 0, r
    total = sum(len(s) for s in segments)
    cap = L.deflateBound(C.byref(zs), total) + 64 + 16 * len(segments)
    out = C.create_string_buffer(cap)
    zs.next_out = C.cast(out, C.c_void_p)
    zs.avail_out = cap
    ends, keep = [], []
    for i, seg in enumerate(segments):
        src = C.create_string_buffer(bytes(seg), max(len(seg), 1))
        keep.append(src)
        zs.next_in = C.cast(src, C.c_void_p)
        zs.avail_in = len(seg)
        last = finish and i == len(segments) - 1
        r = L.deflate(C.byref(zs), Z_FINISH if last else how)
        assert r == (zstrat.Z_STREAM_END if last else 0) and zs.avail_in == 0, r
        ends.append(zs.total_out)
    n = zs.total_out
    L.deflateEnd(C.byref(zs))
    return out.raw[:n], ends


def flushed_deflate(data, level, memlevel, window=15):
    """The raw body of `data` as deflate(Z_FULL_FLUSH) ends it: what a flush-terminated segment holds."""
    return flush_stream([data], level, memlevel, -window, Z_FULL_FLUSH, finish=False)[0]


# ---- the marker list ---------------------------------------------------------------------------------
def markers(data):
    """Every q with q + 4 <= len(data) and data[q:q+4] == 00 00 FF FF, ascending: k_marker_ordered's list."""
    out, at = [], data.find(MARKER)
    while at >= 0:
        out.append(at)
        at = data.find(MARKER, at + 1)
    return out


# ---- the segment decoder -----------------------------------------------------------------------------
def seg_inflate(buf):
    """A raw deflate decode of `buf` that also ends at the first stored block with BFINAL = 0 and LEN = 0 ->
    (status, consumed, output, at_marker); consumed is exact for END only.  A distance reaching before the start
    is an error; running out of input is NEED."""
    br, out = zgnu._Bits(buf), bytearray()
    try:
        while True:
            last, btype = br.get(1), br.get(2)
            if btype == 0:
                br.align()
                if br.pos + 4 > len(buf):
                    return NEED, len(buf), bytes(out), False
                n = buf[br.pos] | (buf[br.pos + 1] << 8)
                if n ^ 0xffff != buf[br.pos + 2] | (buf[br.pos + 3] << 8):
                    return ERROR, br.pos + 4, bytes(out), False
                br.pos += 4
                if not last and n == 0:
                    return END, br.pos, bytes(out), True
                if br.pos + n > len(buf):
                    return NEED, len(buf), bytes(out), False
                out += buf[br.pos:br.pos + n]
                br.pos += n
            elif btype == 3:
                return ERROR, br.pos, bytes(out), False
            else:
                if btype == 1:
                    tl, td = zgnu._FIXED_L, zgnu._FIXED_D
                else:
                    hlit, hdist, hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
                    if hlit > 286 or hdist > 30:
                        return ERROR, br.pos, bytes(out), False
                    cl = [0] * 19
                    for i in range(hclen):
                        cl[zgnu.CLORD[i]] = br.get(3)
                    tc, lens = zgnu._table(cl), []
                    while len(lens) < hlit + hdist:
                        s = zgnu._sym(br, tc)
                        if s < 16:
                            lens.append(s)
                        elif s == 16:
                            if not lens:
                                return ERROR, br.pos, bytes(out), False
                            lens += [lens[-1]] * (3 + br.get(2))
                        elif s == 17:
                            lens += [0] * (3 + br.get(3))
                        else:
                            lens += [0] * (11 + br.get(7))
                    if len(lens) != hlit + hdist or lens[256] == 0:
                        return ERROR, br.pos, bytes(out), False
                    tl, td = zgnu._table(lens[:hlit]), zgnu._table(lens[hlit:])
                while True:
                    s = zgnu._sym(br, tl)
                    if s < 256:
                        out.append(s)
                    elif s == 256:
                        break
                    elif s > 285:
                        return ERROR, br.pos, bytes(out), False
                    else:
                        ln = zgnu.LBASE[s - 257] + br.get(zgnu.LEXT[s - 257])
                        d = zgnu._sym(br, td)
                        if d > 29:
                            return ERROR, br.pos, bytes(out), False
                        dist = zgnu.DBASE[d] + br.get(zgnu.DEXT[d])
                        if dist > len(out):
                            return ERROR, br.pos, bytes(out), False
                        for _ in range(ln):
                            out.append(out[-dist])
            if last:
                return END, br.pos, bytes(out), False
    except IndexError:
        return NEED, len(buf), bytes(out), False
    except AssertionError:   # no code of up to 15 bits matches
        return ERROR, br.pos, bytes(out), False


# ---- the chain rule and the replacement --------------------------------------------------------------
def hint_type(data, rec):
    """24 + hint of a record's segments: a raw parent's own; a zlib parent's FLEVEL 0, 1 -> fast, 2 -> none, 3 -> max"""
    off, typ = rec[0], rec[1]
    if typ >= 24:
        return typ
    return {0: 25, 1: 25, 2: 24, 3: 26}[data[off + 1] >> 6]


def body_of(data, rec):
    """-> None (not eligible by its kind) or (body_start, body_end).  Stitched records are the caller's to drop."""
    off, typ, cl = rec[0], rec[1], rec[2]
    if 24 <= typ <= 26:
        return off, off + cl
    if typ < 24 and cl >= 7 and data[off] >> 4 == 7 and not rec[4] & 64:
        return off + 2, off + cl - 4
    return None


def chain(data, b0, b1, infl_len):
    """-> None unless the chain from b0 completes, else [(start, consumed, produced, at_marker)] (k >= 2 entries,
    the last one the final segment, possibly with produced 0)."""
    s, segs, total = b0, [], 0
    while s < b1:
        st, consumed, out, am = seg_inflate(data[s:b1])
        if st != END:
            return None
        if am:
            if len(out) < 1:
                return None
            segs.append((s, consumed, len(out), True))
            s += consumed
            total += len(out)
            continue
        if s + consumed != b1:
            return None
        segs.append((s, consumed, len(out), False))
        total += len(out)
        return segs if len(segs) >= 2 and total == infl_len else None
    return None


def split(data, recs):
    """The scan's records [(offset, type, comp_len, infl_len, flags)] with every record whose chain completes
    replaced by its segments: what atz_scan returns under the mask."""
    ms, out = markers(data), []
    for rec in recs:
        b = body_of(data, rec)
        segs = None
        if b is not None and any(b[0] <= q and q + 4 < b[1] for q in ms):
            segs = chain(data, b[0], b[1], rec[3])
        if segs is None:
            out.append(tuple(rec))
            continue
        typ = hint_type(data, rec)
        for s, consumed, produced, am in segs:
            if produced:
                out.append((s, typ, consumed, produced, FLAG_FLUSH if am else 0))
    return out


# ---- the walk ------------------------------------------------------------------------------------------
def rule(body, inflated, hint, flush, recomp_tresh=128, sizediff_tresh=128, mismatch_tol=2, shortcut_len=512):
    """zraw.rule with the outputs a segment's trials write, flush-terminated when `flush` (a bit-7 record):
    testDeflateParams and the stop rule (main.cpp:616-700) restarted with identBytes = 0 over zraw.candidates(hint).
    -> None if the body is not recorded, else dict(level, window, memlevel, ident, diff_pos, diff_val)."""
    if not flush:
        return zraw.rule(body, inflated, hint, recomp_tresh, sizediff_tresh, mismatch_tol, shortcut_len)
    C_ = len(body)
    best, ident = None, 0
    for cand in zraw.candidates(hint):
        lv, w, m = cand
        out = flushed_deflate(inflated, lv, m, w)
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
