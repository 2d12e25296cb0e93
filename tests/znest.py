"""The tests' model of a nested file (atz_set_nesting):
    "ATN" 1 | u64 length (whole file) | u64 outer_len | outer (outer_len bytes) | inner (to the end)
outer: an ATZ file (version 1-6) without its descriptors' payload bytes; inner: the ATZ or ATN file of P, the outer's
payloads concatenated in descriptor order.  Like tests/atzfile.py it trusts the file.  expected() is what a context with
a depth and no mask must write, from the oracle level by level; reconstruct() is the oracle's reader level by level."""
import struct

import _libs
import atzfile

HEADER = 20
MAX_LEVELS = 8   # "ATN" headers a reader follows


def _head(d):
    return 35 + (8 + 9 * d["nd"] if d["nd"] else 0)


def payloads(atz):
    """The payload of every descriptor of a flat file, in order."""
    return [d["raw"][_head(d):_head(d) + d["il"]] for d in atzfile.parse(atz)[2]]


def strip(atz):
    """A flat file -> (its stripped outer, P)."""
    _, origlen, descs, residue = atzfile.parse(atz)
    body = b"".join(d["raw"][:_head(d)] + d["raw"][_head(d) + d["il"]:] for d in descs)
    n = 28 + len(body) + len(residue)
    return atz[:4] + struct.pack("<QQQ", n, origlen, len(descs)) + body + residue, b"".join(payloads(atz))


def parse_stripped(outer):
    """-> (version, origlen, [dict(off, cl, il, c, w, m, nd, first_diff, pieces, raw, ipos)], residue): raw the stripped
    descriptor's bytes, ipos its payload's offset in P."""
    assert outer[:3] == b"ATZ"
    total, origlen, ns = struct.unpack_from("<QQQ", outer, 4)
    assert total == len(outer)
    at, out, pat = 28, [], 0
    for _ in range(ns):
        off, cl, il, c, w, m, nd = struct.unpack_from("<QQQBBBQ", outer, at)
        end = at + 35
        first_diff = -1
        if nd:
            first_diff, = struct.unpack_from("<Q", outer, end)
            end += 8 + 9 * nd
        split_at = end - at
        pieces = None
        if outer[3] >= 4 and c & 0x80:
            k, = struct.unpack_from("<I", outer, end)
            pieces = list(struct.unpack_from("<%dI" % k, outer, end + 4))
            end += 4 + 4 * k
        out.append(dict(off=off, cl=cl, il=il, c=c, w=w, m=m, nd=nd, first_diff=first_diff, pieces=pieces,
                        raw=outer[at:end], ipos=pat, split_at=split_at))
        pat += il
        at = end
    return outer[3], origlen, out, outer[at:]


def unstrip(outer, P):
    """The flat file of a stripped outer and its payloads."""
    _, origlen, descs, residue = parse_stripped(outer)
    assert sum(d["il"] for d in descs) == len(P)
    body = b"".join(d["raw"][:d["split_at"]] + P[d["ipos"]:d["ipos"] + d["il"]] + d["raw"][d["split_at"]:] for d in descs)
    n = 28 + len(body) + len(residue)
    return outer[:4] + struct.pack("<QQQ", n, origlen, len(descs)) + body + residue


def join(outer, inner):
    return b"ATN\1" + struct.pack("<QQ", HEADER + len(outer) + len(inner), len(outer)) + outer + inner


def split(atn):
    """-> (outer, inner)"""
    assert atn[:4] == b"ATN\1"
    total, outer_len = struct.unpack_from("<QQ", atn, 4)
    assert total == len(atn) and HEADER + outer_len <= total
    return atn[HEADER:HEADER + outer_len], atn[HEADER + outer_len:]


def levels(f):
    """The file's levels, outermost first: every one but the last a stripped outer, the last a flat file."""
    out = []
    while f[:3] == b"ATN":
        outer, f = split(f)
        out.append(outer)
    return out + [f]


def origlen(f):
    return struct.unpack_from("<Q", levels(f)[0], 12)[0]


def _level(data, depth, opts):
    """-> (rc, file, recorded streams of this level)"""
    rc, flat, _ = _libs.ora_precompress(data, **opts)
    if rc != 0:
        return rc, None, 0
    n = struct.unpack_from("<Q", flat, 20)[0]
    if depth == 0 or n == 0:
        return 0, flat, n
    outer, P = strip(flat)
    if not P:
        return 0, flat, n
    rc2, inner, n2 = _level(P, depth - 1, opts)
    if rc2 != 0 or n2 == 0:   # (the oracle's failures are the reference's own deaths: the file stays flat)
        return 0, flat, n
    return 0, join(outer, inner), n


def expected(data, depth, **opts):
    """What precompress at `depth` must write with no mask on (opts: _libs.ora_precompress's)."""
    rc, out, _ = _level(data, depth, opts)
    assert rc == 0, rc
    return out


def reconstruct(f):
    """-> (rc, the original), by the oracle's reader level by level (ATZ1 levels only)."""
    if f[:3] == b"ATN":
        outer, inner = split(f)
        rc, P = reconstruct(inner)
        if rc != 0:
            return rc, None
        return _libs.ora_reconstruct(unstrip(outer, P))
    return _libs.ora_reconstruct(f)


# ---- inputs ------------------------------------------------------------------------------------------------
def z(data, level, window=15, memlevel=8):
    """A zlib stream as the reference's deflate writes it."""
    return _libs.ora_deflate(data, level, window, memlevel)[0]


def sample(r, inner_levels=(1, 9), outer_level=6, deeper=0):
    """Text around one level-`outer_level` stream whose payload is text, a stream of each of `inner_levels` and text;
    deeper: that many more levels of the same shape inside the first inner stream."""
    def body(depth):
        parts = [_libs.text(r, 700)]
        for i, lv in enumerate(inner_levels):
            inside = body(depth - 1) if depth and i == 0 else _libs.text(r, 1500 + 300 * i)
            parts += [z(inside, lv), _libs.text(r, 400)]
        return b"".join(parts)
    return _libs.text(r, 900) + z(body(deeper), outer_level) + _libs.text(r, 500)


def near(s):
    """zlib stream s with the spare bits behind its last end-of-block code set (tests/nearmiss.py eobpad): one byte off
    what any trial writes and the same stream to a decoder; None if that code ends on a byte boundary."""
    import nearmiss
    end = nearmiss.walk_blocks(s)[-1][4]
    if end % 8 == 0:
        return None
    b = bytearray(s)
    nearmiss._set_bits(b, end, (end + 7) & ~7)
    return bytes(b)


def near_sample(r):
    """Text around a near-miss level-6 stream (recorded with one diff) whose payload holds two streams."""
    while True:
        s = near(z(_libs.text(r, r.randint(300, 900)) + z(_libs.text(r, 2000), 4) + _libs.text(r, 300) +
                   z(_libs.text(r, 1200), 7), 6))
        if s is not None:
            return _libs.text(r, 300) + s + _libs.text(r, 300)
