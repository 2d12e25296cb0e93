"""The probe extension restated in Python: the rule k_probe_ordered applies to every byte
position, its position list, the host's pre-drop, acceptance and merge, and hand-built dynamic-block headers.
The model's inflate is Python's zlib.decompressobj(-15) (zraw.inflate_raw); the walk of a probe record is the
container extension's without a hint (zraw.candidates / zraw.rule on libz128's raw output).
"""
import random

import numpy as np

import zraw

PROBE_MIN_OUT = 256
TYPE = 24   # raw, hint none


# ---- the rule ----------------------------------------------------------------------------------------
def header_bytes(nc):
    """Bytes that the 17 + 3 nc bits of a dynamic block's fixed fields and code-length-code lengths occupy."""
    return (17 + 3 * nc + 7) // 8


def probe_ok(data, p):
    """Does position p survive?  Bits are read LSB-first from byte p."""
    n = len(data)
    if p + header_bytes(4) > n:   # nc >= 4: no header fits (and bits 13-16 may lie past the end)
        return False
    v = int.from_bytes(data[p:p + 3], "little")
    if (v >> 1) & 3 != 2:                              # 1. BTYPE dynamic, BFINAL either
        return False
    if (v >> 3) & 31 > 29 or (v >> 8) & 31 > 29:       # 2. HLIT, HDIST
        return False
    nc = ((v >> 13) & 15) + 4
    if p + header_bytes(nc) > n:                       # 3. the whole header inside the file
        return False
    v = int.from_bytes(data[p:p + header_bytes(nc)], "little") >> 17
    kraft = 0
    for i in range(nc):                                # 4. a complete code-length code
        l = (v >> (3 * i)) & 7
        if l:
            kraft += 1 << (7 - l)
    return kraft == 128


def positions(data):
    """The surviving positions, ascending: what k_probe_ordered reports ([p for p in range(n) if probe_ok(data, p)],
    vectorised)."""
    n = len(data)
    if n < 4:
        return []
    b = np.concatenate((np.frombuffer(data, dtype=np.uint8), np.zeros(12, dtype=np.uint8))).astype(np.uint64)
    lo16 = b[:n] | (b[1:n + 1] << np.uint64(8))
    cheap = (((lo16 >> np.uint64(1)) & np.uint64(3)) == 2) & (((lo16 >> np.uint64(3)) & np.uint64(31)) <= 29) & \
            (((lo16 >> np.uint64(8)) & np.uint64(31)) <= 29)
    p = np.nonzero(cheap)[0].astype(np.int64)
    p = p[p + 4 <= n]
    lo = np.zeros(len(p), dtype=np.uint64)
    for k in range(8):
        lo |= b[p + k] << np.uint64(8 * k)
    hi = np.zeros(len(p), dtype=np.uint64)
    for k in range(4):
        hi |= b[p + 8 + k] << np.uint64(8 * k)
    nc = ((lo >> np.uint64(13)) & np.uint64(15)).astype(np.int64) + 4
    fits = p + (17 + 3 * nc + 7) // 8 <= n
    u = (lo >> np.uint64(17)) | (hi << np.uint64(47))
    kraft = np.zeros(len(p), dtype=np.int64)
    for i in range(19):
        l = ((u >> np.uint64(3 * i)) & np.uint64(7)).astype(np.int64)
        kraft += np.where((i < nc) & (l > 0), 128 >> l, 0)
    return [int(x) for x in p[fits & (kraft == 128)]]


# ---- hand-built headers --------------------------------------------------------------------------------
def complete_lengths(nc, r):
    """nc code-length-code lengths (0..7) whose non-zero ones form a complete code, zeros scattered among them."""
    ls = [1, 1]
    want = r.randrange(2, nc + 1)
    while len(ls) < want:
        short = [k for k, l in enumerate(ls) if l < 7]
        if not short:
            break
        k = r.choice(short)
        ls[k] += 1
        ls.append(ls[k])
    ls += [0] * (nc - len(ls))
    r.shuffle(ls)
    return ls


def header(nc, r, bfinal=0, hlit=None, hdist=None, lens=None):
    """The header_bytes(nc) bytes of a dynamic block's start that survives the probe (unless the arguments say
    otherwise); the last byte's spare bits are random."""
    hlit = r.randrange(30) if hlit is None else hlit
    hdist = r.randrange(30) if hdist is None else hdist
    lens = complete_lengths(nc, r) if lens is None else lens
    v = bfinal | (2 << 1) | (hlit << 3) | (hdist << 8) | ((nc - 4) << 13)
    for i, l in enumerate(lens):
        v |= l << (17 + 3 * i)
    nb = header_bytes(nc)
    v |= r.getrandbits(8 * nb - (17 + 3 * nc)) << (17 + 3 * nc)
    return v.to_bytes(nb, "little")


def skewed(seed, nbytes):
    """Bytes from a small, skewed alphabet without long repeats: even a few hundred of them make zlib choose a
    dynamic block."""
    r = random.Random(seed)
    return bytes(r.choice(b"eeeeeeeeettttttaaaaaooooiiinnsh r,d") for _ in range(nbytes))


# ---- pre-drop, acceptance, merge ----------------------------------------------------------------------------
def pre_drop(pos, records):
    """The survivors that lie in no record made before; records = [(offset, hull)]."""
    return [p for p in pos if not any(o <= p < o + h for o, h in records)]


def accept(data, p):
    """-> None, or (consumed, produced) of the raw stream that starts at p, ends inside the file and produces
    PROBE_MIN_OUT bytes or more (and fewer than 2^31)."""
    r = zraw.inflate_raw(data[p:])
    if r is None or not PROBE_MIN_OUT <= len(r[1]) < 1 << 31:
        return None
    return r[0], len(r[1])


def probe_records(data, records, stats=None):
    """The records the probe adds to those made before, records = [(offset, hull)]:
    [(offset, comp_len, infl_len, 24)] ascending."""
    pos = positions(data)
    todo = pre_drop(pos, records)
    out, end, accepted = [], 0, 0
    for p in todo:
        a = accept(data, p)
        if a is None:
            continue
        accepted += 1
        consumed, produced = a
        if any(o < p + consumed and p < o + h for o, h in records):   # meets a record made before
            continue
        if p < end:                                                   # starts inside the one kept before it
            continue
        end = p + consumed
        out.append((p, consumed, produced, TYPE))
    if stats is not None:
        stats.update(survivors=len(pos), decoded=len(todo), accepted=accepted, kept=len(out))
    return out


# ---- the walk ----------------------------------------------------------------------------------------------
def candidates():
    return zraw.candidates(zraw.HINT_NONE)


def rule(body, inflated, **opts):
    """The raw walk's rule on a probe record (no hint): None, or dict(level, window, memlevel, ident, diff_pos,
    diff_val)."""
    return zraw.rule(body, inflated, zraw.HINT_NONE, **opts)
