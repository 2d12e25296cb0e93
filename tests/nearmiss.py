"""Seeded near-miss streams: zlib streams that some trial reproduces ALMOST exactly.

Every other input of the suite is either an exact one-shot zlib output (it stops at its first full
match), one byte off at offset 1 (`near`) or hopeless (the PNG-like Z_FILTERED streams).  The streams
here miss their best trial by 1 to ~140 bytes, deep in the stream or past the end of the trial's
output, so the diff list (main.cpp:699-714), the recompress threshold (main.cpp:454), the
first-improving rule over a whole trial list (main.cpp:685-700) and the tolerance stop decide them.
Python's zlib and byte surgery only; every mutated stream is asserted to decompress to its data.

Families (one or two files each, a few dozen streams per file, 0-40 noise bytes between them):
  storedpad  random bytes at memLevel 1-3: all stored blocks; the five padding bits of k block-header
             bytes (never the first) are set, so exactly those k bytes differ from the right trial.
  tailflush  compress(d) + flush(F) + flush() for F in SYNC, FULL, PARTIAL, Z_BLOCK: the original is
             longer than every trial, so the diff list ends in its tail (i >= out_len).
  midflush   one Z_SYNC_FLUSH t bytes before the end at memLevel 1-2: the blocks before the flushed one
             stay identical, the rest differs; t is drawn so that the mismatch count against the
             same-parameter one-shot stream lands on both sides of recomp_tresh = 128.
  eobpad     the spare bits after the last end-of-block code are set (one diff at C - 5); half of the
             streams also get another FLEVEL (datagen._relevel): two diffs, at both ends.
  mixed      text with 1-3 KB random stretches at memLevel 1-2: stored blocks inside dynamic-block
             streams; the padding bits after k of their 3-bit headers are set.
  strategy   Z_FILTERED, Z_RLE, Z_HUFFMAN_ONLY, Z_FIXED at 40 / 400 / 3000 B, unmodified.
  tolstop    short streams whose first trial (level 5) misses by d0 = 1, 2, 3, 10, 11 or 12 bytes and whose
             own level, an exact match, comes a few trials later: whether the sweep stops at the first
             (ident + mismatch_tol >= C, main.cpp:700) changes the chosen parameters and the diff list.
  wrongwin   text deflated with a 1-2 KiB window under a header that claims 8-32 KiB: only the brute-window
             phase (main.cpp:590) finds the trial that matches, two header bytes off.
tests/golden/nearmiss.json (tools/make_nearmiss_golden.py) pins the real reference's ATZ1 on every file.
"""
import collections
import functools
import random
import zlib

import numpy as np

import _libs
import atzfile
from antiz_amd import datagen

Stream = collections.namedtuple("Stream", "offset length family tag data_len pads")
# pads: the byte offsets (inside the stream) whose padding bits were set, in rising order

FLUSHES = {"sync": zlib.Z_SYNC_FLUSH, "full": zlib.Z_FULL_FLUSH, "partial": 1, "block": 5}   # zlib.h
STRATEGIES = {"filtered": zlib.Z_FILTERED, "rle": zlib.Z_RLE, "huffman": zlib.Z_HUFFMAN_ONLY,
              "fixed": zlib.Z_FIXED}
PAD_KS = (1, 2, 3, 16, 17, 127, 128, 129, 140)
SEED = 20261019
NAMES = ("storedpad_small", "storedpad_big", "tailflush", "midflush", "eobpad", "mixed", "strategy", "tolstop",
         "wrongwin")     # the files of the corpus (static: tests parametrize over them without generating it)


# ---- a deflate block walker (RFC 1951): bit positions and block types only, no output -----------------
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]          # extra bits of length codes 257..285
_DEXT = [0, 0] + [d // 2 - 1 for d in range(2, 30)]                             # extra bits of distance codes 0..29
_CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _canon(lens):
    """{(code length, code): symbol} of the canonical Huffman code with these lengths (RFC 1951 3.2.2)."""
    tab, code = {}, 0
    for n in range(1, 16):
        for sym, ln in enumerate(lens):
            if ln == n:
                tab[(n, code)] = sym
                code += 1
        code <<= 1
    return tab


_FIXED_LL = _canon([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_FIXED_D = _canon([5] * 30)


def walk_blocks(s):
    """The deflate blocks of zlib stream `s`: [(header bit, btype, pad_lo bit, pad_hi bit, end bit)].
    pad_lo..pad_hi are the ignored bits between a stored block's header and its LEN field (empty for
    the other types); the last block's end bit is where the padding before the Adler-32 starts."""
    pos = 16

    def bits(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= ((s[pos >> 3] >> (pos & 7)) & 1) << i
            pos += 1
        return v

    def sym(tab):
        nonlocal pos
        code = 0
        for n in range(1, 16):
            code = (code << 1) | ((s[pos >> 3] >> (pos & 7)) & 1)
            pos += 1
            if (n, code) in tab:
                return tab[(n, code)]
        raise ValueError("bad code")

    blocks = []
    while True:
        p0 = pos
        final, bt = bits(1), bits(2)
        lo = hi = pos
        if bt == 0:
            pos = hi = (pos + 7) & ~7
            ln, nl = bits(16), bits(16)
            if ln ^ nl != 0xffff:
                raise ValueError("stored LEN/NLEN")
            pos += 8 * ln
        elif bt == 3:
            raise ValueError("block type 3")
        else:
            ll, dd = _FIXED_LL, _FIXED_D
            if bt == 2:
                nlen, ndist, ncode = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(ncode):
                    cl[_CLORDER[i]] = bits(3)
                ct, lens = _canon(cl), []
                while len(lens) < nlen + ndist:
                    c = sym(ct)
                    if c < 16:
                        lens.append(c)
                    elif c == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    elif c == 17:
                        lens += [0] * (3 + bits(3))
                    else:
                        lens += [0] * (11 + bits(7))
                ll, dd = _canon(lens[:nlen]), _canon(lens[nlen:nlen + ndist])
            while True:
                c = sym(ll)
                if c == 256:
                    break
                if c > 256:
                    pos += _LEXT[c - 257]
                    d = sym(dd)      # (not `pos += _DEXT[sym(dd)]`: sym() moves pos)
                    pos += _DEXT[d]
        blocks.append((p0, bt, lo, hi, pos))
        if final:
            break
    if (pos + 7) // 8 != len(s) - 4:
        raise ValueError("stream does not end at its Adler-32")
    return blocks


def _set_bits(b, lo, hi):
    """Set bits lo..hi-1 (all inside one byte) of bytearray b; returns that byte's offset."""
    assert lo < hi and (lo >> 3) == ((hi - 1) >> 3)
    for p in range(lo, hi):
        b[p >> 3] |= 1 << (p & 7)
    return lo >> 3


def _z(data, c, w, m, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(c, zlib.DEFLATED, w, m, strategy)
    return co.compress(data) + co.flush()


def mismatches(orig, trial):
    """The reference's count for one trial (main.cpp:699-714): differing bytes of the common prefix plus
    the original's bytes past the trial's end."""
    sm = min(len(orig), len(trial))
    a, b = np.frombuffer(orig, np.uint8, sm), np.frombuffer(trial, np.uint8, sm)
    return int(np.count_nonzero(a != b)) + (len(orig) - sm)


# ---- families: each returns (stream bytes, data, tag, pads) -------------------------------------------
def stored_headers(s):
    """Offsets of the block-header bytes of an all-stored zlib stream, by its LEN/NLEN fields from
    offset 2 to the Adler-32 trailer; None if the stream is not all stored blocks."""
    at, hdr = 2, []
    while True:
        if at + 5 > len(s) - 4 or s[at] & 0xfe:
            return None
        ln = s[at + 1] | (s[at + 2] << 8)
        if (ln ^ (s[at + 3] | (s[at + 4] << 8))) != 0xffff:
            return None
        hdr.append(at)
        last = s[at] & 1
        at += 5 + ln
        if last:
            return hdr if at == len(s) - 4 else None


def storedpad(r, k, early=False):
    """early: the pads are the first k headers after the first and a dozen blocks follow them, in a stream
    longer than two windows (no symbol replay): a trial that is given up at its k-th mismatch is given up
    well before its end."""
    while True:
        m = 1 if k > 17 else r.randint(1, 3)
        nblk = k + 1 + (12 if early else r.randint(0, 3 if k > 17 else 6))
        data = r.randbytes(nblk * ((1 << (m + 6)) - 1) + r.randint(0, 100))
        c, w = r.randint(1, 9), r.randint(10, 13 if early else 15)
        s = _z(data, c, w, m)
        hdr = stored_headers(s)
        if hdr is None or len(hdr) < nblk:
            continue
        pads = hdr[1:k + 1] if early else sorted(r.sample(hdr[1:], k))
        b = bytearray(s)
        for p in pads:
            b[p] |= 0xf8
        return bytes(b), data, "k%d%s" % (k, "e" if early else ""), tuple(pads)


def tailflush(r, kind):
    data = _libs.text(r, r.choice([r.randint(300, 3000), r.randint(3000, 20000)]))
    co = zlib.compressobj(r.randint(1, 9), zlib.DEFLATED, r.randint(10, 15), r.randint(1, 9))
    return co.compress(data) + co.flush(FLUSHES[kind]) + co.flush(), data, kind, ()


def midflush(r, band):
    """band: (lo, hi) for the mismatch count against the same-parameter one-shot stream, or None."""
    while True:
        data = _libs.text(r, r.randint(6000, 16000))
        c, w, m = r.randint(1, 9), r.randint(10, 15), r.randint(1, 2)
        one = _z(data, c, w, m)
        ts = list(range(1, 400 if band is None else 160))
        r.shuffle(ts)
        for t in ts[:40 if band else 1]:
            co = zlib.compressobj(c, zlib.DEFLATED, w, m)
            s = co.compress(data[:len(data) - t]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(data[len(data) - t:]) + co.flush()
            if band is None or band[0] <= mismatches(s, one) <= band[1]:
                return s, data, "t%d" % t, ()


def eobpad(r, relevel):
    while True:
        data = _libs.text(r, r.randint(300, 6000))
        s = _z(data, r.randint(1, 9), r.randint(10, 15), r.randint(1, 9))
        end = walk_blocks(s)[-1][4]
        if end % 8 == 0:      # the end-of-block code ends on a byte boundary: no spare bits
            continue
        b = bytearray(s)
        at = _set_bits(b, end, (end + 7) & ~7)
        assert at == len(s) - 5
        s = bytes(b)
        if relevel:
            s = datagen._relevel(s, (((s[1] >> 6) & 3) + r.randint(1, 3)) % 4)
        return s, data, "relevel" if relevel else "plain", (at,)


def mixed(r, k):
    while True:
        parts = []
        for _ in range(r.randint(2, 3)):
            parts.append(_libs.text(r, r.randint(800, 4000)))
            parts.append(r.randbytes(r.randint(1000, 3000)))
        parts.append(_libs.text(r, r.randint(200, 2000)))
        data = b"".join(parts)
        s = _z(data, r.randint(1, 9), r.randint(10, 15), r.randint(1, 2))
        blocks = walk_blocks(s)
        sites = [(lo, hi) for (_, bt, lo, hi, _) in blocks[1:] if bt == 0 and hi > lo]
        if len(sites) < k or all(bt == 0 for _, bt, _, _, _ in blocks):
            continue
        b = bytearray(s)
        pads = sorted(_set_bits(b, lo, hi) for lo, hi in r.sample(sites, k))
        return bytes(b), data, "k%d" % k, tuple(pads)


def strategy(r, name, n):
    data = _libs.text(r, n)
    return _z(data, r.randint(1, 9), r.randint(10, 15), r.randint(1, 9), STRATEGIES[name]), data, "%s%d" % (name, n), ()


def _tolstop_try(seed):
    """A short stream over a small alphabet made at level 2, 3 or 4 with the header of its own class
    (FLEVEL 1), or None.  Its list starts with level 5 at memLevel 8 (main.cpp:510), whose output misses
    it by d0 bytes, and reaches its own level, an exact match, a few trials later: a sweep that stops at
    tolerance >= d0 keeps level 5 and d0 diffs, one that does not ends exact.  -> (stream, data, d0)"""
    r = random.Random(seed)
    alpha = r.choice([b"ab", b"abc", b"abcd", b"abcdefgh"])
    data = bytes(r.choice(alpha) for _ in range(r.randint(40, 400)))
    w, c = r.randint(10, 15), r.randint(2, 4)
    s, first = _z(data, c, w, 8), _z(data, 5, w, 8)
    if len(s) <= 16 or any(_z(data, e, w, 8) == s for e in range(5, c, -1)):
        return None
    return s, data, mismatches(s, first)


def find_tolstop_seeds(targets, each=3, start=0):
    """The search that made TOLSTOP_SEEDS (about one seed in a thousand qualifies)."""
    out, seed = {d: [] for d in targets}, start
    while any(len(v) < each for v in out.values()):
        t = _tolstop_try(seed)
        if t and t[2] in out and len(out[t[2]]) < each:
            out[t[2]].append(seed)
        seed += 1
    return out


# d0 -> seeds, for d0 around the default tolerance (2) and around T = 11 (the tolT / tolT-1 settings)
TOLSTOP_SEEDS = {1: [437, 1494, 11710], 2: [8021, 13175, 27748], 3: [894, 2587, 2739], 10: [1233, 1455, 2153],
                 11: [865, 1663, 3204], 12: [1097, 4452, 4666]}


def tolstop(seed, d0):
    s, data, d = _tolstop_try(seed)
    assert d == d0, (seed, d, d0)
    return s, data, "d%d" % d0, ()


def wrongwin(r):
    """Text deflated with a 1 or 2 KiB window under a header that claims a larger one: every trial at the
    claimed window misses by far, and the brute-window phase finds the real one, two header bytes off."""
    data = _libs.text(r, r.randint(3000, 9000))
    w, claim = r.randint(10, 11), r.randint(13, 15)
    s = _z(data, r.randint(1, 9), w, r.randint(1, 9))
    cmf = ((claim - 8) << 4) | 8
    flg = s[1] & 0xc0
    flg |= (31 - (cmf * 256 + flg) % 31) % 31
    return bytes([cmf, flg]) + s[2:], data, "w%dc%d" % (w, claim), ()


def _file(r, family, items):
    out, streams = bytearray(), []
    for s, data, tag, pads in items:
        assert zlib.decompress(s) == data, (family, tag)
        out += r.randbytes(r.randint(0, 40))
        streams.append(Stream(len(out), len(s), family, tag, len(data), pads))
        out += s
    out += r.randbytes(r.randint(0, 40))
    return bytes(out), streams


@functools.lru_cache(maxsize=None)
def files(seed=SEED):
    """{name: (file bytes, [Stream])}: the corpus, from its seed alone."""
    r = random.Random(seed)
    out = {}
    out["storedpad_small"] = _file(r, "storedpad", [storedpad(r, k) for k in (1, 2, 3) for _ in range(4)] +
                                   [storedpad(r, k) for k in (16, 17) for _ in range(2)])
    out["storedpad_big"] = _file(r, "storedpad", [storedpad(r, k) for k in (127, 127, 128, 128, 129, 129, 140)] +
                                 [storedpad(r, k, early=True) for k in (127, 128, 129)])
    out["tailflush"] = _file(r, "tailflush", [tailflush(r, kind) for _ in range(6) for kind in FLUSHES])
    out["midflush"] = _file(r, "midflush", [midflush(r, band) for band in [(113, 128), (129, 144)] * 6 + [None] * 3])
    out["eobpad"] = _file(r, "eobpad", [eobpad(r, i % 2 == 1) for i in range(24)])
    out["mixed"] = _file(r, "mixed", [mixed(r, k) for k in (3, 5, 20) for _ in range(3)])
    out["strategy"] = _file(r, "strategy", [strategy(r, name, n) for _ in range(2) for name in STRATEGIES
                                            for n in (40, 400, 3000)])
    out["tolstop"] = _file(r, "tolstop", [tolstop(seed, d0) for d0, seeds in TOLSTOP_SEEDS.items() for seed in seeds])
    out["wrongwin"] = _file(r, "wrongwin", [wrongwin(r) for _ in range(8)])
    assert tuple(out) == NAMES
    for name, (data, streams) in out.items():
        assert len(data) <= 400 * 1024 and all(s.length <= 25 * 1024 for s in streams), name
    return out


def mutated_streams():
    """[(stream bytes, data length)] of every stream of the corpus, for the inflate tests."""
    return [(data[s.offset:s.offset + s.length], s.data_len) for data, streams in files().values() for s in streams]


# ---- settings (the reference's command-line flags) ---------------------------------------------------
def settings(T, D):
    """name -> flags; T: the diff count of the tailflush SYNC streams, D: their exact size difference
    (both read from the reference's default run and recorded in nearmiss.json)."""
    return {
        "default": [],
        "tol0": ["--mismatch-tol", "0"],
        "tolT": ["--mismatch-tol", str(T)],
        "tolT-1": ["--mismatch-tol", str(T - 1)],
        "floor_off": ["--mismatch-tol", "200", "--recomp-tresh", "128"],
        "strict_shortcut": ["--recomp-tresh", "16", "--shortcut-len", "64"],
        "recomp0": ["--recomp-tresh", "0"],
        "sizediffD": ["--sizediff-tresh", str(D)],
        "sizediffD-1": ["--sizediff-tresh", str(D - 1)],
        "brute": ["--brute-window"],
        "brute_tol0": ["--brute-window", "--mismatch-tol", "0"],
    }


def flags_kwargs(flags, names=("recomp", "sizediff", "shortcut", "tol", "brute")):
    """Flags -> keyword arguments of _libs.ora_precompress (or, with other names, of antiz_amd.Context)."""
    key = dict(zip(("--recomp-tresh", "--sizediff-tresh", "--shortcut-len", "--mismatch-tol", "--brute-window"), names))
    kw, i = {}, 0
    while i < len(flags):
        if flags[i] == "--brute-window":
            kw[key[flags[i]]] = 1
            i += 1
        else:
            kw[key[flags[i]]] = int(flags[i + 1])
            i += 2
    return kw


def parse_atz1(atz):
    """The stream table of an ATZ1 file: one dict per recompressed stream with its
    offset, comp_len, c, w, m, n_diff, first_diff and the absolute diff positions and values."""
    assert atz[:4] == b"ATZ\x01"
    return [dict(offset=d["off"], comp_len=d["cl"], c=d["c"], w=d["w"], m=d["m"], n_diff=d["nd"], first_diff=d["first_diff"],
                 pos=d["pos"], val=d["val"]) for d in atzfile.parse(atz)[2]]


# ---- the fixture (tests/golden/nearmiss.json) --------------------------------------------------------
def fixture():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nearmiss.json")) as f:
        return json.load(f)


def check_pinned(fx):
    """The corpus is the fixture's, byte for byte (SHA-256 of every file).  The generator depends on the
    interpreter's zlib; with fewer than ten files the rule "at most 10 % of the files may differ" lets none
    differ, so any drift fails here, plainly, rather than weakening the reference pin."""
    import hashlib
    assert fx["seed"] == SEED and tuple(fx["files"]) == NAMES
    bad = [name for name, (data, _) in files().items()
           if hashlib.sha256(data).hexdigest() != fx["files"][name]["input_sha256"]]
    assert not bad, "generator output changed (another zlib?): %s" % bad
