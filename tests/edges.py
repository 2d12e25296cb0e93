"""Seeded inputs that stand exactly on the library's size-class and window thresholds.

The library picks kernels, LDS sizes and code paths by thresholds on a stream's length and window:
the k_buckets_sort classes of padded length 4096 .. 20480 and 65472, the 16-bit bucket kernels up to 65535 and
k_buckets from 65536; the k_match_lds classes of 4096 .. 49152 staged bytes and the 16320-position ranges past
them; the no-slide walks up to wsize + MAX_DIST, replay up to MAX_DIST, the hash head that is walked at distance
exactly MAX_DIST where a chain successor is not; blocks of lit_bufsize - 1 symbols; deflate_stored's cuts; and
k_inflate<4096>'s far copies past distance 4032, its flush every 2048 bytes and the 64 KiB arena slot.  Every
other input of the suite has a random length; these have lengths n - 1, n, n + 1 around each threshold.

items() -> (Item(family, tag, data, level, window, memlevel, strategy), ...), default strategy:
  D1  class edges at windowBits 15: LENGTHS_D1 x {zeros, per3, text, text_run} x levels {1, 3, 4, 6, 9} x
      memLevels {1, 8, 9} (1620 items).  zeros puts a whole stream into one hash bucket.
  D2  window edges: for w in 9..15, W = 2^w, MD = W - 262 (MAX_DIST), the 13 lengths of d2_lengths(w) x
      {periodic random block of MD - 1, MD and MD + 1 bytes: levels {1, 2, 3, 4, 6, 9} x memLevels {1, 9};
       periodic text block of MD bytes, zeros, text: three (level, memLevel) pairs each, rotated}.
  D3  block ends: for every memLevel m, L = 2^(m + 6) = lit_bufsize, uniq3 (no trigram twice: n literals at
      every level) of L - 2, L - 1, L, L + 1, 2 (L - 1), 2 (L - 1) + 1 bytes at levels {1, 4, 9} and windows
      {9, 15}; and level 0 with B = min(65535, 4 L - 5): text of B - 1, B, B + 1, 2 B, 2 B + 1 bytes at
      windows {9, 12, 15}.
  D4  neighbours: pairs (A, B) that follow each other in the batch; A ends in a match that reaches its last
      byte, at a multiple of 256, and B goes on with the bytes that match's source goes on with.
strategy_items() -> D5: the D3 uniq3 payloads at their memLevel, and zeros / text_run / gradient of the lengths
      W + MD - 1 .. W + MD + 2, 2 W, 2 W + 1 at memLevels {1, 9}; windows {9, 12, 15}, level 6, under
      Z_FILTERED, Z_HUFFMAN_ONLY and Z_RLE.
inflate_payloads() -> I1: per P of DIST_PS a payload of i % 67 random bytes and a random block of P bytes
      repeated over 2 P + 300 + 37 (i % 13) bytes: its stream copies at distance exactly P, through every phase
      of the 4 KiB ring.  inflate_cases(stream, i): the stream, the stream and 7 more bytes, three seeded cuts.
e2e_file() -> the I1 streams, streams of the inflated lengths E2E_SIZES and the D4 pairs in one file.
walk_symbols() reads a zlib stream's blocks, literal counts and (distance, length) pairs, for the premises that
tests/test_edges_cpu.py asserts.  tests/golden/edges.json (make_edges.py) pins zlib 1.2.8's result on all of it.
"""
import collections
import functools
import hashlib
import json
import os
import random

import _libs
import nearmiss

Item = collections.namedtuple("Item", "family tag data level window memlevel strategy")
Block = collections.namedtuple("Block", "btype final nlit matches tail")
# matches: [(distance, length)]; tail: the block's last symbol is a match
Z_DEFAULT, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE = 0, 1, 2, 3
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edges.json")
SEED = 20261020

LENGTHS_D1 = (4095, 4096, 4097, 8192, 8193, 12288, 12289, 16384, 16385, 20480, 20481, 24576, 24577, 32768, 32769,
              40960, 40961, 49152, 49153, 65279, 65280, 65281, 65472, 65473, 65535, 65536, 65537)
LEVELS_D1, MEMLEVELS_D1 = (1, 3, 4, 6, 9), (1, 8, 9)
LEVELS_D2, MEMLEVELS_D2 = (1, 2, 3, 4, 6, 9), (1, 9)
N_D1 = len(LENGTHS_D1) * 4 * len(LEVELS_D1) * len(MEMLEVELS_D1)
N_D2 = 7 * 13 * (3 * len(LEVELS_D2) * len(MEMLEVELS_D2) + 3 * 3)
N_D3 = 9 * (6 * 3 * 2 + 5 * 3)
N_D4 = 7 * 3 * 2
N_D5 = (9 * 6 + 6 * 3 * 2) * 3 * 3
DIST_PS = tuple(range(4020, 4111)) + (259, 260, 2047, 2048, 2049, 8191, 8192, 8193, 16384, 32505, 32506)
E2E_SIZES = (2047, 2048, 2049, 4095, 4096, 4097, 16320, 49152, 49153, 65279, 65280, 65281, 65472, 65473, 65535,
             65536, 65537, 67584, 98304, 131072)
D4_BLOCK = 3000
D4_TEXT_CUTS = (3328, 6656, 9216)
D4_NEXT = 5000


def sha16(b):
    return hashlib.sha256(b).hexdigest()[:16]


def first_diff(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


# ---- contents ---------------------------------------------------------------------------------------
def zeros(seed, n):
    return bytes(n)


def per3(seed, n):
    return (b"abc" * (n // 3 + 1))[:n]


def _text(r, n):
    """Exactly n bytes (_libs.text gives n - 1 when its last word ends at n)."""
    return _libs.text(r, n + 1)[:n]


def text(seed, n):
    return _text(random.Random(seed), n)


def text_run(seed, n):
    """Text whose last min(n, 700) bytes are one run of zeros: the stream ends inside a long match."""
    k = min(n, 700)
    return text(seed, n - k) + bytes(k)


def periodic(seed, n, period, kind):
    """A random ("rnd") or text ("txt") block of `period` bytes, repeated."""
    r = random.Random(seed)
    blk = r.randbytes(period) if kind == "rnd" else _text(r, period)
    return (blk * (n // period + 1))[:n]


@functools.lru_cache(maxsize=None)
def uniq3(seed, n):
    """Random bytes in which no trigram occurs twice (the next byte is drawn again while its trigram was seen):
    deflate finds no match, so every level emits n literals."""
    r, seen, out = random.Random(seed), set(), bytearray()
    while len(out) < n:
        b = r.randrange(256)
        if len(out) >= 2:
            t = (out[-2] << 16) | (out[-1] << 8) | b
            if t in seen:
                continue
            seen.add(t)
        out.append(b)
    return bytes(out)


def gradient(seed, n):
    """Rows of a smooth image after a scanline filter: a filter byte, then small deltas (many zeros, short
    matches), as a PNG's IDAT payload before compression."""
    r, out = random.Random(seed), bytearray()
    width = r.randrange(48, 360)
    while len(out) < n:
        out.append(r.randrange(3))
        out += bytes(r.choice((0, 0, 0, 1, 255, 2, 254, 3)) for _ in range(width))
    return bytes(out[:n])


# ---- the families -----------------------------------------------------------------------------------
def d2_lengths(w):
    W = 1 << w
    MD = W - 262
    return (MD, MD + 1, MD + 2, MD + 3, W, W + MD - 1, W + MD, W + MD + 1, W + MD + 2, 2 * W - 1, 2 * W, 2 * W + 1,
            2 * W + MD + 1)


def _d1(add):
    k = 0
    for n in LENGTHS_D1:
        for gen in (zeros, per3, text, text_run):
            d = gen(SEED + 1000 + k, n)
            k += 1
            for lv in LEVELS_D1:
                for m in MEMLEVELS_D1:
                    add("D1", gen.__name__, d, lv, 15, m)


def _d2(add):
    k = 0
    for w in range(9, 16):
        MD = (1 << w) - 262
        for n in d2_lengths(w):
            for off in (-1, 0, 1):
                d = periodic(SEED + 2000 + 16 * w + off, n, MD + off, "rnd")   # one block a window, cut to each length
                for lv in LEVELS_D2:
                    for m in MEMLEVELS_D2:
                        add("D2", "rnd%+d" % off, d, lv, w, m)
            for tag, d in (("txt+0", periodic(SEED + 2500 + w, n, MD, "txt")), ("zeros", zeros(0, n)),
                           ("text", text(SEED + 2600 + w, n))):
                for j in range(3):
                    add("D2", tag, d, 1 + (k + 3 * j) % 9, w, 1 + (k + 4 * j) % 9)
                k += 1


def d3_lengths(m):
    L = 1 << (m + 6)
    return (L - 2, L - 1, L, L + 1, 2 * (L - 1), 2 * (L - 1) + 1)


def stored_max(m):
    """deflate_stored's max_block_size (Z/deflate.c:1477-1481): pending_buf_size - 5, 65535 at most."""
    return min(65535, 4 * (1 << (m + 6)) - 5)


def _d3(add):
    for m in range(1, 10):
        for n in d3_lengths(m):
            d = uniq3(SEED + 3000 + m, n)
            for lv in (1, 4, 9):
                for w in (9, 15):
                    add("D3", "uniq3", d, lv, w, m)
        B = stored_max(m)
        for w in (9, 12, 15):
            for n in (B - 1, B, B + 1, 2 * B, 2 * B + 1):
                add("D3", "stored", text(SEED + 3100 + m, n), 0, w, m)


@functools.lru_cache(maxsize=None)
def d4_pairs():
    """[(tag, big, cut)]: A = big[:cut], B = big[cut:cut + D4_NEXT].  The text pairs repeat a block of D4_BLOCK
    bytes, so the match that ends A (from D4_BLOCK back) would go on through B's first bytes."""
    big = text(SEED + 4000, D4_BLOCK) * 6
    out = [("text", big, cut) for cut in D4_TEXT_CUTS]
    for cut in (4096, 65536):
        out.append(("zeros", zeros(0, cut + D4_NEXT), cut))
        out.append(("per3", per3(0, cut + D4_NEXT), cut))
    assert all(cut % 256 == 0 and len(big) >= cut + D4_NEXT for _, big, cut in out)
    return out


def _d4(add):
    pairs = ((1, 8), (6, 9), (9, 1), (3, 9), (4, 1), (8, 8), (2, 1), (7, 9), (5, 8))   # every three: one of levels 1-3
    for k, (tag, big, cut) in enumerate(d4_pairs()):
        for j in range(3):
            lv, m = pairs[(3 * k + j) % 9]
            add("D4", tag + "A", big[:cut], lv, 15, m)
            add("D4", tag + "B", big[cut:cut + D4_NEXT], lv, 15, m)


@functools.lru_cache(maxsize=None)
def items():
    """Families D1-D4 in this order; an item's position is its key in the fixture."""
    out = []

    def add(family, tag, data, level, window, memlevel):
        out.append(Item(family, tag, data, level, window, memlevel, Z_DEFAULT))

    for fam, n in ((_d1, N_D1), (_d2, N_D2), (_d3, N_D3), (_d4, N_D4)):
        before = len(out)
        fam(add)
        assert len(out) - before == n, (fam.__name__, len(out) - before)
    return tuple(out)


def family(name):
    """[(position in items(), item)] of one family."""
    return [(k, it) for k, it in enumerate(items()) if it.family == name]


@functools.lru_cache(maxsize=None)
def strategy_items():
    out = []
    for strat in (Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE):
        for w in (9, 12, 15):
            for m in range(1, 10):
                for n in d3_lengths(m):
                    out.append(Item("D5", "uniq3", uniq3(SEED + 3000 + m, n), 6, w, m, strat))
            W = 1 << w
            MD = W - 262
            for k, n in enumerate((W + MD - 1, W + MD, W + MD + 1, W + MD + 2, 2 * W, 2 * W + 1)):
                for gen in (zeros, text_run, gradient):
                    d = gen(SEED + 5000 + 8 * w + k, n)
                    for m in (1, 9):
                        out.append(Item("D5", gen.__name__, d, 6, w, m, strat))
    assert len(out) == N_D5
    return tuple(out)


def label(it):
    return "%s %s n=%d level=%d window=%d memLevel=%d strategy=%d" % (it.family, it.tag, len(it.data), it.level,
                                                                     it.window, it.memlevel, it.strategy)


def describe(it, got, want):
    """A failing item as the deflate tests report it, in one string (pytest shortens long tuples)."""
    return "%s: first difference at byte %d (lengths %d / %d)" % (label(it), first_diff(got, want), len(got), len(want))


# ---- inflate ----------------------------------------------------------------------------------------
INFLATE_PARAMS = ((6, 15, 8), (1, 15, 8), (9, 15, 8), (4, 15, 8))


@functools.lru_cache(maxsize=None)
def inflate_payloads():
    """[(P, payload, (level, window, memlevel))] of family I1."""
    r = random.Random(SEED + 6000)
    out = []
    for i, P in enumerate(DIST_PS):
        pre = r.randbytes(i % 67)
        out.append((P, pre + periodic(SEED + 6100 + i, 2 * P + 300 + 37 * (i % 13), P, "rnd"), INFLATE_PARAMS[i % 4]))
    return out


def inflate_cases(s, i):
    """[(tag, bytes)]: the whole stream, the stream and 7 bytes of garbage, the stream cut at three seeded points
    (inside the header or first block, anywhere, inside the last 8 bytes)."""
    r = random.Random(SEED + 6500 + i)
    cuts = (r.randrange(1, 40), r.randrange(40, len(s) - 8), len(s) - r.randrange(1, 9))
    return [("whole", s), ("garbage", s + r.randbytes(7))] + [("cut%d" % c, s[:c]) for c in cuts]


# ---- the end-to-end file ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e2e_payloads():
    """[(tag, payload, level, window, memlevel)] in file order: I1, the size edges, the D4 pairs."""
    out = [("dist%d" % P, d, lv, w, m) for P, d, (lv, w, m) in inflate_payloads()]
    for i, n in enumerate(E2E_SIZES):
        for j, gen in enumerate((text, zeros, per3)):
            k = 3 * i + j
            out.append(("size%d%s" % (n, gen.__name__), gen(SEED + 7000 + k, n), (6, 9, 1, 3, 4, 8)[k % 6],
                        (15, 14, 13, 12)[k % 4] if n <= 65537 else 15, (8, 9, 1, 5, 2)[k % 5]))
    for k, (tag, big, cut) in enumerate(d4_pairs()):
        lv, m = ((6, 8), (1, 9), (9, 1))[k % 3]
        out.append(("nbrA%s%d" % (tag, cut), big[:cut], lv, 15, m))
        out.append(("nbrB%s%d" % (tag, cut), big[cut:cut + D4_NEXT], lv, 15, m))
    return out


def e2e_file(deflate=None):
    """-> (file bytes, [(offset, stream length, tag, inflated length)]).  The streams are `deflate`'s (the
    oracle's by default; the recorder passes the real zlib's), with 5-40 bytes of text between them.  The
    reference reads the file in chunks of 524288 bytes (524287 new ones from the second on) and loses a stream
    that lies across a chunk's end (tests/golden/cases.json has that case); here the fill before such a stream
    is as long as it takes to start the stream in the next chunk."""
    deflate = deflate or (lambda d, lv, w, m: _libs.ora_deflate(d, lv, w, m)[0])
    r = random.Random(SEED + 8000)
    parts, recs, pos = [], [], 0
    for tag, d, lv, w, m in e2e_payloads():
        fill = _libs.text(r, r.randrange(5, 40))
        s = deflate(d, lv, w, m)
        at = pos + len(fill)
        end = next(b for b in range(524288, 1 << 30, 524287) if b > at)    # the end of the chunk the stream starts in
        if at + len(s) + 8 > end:
            fill += _libs.text(r, end + 8 - at)
        recs.append((pos + len(fill), len(s), tag, len(d)))
        parts += [fill, s]
        pos += len(fill) + len(s)
    parts.append(_libs.text(r, 33))
    return b"".join(parts), recs


# ---- a deflate symbol walker (RFC 1951) -------------------------------------------------------------
_LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
          6145, 8193, 12289, 16385, 24577)
_FAST = 10


def _fast_table(canon):
    """canon: nearmiss._canon's {(length, code): symbol}.  -> a list indexed by the next _FAST stream bits
    (codes lie in the stream most significant bit first): symbol << 4 | length, or 0 for a longer code."""
    tab = [0] * (1 << _FAST)
    for (n, code), sym in canon.items():
        if n <= _FAST:
            rev = int(format(code, "0%db" % n)[::-1], 2)
            for k in range(rev, 1 << _FAST, 1 << n):
                tab[k] = (sym << 4) | n
    return tab


_FIXED = (nearmiss._FIXED_LL, _fast_table(nearmiss._FIXED_LL), nearmiss._FIXED_D, _fast_table(nearmiss._FIXED_D))


def walk_symbols(s):
    """The blocks of zlib stream `s` as [Block(btype, final, literals, [(distance, length)], tail)]; a stored block's
    bytes count as literals.  nearmiss.walk_blocks with the symbols kept; raises ValueError on a stream that
    does not end at its Adler-32."""
    data = bytes(s) + bytes(16)
    pos, acc, cnt = 2, 0, 0    # next byte to load; the bits loaded and not yet used

    def slow(canon):
        code = 0
        for n in range(1, 16):
            code = (code << 1) | ((acc >> (n - 1)) & 1)
            if (n, code) in canon:
                return (canon[(n, code)] << 4) | n
        raise ValueError("bad code")

    blocks = []
    while True:
        if cnt < 32:
            acc |= int.from_bytes(data[pos:pos + 4], "little") << cnt
            pos += 4
            cnt += 32
        final, bt = acc & 1, (acc >> 1) & 3
        acc >>= 3
        cnt -= 3
        if bt == 0:
            at = pos - (cnt >> 3)      # the byte boundary: whole unused bytes go back
            ln, nl = data[at] | (data[at + 1] << 8), data[at + 2] | (data[at + 3] << 8)
            if ln ^ nl != 0xffff:
                raise ValueError("stored LEN/NLEN")
            pos, acc, cnt = at + 4 + ln, 0, 0
            blocks.append(Block(0, final, ln, [], False))
        elif bt == 3:
            raise ValueError("block type 3")
        else:
            lcanon, lfast, dcanon, dfast = _FIXED
            if bt == 2:
                def bits(n):      # n <= 16: a code-length code and its repeat count take 14 bits
                    nonlocal acc, cnt, pos
                    if cnt < 16:
                        acc |= int.from_bytes(data[pos:pos + 4], "little") << cnt
                        pos += 4
                        cnt += 32
                    v = acc & ((1 << n) - 1)
                    acc >>= n
                    cnt -= n
                    return v

                nlen, ndist, ncode = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(ncode):
                    cl[nearmiss._CLORDER[i]] = bits(3)
                ct, lens = nearmiss._canon(cl), []
                while len(lens) < nlen + ndist:
                    bits(0)
                    c = slow(ct)
                    c, _ = c >> 4, bits(c & 15)
                    if c < 16:
                        lens.append(c)
                    elif c == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    elif c == 17:
                        lens += [0] * (3 + bits(3))
                    else:
                        lens += [0] * (11 + bits(7))
                lcanon, dcanon = nearmiss._canon(lens[:nlen]), nearmiss._canon(lens[nlen:nlen + ndist])
                lfast, dfast = _fast_table(lcanon), _fast_table(dcanon)
            nlit, matches, mask, tail = 0, [], (1 << _FAST) - 1, False
            while True:
                if cnt < 48:      # a length and a distance take at most 15 + 5 + 15 + 13 bits
                    acc |= int.from_bytes(data[pos:pos + 4], "little") << cnt
                    pos += 4
                    cnt += 32
                e = lfast[acc & mask] or slow(lcanon)
                acc >>= e & 15
                cnt -= e & 15
                sym = e >> 4
                if sym < 256:
                    nlit += 1
                    tail = False
                elif sym == 256:
                    break
                else:
                    if sym > 285:
                        raise ValueError("bad length symbol")
                    eb = nearmiss._LEXT[sym - 257]
                    length = _LBASE[sym - 257] + (acc & ((1 << eb) - 1))
                    acc >>= eb
                    cnt -= eb
                    e = dfast[acc & mask] or slow(dcanon)
                    acc >>= e & 15
                    cnt -= e & 15
                    if (e >> 4) > 29:
                        raise ValueError("bad distance symbol")
                    eb = nearmiss._DEXT[e >> 4]
                    matches.append((_DBASE[e >> 4] + (acc & ((1 << eb) - 1)), length))
                    acc >>= eb
                    cnt -= eb
                    tail = True
            blocks.append(Block(bt, final, nlit, matches, tail))
        if final:
            break
    if pos - (cnt >> 3) != len(s) - 4:
        raise ValueError("stream does not end at its Adler-32")
    return blocks


def matches_of(s):
    return [m for b in walk_symbols(s) for m in b.matches]


# ---- the fixture ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)
