"""Seeded inputs whose Huffman trees are deeper than zlib allows, so that gen_bitlen's length-limit fix-up
(Z/trees.c:531-564) decides the bytes.

Every other input of the suite builds trees that fit: over four of test_gpu.py's deflate tests the fix-up
ran once in 38 926 blocks.  A fix-up with a wrong pop order, depth tie-break, capped-node count or
`m > max_code` skip still yields a valid Huffman code, only not zlib's, so these inputs are compared byte
for byte.  The streams they deflate to carry 15-bit literal/length and distance codes and 7-bit
code-length codes, which k_inflate decodes past its 6-bit root table.

items() -> [Item(name, data, level, window, memlevel, strategy)], families:
  huff_fib   Z_HUFFMAN_ONLY; one block whose byte histogram is 1, 2, 3, 5, ... (F2..F(k+1); the end-of-block
             symbol is the first 1), so the unlimited depth is k: 16, 17, 20.  Alone (<= 63 leaves: the
             register heap of k_deflate's build_tree) and on top of 60-110 flat byte values (the LDS heap);
             two inputs whose first block is such a histogram and whose second is text.
  rle_fib    the same histograms under Z_RLE, runs kept below 3 where possible.
  bl_deep    fibtail(): the code-length tree's fix-up, default strategy.
  d_deep     distskew(): the distance tree's fix-up, where the seed search found it (D_DEEP).
  d_chain    distchain(): the same with set counts per distance code, which reaches it by construction.
  l_deep     the literal/length tree's fix-up under the default strategy: (params, seed) found by
             tests/golden/make_deeptrees.py with the oracle's path counters (L_DEEP_LARGE: more than 63
             leaves; L_DEEP_SMALL: at most 63, a de Bruijn base without matches).
  edge       lengths 0, 1, 2; one byte repeated; two byte values without matches (forced codes); short inputs
             at which static_lenb == opt_lenb or stored_len + 4 == opt_lenb (found by the same script).
tests/golden/deeptrees.json (make_deeptrees.py) pins zlib 1.2.8's output on every item and records how often
the default-strategy items reach each path (test_oracle.py asserts those counts).
"""
import collections
import functools
import heapq
import json
import os
import random

import numpy as np

import _libs

Item = collections.namedtuple("Item", "name data level window memlevel strategy")
Z_DEFAULT, Z_HUFFMAN_ONLY, Z_RLE = 0, 2, 3
CUTS = (0, 1, 2, 5, 9)     # the fixture's inflate results: the whole stream, and cut this many bytes short


def cuts_of(s):
    """[(cut, the stream without its last `cut` bytes)] for the cuts that leave something."""
    return [(cut, s[:len(s) - cut]) for cut in CUTS if cut < len(s)]


FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deeptrees.json")


def huffman_depth(hist):
    """Depth of the Huffman tree of the non-zero counts of `hist`, with no length limit.  Ties go to the
    shallower subtree, as zlib's smaller() (Z/trees.c:442), which keeps the tree as flat as the counts allow."""
    h = [(f, 0) for f in hist if f]
    heapq.heapify(h)
    while len(h) > 1:
        (fa, da), (fb, db) = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (fa + fb, max(da, db) + 1))
    return h[0][1] if h else 0


def fib_counts(k):
    """F2..F(k+1) = 1, 2, 3, 5, ...: k counts."""
    out, a, b = [], 1, 2
    for _ in range(k):
        out.append(a)
        a, b = b, a + b
    return out


def literal_blocks(data, memlevel):
    """The byte histograms (plus the end-of-block symbol) of the blocks deflate_huff cuts `data` into: one
    every lit_bufsize - 1 literals (Z/deflate.h:323-339)."""
    n = (1 << (memlevel + 6)) - 1
    out = []
    for at in range(0, max(len(data), 1), n):
        out.append(np.bincount(np.frombuffer(data[at:at + n], dtype=np.uint8), minlength=256).tolist() + [1])
    return out


def _spread(vals, counts, r, max_run=None):
    """The multiset {vals[i] x counts[i]} in seeded random order; with max_run, equal bytes in a row are
    kept to at most max_run by swapping the byte that makes a longer run with a random other position."""
    b = bytearray()
    for v, c in zip(vals, counts):
        b += bytes([v]) * c
    r.shuffle(b)
    if max_run:
        def run_at(i):   # longest run through position i
            lo = hi = i
            while lo > 0 and b[lo - 1] == b[i]:
                lo -= 1
            while hi + 1 < len(b) and b[hi + 1] == b[i]:
                hi += 1
            return hi - lo + 1
        for i in range(max_run, len(b)):
            for _ in range(50):
                if run_at(i) <= max_run:
                    break
                j = r.randrange(len(b))
                b[i], b[j] = b[j], b[i]
                if run_at(i) > max_run or run_at(j) > max_run:
                    b[i], b[j] = b[j], b[i]
    return bytes(b)


def fib_block(seed, k, flat=0, flat_count=0, max_run=None):
    """One block's worth of bytes: k byte values with counts F2..F(k+1), and `flat` more with flat_count each."""
    r = random.Random(seed)
    vals = r.sample(range(256), k + flat)
    return _spread(vals, fib_counts(k) + [flat_count] * flat, r, max_run)


def fibtail(seed, n, nbase, ntail):
    """n bytes uniform over nbase byte values; ntail other values overwrite random positions 1, 2, 3, 5, 8, ...
    times: literal lengths spread one by one over 8..15 bits, so the code-length tree's counts are skewed."""
    rng = np.random.default_rng(seed)
    vals = rng.permutation(256)
    d = vals[rng.integers(0, nbase, size=n)].astype(np.uint8)
    for v, c in zip(vals[nbase:nbase + ntail], fib_counts(ntail)):
        d[rng.integers(0, n, size=c)] = v
    return d.tobytes()


_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
          4097, 6145, 8193, 12289, 16385, 24577, 32769]


def distskew(seed, n, head=33000, ratio=0.55):
    """`head` random bytes, then 3-byte copies whose distance code is drawn with weight ratio^i over codes
    2..29, each followed by one random byte: the distance tree's counts fall off geometrically."""
    r = random.Random(seed)
    b = bytearray(r.randbytes(head))
    codes = list(range(2, 30))
    weights = [ratio ** i for i in range(len(codes))]
    while len(b) < n:
        c = r.choices(codes, weights)[0]
        dist = r.randrange(_DBASE[c], _DBASE[c + 1])
        at = len(b) - dist
        b += b[at:at + 3]    # (dist >= 3, so the three bytes exist)
        b.append(r.randrange(256))
    return bytes(b[:n])


def chain_counts(k):
    """k counts 1, 1, 3, 4, 7, 11, 18, ... whose Huffman tree is one chain (depth k - 1) and stays one when a few
    counts are off: each is the sum of all counts up to the one before its predecessor, plus a tenth (2 at least).
    (Fibonacci counts are the limit case: one more count of 1 and the chain splits.)"""
    out = [1, 1]
    while len(out) < k:
        below = sum(out[:-1])
        out.append(below + max(2, below // 10))
    return out[:k]


def distchain(seed, k, head=5000):
    """The same shape with set counts: k of the distance codes 2..23 (distances up to 4096, which deflate_slow
    keeps at length 3: TOO_FAR) get chain_counts(k) copies in seeded random order.  So that deflate finds these
    matches and hardly any other, a copy's source is drawn again while its three bytes occur once more nearer
    by, and the trigrams across a copy's ends are new.  In one block (memLevel 9) the distance tree's
    unlimited depth is k - 1: 16 for k = 17 (two nodes below 15: overflow 2), 17 for k = 18 (overflow 4)."""
    r = random.Random(seed)
    b = bytearray(r.randbytes(head))
    last = {}    # trigram -> its latest position

    def index(lo):
        for i in range(lo, len(b) - 2):
            last[bytes(b[i:i + 3])] = i

    index(0)
    order = []
    for c, cnt in zip(r.sample(range(2, 24), k), chain_counts(k)):
        order += [c] * cnt
    r.shuffle(order)
    deferred = 0
    while order:
        c, n = order.pop(), len(b)
        for _ in range(50):
            at = n - r.randrange(_DBASE[c], _DBASE[c + 1])
            b += b[at:at + 3]
            if last.get(bytes(b[at:at + 3])) == at and bytes(b[n - 2:n + 1]) not in last and bytes(b[n - 1:n + 2]) not in last \
                    and b[n - 2:n + 1] != b[n - 1:n + 2]:
                break
            del b[n:]
        else:    # no source fits here (the near codes have one or two distances): this copy comes later
            deferred += 1
            if deferred > 10 * k or not order:
                raise ValueError("distchain: no source for code %d at %d" % (c, n))
            order.insert(r.randrange(len(order)), c)
            continue
        b.append(r.randrange(256))
        while bytes(b[n + 1:n + 4]) in last:     # (these two bytes have been followed by a few byte values, not by all)
            b[n + 3] = r.randrange(256)
        index(n - 2)
    return bytes(b)


def de_bruijn(k, n=3):
    """The lexicographically least de Bruijn sequence B(k, n) as a list (Fredricksen-Kessler-Maiorana):
    read cyclically, every n-gram over k symbols occurs once -- deflate finds no match in it."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return seq


def bruijn_tail(seed, nbase, ntail, scale=1):
    """An order-3 de Bruijn sequence over nbase byte values (nbase^3 bytes, no repeated trigram), then ntail
    other values overwriting random positions scale * (1, 2, 3, 5, ...) times."""
    rng = np.random.default_rng(seed)
    vals = rng.permutation(256)
    d = vals[np.array(_bruijn3(nbase))].astype(np.uint8)
    for v, c in zip(vals[nbase:nbase + ntail], fib_counts(ntail)):
        d[rng.integers(0, len(d), size=c * scale)] = v
    return d.tobytes()


@functools.lru_cache(maxsize=None)
def _bruijn3(k):
    return tuple(de_bruijn(k, 3))


def small(seed, n, alphabet):
    """n bytes over the first `alphabet` letters: the tie search's inputs."""
    r = random.Random(seed)
    return bytes((97 + r.randrange(alphabet)) & 255 for _ in range(n))


# ---- what tests/golden/make_deeptrees.py found (its search is seeded; rerun it to check) ---------------
# (seed, n, nbase, ntail, level) for fibtail at memLevel 9, windowBits 15: more than 63 leaves
L_DEEP_LARGE = [(37268, 30686, 181, 13, 3), (498360, 29489, 136, 15, 9), (886336, 28645, 63, 13, 4),
                (83561, 30757, 172, 13, 9), (814619, 29130, 154, 15, 1), (128153, 29168, 154, 13, 1),
                (621115, 29313, 105, 13, 4), (628913, 25064, 157, 14, 9)]
# (seed, nbase, ntail, scale, level) for bruijn_tail at memLevel 9, windowBits 15: at most 63 leaves
L_DEEP_SMALL = [(976662, 31, 13, 2, 3), (651455, 31, 13, 3, 1), (677886, 30, 13, 2, 6), (568312, 31, 14, 1, 9)]
# (seed, ratio, memlevel) for distskew(seed, 70000, ratio=ratio) at windowBits 15; each at levels 1, 6 and 9
D_DEEP = [(139, 0.58, 9), (17, 0.58, 9)]
# (seed, k) for distchain at memLevel 9, windowBits 15; each at levels 1, 6 and 9
D_CHAIN = ((1, 17), (2, 18))
# (seed, n, alphabet, level, memlevel): static_lenb == opt_lenb / stored_len + 4 == opt_lenb
TIE_STATIC = [(292709, 152, 2, 6, 1), (684364, 120, 2, 9, 9), (889427, 48, 3, 6, 1)]
TIE_STORED = [(216897, 75, 64, 9, 8), (631431, 170, 256, 9, 1), (617374, 68, 64, 9, 9)]

HUFF_K = ((16, 7), (16, 8), (16, 9), (17, 7), (17, 8), (17, 9), (20, 9))   # (k, memLevel): fits lit_bufsize - 1
# (k, flat values, count of each, memLevel): more than 63 leaves in one block
HUFF_FLAT = ((17, 60, 400, 9), (16, 64, 150, 8), (20, 70, 58, 9))
# (k, flat values, count of each, memLevel): exactly lit_bufsize - 1 bytes, the whole first block of an input that
# goes on with text (6763 + 2 * 714 = 8191: the register heap; 4179 + 108 * 113 = 16383: the LDS heap)
HUFF_THEN_TEXT = ((17, 2, 714, 7), (16, 108, 113, 8))


def _text(seed, n):
    return _libs.text(random.Random(seed), n)


@functools.lru_cache(maxsize=None)
def items():
    out = []

    def add(name, data, level, window, memlevel, strategy=Z_DEFAULT):
        out.append(Item(name, data, level, window, memlevel, strategy))

    # a, b: one block of the Fibonacci histogram, Z_HUFFMAN_ONLY and Z_RLE (the candidates' level is 6)
    for strat, fam, run in ((Z_HUFFMAN_ONLY, "huff_fib", None), (Z_RLE, "rle_fib", 2)):
        for k, m in HUFF_K:
            add("%s_%d_m%d" % (fam, k, m), fib_block(1000 + 10 * k + m, k, max_run=run), 6, 15, m, strat)
        for k, flat, cnt, m in HUFF_FLAT:
            add("%s_%d_flat%d_m%d" % (fam, k, flat, m), fib_block(2000 + 10 * k + m, k, flat, cnt, max_run=run),
                6, 15, m, strat)
        for k, flat, cnt, m in HUFF_THEN_TEXT:
            assert sum(fib_counts(k)) + flat * cnt == (1 << (m + 6)) - 1
            add("%s_%d_then_text_m%d" % (fam, k, m), fib_block(3000 + m, k, flat, cnt, max_run=run) + _text(3001, 5000),
                6, 15, m, strat)
    # c: code-length tree
    k = 0
    for level in (1, 3, 4, 6, 9):
        for m in (6, 8, 9):
            for w in (9, 12, 15):
                n = (6000, 12000, 20000, 33000)[k % 4]
                nbase, ntail = 100 + (k * 37) % 101, 12 + k % 6
                add("bl_deep_l%d_w%d_m%d" % (level, w, m), fibtail(4000 + k, n, nbase, ntail), level, w, m)
                k += 1
    # d: distance tree
    for seed, ratio, m in D_DEEP:
        for level in (1, 6, 9):
            add("d_deep_s%d_l%d_m%d" % (seed, level, m), distskew(seed, 70000, ratio=ratio), level, 15, m)
    for seed, k in D_CHAIN:
        for level in (1, 6, 9):
            add("d_chain_%d_l%d" % (k, level), distchain(seed, k), level, 15, 9)
    # e: literal/length tree, default strategy
    for seed, n, nbase, ntail, level in L_DEEP_LARGE:
        add("l_deep_large_s%d_l%d" % (seed, level), fibtail(seed, n, nbase, ntail), level, 15, 9)
    for seed, nbase, ntail, scale, level in L_DEEP_SMALL:
        add("l_deep_small_s%d_l%d" % (seed, level), bruijn_tail(seed, nbase, ntail, scale), level, 15, 9)
    # f: forced codes and ties
    t = _text(5000, 64)
    for name, d in (("len0", b""), ("len1", b"q"), ("len2", b"qr"), ("one_byte_3", b"aaa"), ("one_byte_300", b"a" * 300),
                    ("two_bytes", b"abbaab"), ("two_bytes_2", b"ab")):
        for level in (1, 6):
            add("edge_%s_l%d" % (name, level), d, level, 15, 8)
    for fam, found in (("tie_static", TIE_STATIC), ("tie_stored", TIE_STORED)):
        for seed, n, alphabet, level, m in found:
            add("edge_%s_s%d" % (fam, seed), small(seed, n, alphabet), level, 15, m)
    add("edge_text64", t, 6, 15, 8)
    assert len({it.name for it in out}) == len(out) <= 250 and sum(len(it.data) for it in out) <= 4 << 20
    return tuple(out)


def default_items():
    return [it for it in items() if it.strategy == Z_DEFAULT]


def deep_block_items():
    """Family a's (item, index of the block named deep, k)."""
    return [(it, 0, int(it.name.split("_")[2])) for it in items() if it.name.startswith("huff_fib")]


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def run_counted(its):
    """ora_deflate over `its` with the path counters reset first -> ([stream], counters)."""
    _libs.ora_counters_reset()
    outs = [_libs.ora_deflate(it.data, it.level, it.window, it.memlevel)[0] for it in its]
    return outs, _libs.ora_counters()


def reference_stream(it):
    """zlib 1.2.8's stream for an item: the oracle under the default strategy (the fixture pins it to the real
    zlib), tests/zstrat.py otherwise."""
    if it.strategy == Z_DEFAULT:
        return _libs.ora_deflate(it.data, it.level, it.window, it.memlevel)[0]
    import zstrat
    return zstrat.deflate(it.data, it.level, it.window, it.memlevel, it.strategy)
