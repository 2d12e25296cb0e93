"""Seeded streams whose symbol count stands exactly on a block boundary, for the code that cuts blocks inside a sweep.

zlib ends a block when lit_bufsize - 1 symbols are tallied (L = lit_bufsize = 2^(memLevel + 6)).  tests/edges.py
puts inputs on that edge and runs each as one whole-stream trial; in a sweep the same edge is decided by other code
(DESIGN.md s3.5, s3.6): parse_replay re-cuts a saved symbol sequence into another memLevel's blocks, a budget-free
replay of at most L - 2 symbols is not launched at all, multi-wave trials hand block after block to their flushers,
and a trial reads match-table entries only for a prefix of P = max(1024, 2 L) positions (P3 = max(3072, 2 L) under
the big-file policies) and is run again when it parses past it.  The families:

  B1  no-match streams (symbol count = length) of the lengths b1_lengths(m): L - 2, L - 1, L, L + 1, 2 (L - 1),
      2 (L - 1) + 1, 4 (L - 1), 4 (L - 1) + 1, P - 1 .. P + 3 and P3 - 1 .. P3 + 3, up to MAX_LEN; every memLevel,
      windowBits 15, levels LEVELS_B1 (every header class, deflate_fast and deflate_slow), two contents:
      "uniq3" (edges.uniq3 over 256 values: zlib stores the blocks, so the flush position shows in the output) and
      "skew3" (no trigram twice over 64 skewed values: dynamic blocks of literals).
  B2  streams with matches and a tuned symbol count T of targets(m): text, then a no-match tail over sixteen byte
      values the text does not use, then either nothing (the last symbol is a literal: deflate_slow's pending one)
      or a copy of 30-40 bytes of the text's end (the last symbol is a match).  Levels LEVELS_B2, memLevels 1-8,
      windowBits 15.  The text supplies most symbols and the tail (TAIL_MIN .. TAIL_MAX bytes) the exact count, so
      the copy's source stays within a few hundred bytes at every T.
  B3  the three replay regimes at windowBits 10 and 12 (MAX_DIST = 2^w - 262): the B1 block-edge lengths, and B2
      targets at levels LEVELS_B3, for the four memLevels B3_MEMLEVELS[w], whose edges fall at most at MAX_DIST
      (unchecked replays allowed), in (MAX_DIST, wsize + MAX_DIST] (checked replays only) and past it (the window
      slides: no replay).  regime(item) names the range.

The tuned (text length, tail length, variant) of every B2 / B3 target is found by tune() with the oracle's deflate
and edges.walk_symbols; that takes some twenty seconds, so tests/golden/make_blockedges.py records the triples
in tests/golden/blockedges.json ("tuned", None for a target that is left out: one that six steps did not reach, or
one whose stream the reference's rule leaves at a near miss) and items() reads them there.  tests/test_blockedges_cpu.py walks every stream and asserts the premises (no match in B1, exactly T
symbols and the named last symbol in B2, the block model), so a stale triple fails there.

files() -> {family: (bytes, [(offset, stream length, item position, inflated length)])}: the oracle's streams with
5-40 bytes of text between them and edges.e2e_file's fill rule before a stream that would cross a 524288-byte chunk
end.  The B1 file holds every (memLevel, length, content) at all five levels up to memLevel 7 and at two rotating
levels (one deflate_fast, one deflate_slow) at memLevels 8 and 9, which keeps the corpus under 16 MB.
"""
import collections
import functools
import itertools
import json
import os
import random

import _libs
import edges as E

Item = collections.namedtuple("Item", "family tag data level window memlevel strategy target ending")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blockedges.json")
SEED = 20261021
MAX_LEN = 70000
LEVELS_B1 = (1, 3, 4, 6, 9)
LEVELS_B2 = (1, 2, 3, 4, 6, 9)
LEVELS_B3 = (1, 4, 9)
MEMLEVELS_B2 = tuple(range(1, 9))
B3_MEMLEVELS = {10: (1, 2, 3, 4), 12: (3, 4, 5, 6)}
ENDINGS = ("match", "literal")
TAIL_MIN, TAIL_MAX = 8, 200
TUNE_STEPS = 6
TEXT_LEN = 260000
FAMILIES = ("B1", "B2", "B3")


def lit_bufsize(m):
    return 1 << (m + 6)


def prefix(m, floor=1024):
    """The positions a sweep trial at memLevel m gets match-table entries for (floor 3072: big-file policies)."""
    return max(floor, 2 * lit_bufsize(m))


def edge_lengths(m):
    L = lit_bufsize(m)
    return (L - 2, L - 1, L, L + 1, 2 * (L - 1), 2 * (L - 1) + 1, 4 * (L - 1), 4 * (L - 1) + 1)


def b1_lengths(m):
    P, P3 = prefix(m), prefix(m, 3072)
    ns = set(edge_lengths(m)) | set(range(P - 1, P + 4)) | set(range(P3 - 1, P3 + 4))
    return tuple(sorted(n for n in ns if n <= MAX_LEN))


def targets(m):
    L = lit_bufsize(m)
    return (L - 2, L - 1, L, 2 * (L - 1), 2 * (L - 1) + 1, 4 * (L - 1))


N_B1 = sum(len(b1_lengths(m)) for m in range(1, 10)) * 2 * len(LEVELS_B1)
N_B2_TARGETS = len(MEMLEVELS_B2) * 6 * len(LEVELS_B2) * 2
N_B3_PLAIN = 2 * 4 * 8 * 2 * len(LEVELS_B1)
N_B3_TARGETS = 2 * 4 * 6 * len(LEVELS_B3) * 2


# ---- contents ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def skew3(seed, n):
    """n bytes over 64 values drawn with weights 1 / (i + 6), the next byte drawn again while its trigram was seen:
    no match at any level, and a literal code short enough that zlib chooses dynamic blocks."""
    r, seen, out = random.Random(seed), set(), bytearray()
    cum = list(itertools.accumulate(1.0 / (i + 6) for i in range(64)))
    rejected = 0
    while len(out) < n:
        for b in r.choices(range(0x30, 0x70), cum_weights=cum, k=4096):
            if len(out) >= 2:
                t = (out[-2] << 16) | (out[-1] << 8) | b
                if t in seen:
                    rejected += 1
                    assert rejected < 100000, "skew3 is stuck at %d bytes" % len(out)
                    continue
                seen.add(t)
            rejected = 0
            out.append(b)
            if len(out) == n:
                break
    return bytes(out)


@functools.lru_cache(maxsize=None)
def _tail16():
    """TAIL_MAX bytes over 'A'..'P' with no trigram twice (the text is lower case and spaces)."""
    r, seen, out = random.Random(SEED + 300), set(), bytearray()
    while len(out) < TAIL_MAX:
        b = 0x41 + r.randrange(16)
        if len(out) >= 2:
            t = (out[-2], out[-1], b)
            if t in seen:
                continue
            seen.add(t)
        out.append(b)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def _long_text():
    return E.text(SEED + 400, TEXT_LEN)


def tuned_payload(k, triple, ending):
    """Target k's bytes: text (a slice of one long text, at an offset of its own), tail, and for a "match" ending
    a copy of 30-40 bytes that lie 40-99 bytes before the text's end; `variant` moves the copy."""
    ntext, ntail, variant = triple
    o = (k * 977) % 4096
    text = _long_text()[o:o + ntext]
    assert len(text) == ntext and TAIL_MIN <= ntail <= TAIL_MAX
    out = text + _tail16()[:ntail]
    if ending == "match":
        clen, back = 30 + (k + 3 * variant) % 11, 40 + (7 * k + 13 * variant) % 60
        at = max(0, ntext - back - clen)
        out += text[at:at + clen]
    return out


def symbols(s):
    """(symbol count, whether the last symbol is a match) of a zlib stream; None if it holds a stored block."""
    blocks = E.walk_symbols(s)
    if any(b.btype == 0 for b in blocks):
        return None
    last = [b for b in blocks if b.nlit or b.matches]
    return sum(b.nlit + len(b.matches) for b in blocks), bool(last and last[-1].tail)


def target_list():
    """[(family, T, level, window, memLevel, ending)] of every tuned target: B2's, then B3's; the position is k."""
    out = [("B2", T, lv, 15, m, e) for m in MEMLEVELS_B2 for T in targets(m) for lv in LEVELS_B2 for e in ENDINGS]
    out += [("B3", T, lv, w, m, e) for w in (10, 12) for m in B3_MEMLEVELS[w] for T in targets(m)
            for lv in LEVELS_B3 for e in ENDINGS]
    assert len(out) == N_B2_TARGETS + N_B3_TARGETS
    return out


def tune(k, target):
    """-> (text length, tail length, variant) for which the oracle's stream has exactly T symbols, no stored block
    and the named last symbol; None when TUNE_STEPS streams did not get there."""
    _, T, lv, w, m, ending = target
    aim = min(100, max(TAIL_MIN, T // 4))
    ntext, ntail, variant = max(48, int((T - aim) * 1.5)), aim, 0
    for _ in range(TUNE_STEPS):
        got = symbols(_libs.ora_deflate(tuned_payload(k, (ntext, ntail, variant), ending), lv, w, m)[0])
        if got is None:
            return None
        count, tail = got
        if count == T:
            if tail == (ending == "match"):
                return (ntext, ntail, variant)
            variant += 1
            continue
        if TAIL_MIN <= ntail + T - count <= TAIL_MAX:
            ntail += T - count
            continue
        in_text = max(1, count - ntail - (ending == "match"))       # symbols of the text
        ntext = max(48, ntext + int((T - count + ntail - aim) * ntext / in_text))
        ntail = aim
    return None


_TUNED = None


def set_tuned(triples):
    """The recorder's: use these triples and not the fixture's."""
    global _TUNED
    _TUNED = [None if t is None else tuple(t) for t in triples]
    items.cache_clear()
    files.cache_clear()


def tuned():
    return _TUNED if _TUNED is not None else [None if t is None else tuple(t) for t in fixture()["tuned"]]


# ---- the families -----------------------------------------------------------------------------------
def _plain(add, family, w, m, lengths):
    for gen, seed in ((E.uniq3, SEED + 100), (skew3, SEED + 200)):
        whole = gen(seed + 16 * w + m, max(lengths))
        for n in lengths:
            for lv in LEVELS_B1:
                add(Item(family, gen.__name__, whole[:n], lv, w, m, E.Z_DEFAULT, n, "literal"))


@functools.lru_cache(maxsize=None)
def items():
    """B1, B2, B3 in this order; an item's position is its key in the fixture.  A target that was not reached is
    left out."""
    out = []
    tl, tr = target_list(), tuned()
    assert len(tl) == len(tr)

    def add_tuned(fam):
        for k, ((f, T, lv, w, m, ending), triple) in enumerate(zip(tl, tr)):
            if f == fam and triple is not None:
                out.append(Item(fam, "tuned", tuned_payload(k, triple, ending), lv, w, m, E.Z_DEFAULT, T, ending))

    for m in range(1, 10):
        _plain(out.append, "B1", 15, m, b1_lengths(m))
    assert len(out) == N_B1
    add_tuned("B2")
    n = len(out)
    for w in (10, 12):
        for m in B3_MEMLEVELS[w]:
            _plain(out.append, "B3", w, m, edge_lengths(m))
    assert len(out) == n + N_B3_PLAIN
    add_tuned("B3")
    return tuple(out)


def family(name):
    """[(position in items(), item)] of one family."""
    return [(k, it) for k, it in enumerate(items()) if it.family == name]


def pack(its):
    """(buffer, items) for antiz_amd.Context.deflate_batch: `its` in this order, each payload at a multiple of 16."""
    buf, batch = bytearray(), []
    for it in its:
        batch.append((len(buf), len(it.data), it.level, it.window, it.memlevel, it.strategy))
        buf += it.data
        buf += bytes(-len(buf) % 16)
    return bytes(buf), batch


def regime(it):
    """Which replays a trial of this stream at its window may use."""
    W = 1 << it.window
    n = len(it.data)
    return "unchecked" if n <= W - 262 else ("checked" if n <= 2 * W - 262 else "slides")


def model_blocks(T, level, m, ending):
    """The symbol counts of the blocks zlib cuts T symbols into.  deflate_fast (levels 1-3), and deflate_slow when
    the last symbol is a match, flush whenever the tally reaches L - 1 (Z/deflate.h:323-339) and Z_FINISH adds a
    last block, empty if need be; deflate_slow tallies its last, pending literal without a flush check
    (Z/deflate.c:1801-1806), so a stream that ends in a literal closes a full last block."""
    full = lit_bufsize(m) - 1
    k = (T - 1) // full if level > 3 and ending == "literal" else T // full
    return [full] * k + [T - k * full]


# ---- the files --------------------------------------------------------------------------------------
def in_file(it):
    if it.family != "B1" or it.memlevel < 8:
        return True
    j = (len(it.data) + it.memlevel) % 6
    return it.level in ((1, 3)[j % 2], (4, 6, 9)[j % 3])


@functools.lru_cache(maxsize=None)
def files(deflate=None):
    """{family: (file bytes, [(offset, stream length, item position, inflated length)])}; `deflate` as in
    edges.e2e_file (the recorder passes the real zlib's)."""
    deflate = deflate or (lambda d, lv, w, m: _libs.ora_deflate(d, lv, w, m)[0])
    out = {}
    for f, fam in enumerate(FAMILIES):
        r = random.Random(SEED + 500 + f)
        parts, recs, pos = [], [], 0
        for k, it in family(fam):
            if not in_file(it):
                continue
            fill = _libs.text(r, r.randrange(5, 40))
            s = deflate(it.data, it.level, it.window, it.memlevel)
            at = pos + len(fill)
            end = next(b for b in range(524288, 1 << 30, 524287) if b > at)    # the end of the chunk the stream starts in
            if at + len(s) + 8 > end:
                fill += _libs.text(r, end + 8 - at)
            recs.append((pos + len(fill), len(s), k, len(it.data)))
            parts += [fill, s]
            pos += len(fill) + len(s)
        parts.append(_libs.text(r, 33))
        out[fam] = (b"".join(parts), recs)
    return out


# the reference's flags per fixture setting; "brute" is recorded for B3 only
SETTINGS = {"default": [], "tol0": ["--mismatch-tol", "0"],
            "strict_shortcut": ["--recomp-tresh", "16", "--shortcut-len", "64"], "brute": ["--brute-window"]}


def settings_of(fam):
    return [s for s in SETTINGS if s != "brute" or fam == "B3"]


@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)
