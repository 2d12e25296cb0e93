"""The size-class and window edge inputs (tests/edges.py) on the CPU: the oracle gives the real zlib 1.2.8's
result (tests/golden/edges.json) on every item, and the inputs are what they are named for -- the premises
below are read off the oracle's streams with edges.walk_symbols, so an input that stopped reaching its edge
(another seed, another generator) fails here and not silently on the GPU."""
import functools
import hashlib
import os

import _libs
import edges as E
import zstrat


def sha(b):
    return hashlib.sha256(b).hexdigest()


@functools.lru_cache(maxsize=None)
def streams():
    """The oracle's stream of every item of edges.items(), by position."""
    return [_libs.ora_deflate(it.data, it.level, it.window, it.memlevel)[0] for it in E.items()]


@functools.lru_cache(maxsize=None)
def inflate_streams():
    return [_libs.ora_deflate(d, lv, w, m)[0] for _, d, (lv, w, m) in E.inflate_payloads()]


@functools.lru_cache(maxsize=None)
def e2e():
    data, recs = E.e2e_file()
    out = {"data": data, "recs": recs}
    for name, brute in (("default", 0), ("brute", 1)):
        rc, atz, stats = _libs.ora_precompress(data, brute=brute)
        assert rc == 0
        out[name] = (atz, stats)
    return out


# ---- 1, 2: the oracle equals the fixture ------------------------------------------------------------
def test_generator_counts_and_lengths():
    """No item is filtered out: the families have the sizes the generator defines, and every length is the
    listed one exactly."""
    its = E.items()
    assert [len(E.family(f)) for f in ("D1", "D2", "D3", "D4")] == [1620, E.N_D2, E.N_D3, E.N_D4] == [1620, 4095, 459, 42]
    assert len(its) == 6216 and len(E.strategy_items()) == E.N_D5 == 810
    assert sorted({len(it.data) for _, it in E.family("D1")}) == list(E.LENGTHS_D1)
    assert {(it.tag, it.level, it.memlevel) for _, it in E.family("D1")} == \
        {(t, lv, m) for t in ("zeros", "per3", "text", "text_run") for lv in E.LEVELS_D1 for m in E.MEMLEVELS_D1}
    for w in range(9, 16):
        mine = [it for _, it in E.family("D2") if it.window == w]
        assert sorted({len(it.data) for it in mine}) == sorted(E.d2_lengths(w))
        for tag in ("rnd-1", "rnd+0", "rnd+1", "txt+0", "zeros", "text"):
            assert {len(it.data) for it in mine if it.tag == tag} == set(E.d2_lengths(w)), (w, tag)
        rot = [it for it in mine if it.tag in ("txt+0", "zeros", "text")]
        assert {it.level for it in rot} == {it.memlevel for it in rot} == set(range(1, 10)), w
    for m in range(1, 10):
        assert {len(it.data) for _, it in E.family("D3") if it.memlevel == m and it.tag == "uniq3"} == set(E.d3_lengths(m))
        B = E.stored_max(m)
        assert {len(it.data) for _, it in E.family("D3") if it.memlevel == m and it.level == 0} == {B - 1, B, B + 1, 2 * B, 2 * B + 1}
    fx = E.fixture()
    assert fx["seed"] == E.SEED and len(fx["deflate"]) == len(its) and len(fx["strategy"]) == E.N_D5
    assert len(fx["inflate"]) == len(E.DIST_PS) == 102


def test_oracle_equals_fixture_on_every_deflate_item():
    fx = E.fixture()["deflate"]
    bad = [(k, E.label(it)) for k, (it, s) in enumerate(zip(E.items(), streams()))
           if [len(s), E.sha16(s)] != fx[k]]
    assert not bad, bad[:10]


def test_oracle_equals_fixture_on_every_inflate_case():
    fx = E.fixture()["inflate"]
    n = 0
    for i, s in enumerate(inflate_streams()):
        assert [len(s), E.sha16(s)] == fx[i]["stream"], E.DIST_PS[i]
        cases = E.inflate_cases(s, i)
        assert len(cases) == len(fx[i]["cases"]) == 5
        for (tag, part), want in zip(cases, fx[i]["cases"]):
            assert _libs.ora_inflate(part) == tuple(want), (E.DIST_PS[i], tag)
            n += 1
    assert n == 510


def test_oracle_equals_fixture_end_to_end():
    fx = E.fixture()["e2e"]
    assert sha(e2e()["data"]) == fx["input_sha256"] and len(e2e()["recs"]) == fx["n_streams"]
    for name in ("default", "brute"):
        assert sha(e2e()[name][0]) == fx["atz_sha256"][name], name


# ---- 3: the fixture is the real zlib's --------------------------------------------------------------
def test_fixture_is_the_reference():
    """Where the reference build is there (oracle/_ref), a fresh run of the recorder gives the committed fixture,
    byte for byte; the strategy items need only its zlib."""
    fx = E.fixture()["strategy"]
    for k, it in enumerate(E.strategy_items()):
        s = zstrat.deflate(it.data, it.level, it.window, it.memlevel, it.strategy)
        assert [len(s), E.sha16(s)] == fx[k], E.label(it)
    if _libs.have_zref() and os.path.exists(_libs.REF_UNCOMP):
        import sys
        sys.path.insert(0, os.path.dirname(E.FIXTURE))
        import make_edges
        with open(E.FIXTURE) as f:
            assert make_edges.dumps(make_edges.record()) == f.read()


# ---- 4: premises ------------------------------------------------------------------------------------
def _d2(tag):
    """{(window, length, level, memlevel): matches} of one D2 content."""
    return {(it.window, len(it.data), it.level, it.memlevel): E.matches_of(streams()[k])
            for k, it in E.family("D2") if it.tag == tag}


def test_d2_period_maxdist_is_matched_at_exactly_maxdist():
    """A block of MAX_DIST random bytes, repeated: at memLevel 9 (no hash collisions to speak of) the copy one
    period back is the hash head, which is walked at distance exactly MAX_DIST (Z/deflate.c:1227) -- every
    window, every level, every length from W + MD + 1."""
    got = _d2("rnd+0")
    n = 0
    for (w, length, lv, m), ms in got.items():
        W = 1 << w
        MD = W - 262
        if m == 9 and length >= W + MD + 1:
            assert any(d == MD for d, _ in ms), (w, length, lv)
            n += 1
        assert all(d <= MD for d, _ in ms)
    assert n == 7 * 6 * 6


def test_d2_head_is_walked_at_maxdist_and_a_successor_is_not():
    """The same data at memLevel 1 (256 hash buckets): a later position with the same hash has displaced the
    head, and a chain successor at distance MAX_DIST fails `cur_match > limit` (Z/deflate.c:1227).  For every
    window from 12 and every level, at lengths W + MD + 1 and 2 W + MD + 1 the memLevel 9 stream has matches at
    distance MAX_DIST (16 and more) and the memLevel 1 stream has none."""
    got = _d2("rnd+0")
    for w in range(12, 16):
        W = 1 << w
        MD = W - 262
        for length in (W + MD + 1, 2 * W + MD + 1):
            for lv in E.LEVELS_D2:
                hi = sum(d == MD for d, _ in got[(w, length, lv, 9)])
                lo = sum(d == MD for d, _ in got[(w, length, lv, 1)])
                assert hi >= 16 and lo == 0, (w, length, lv, hi, lo)


def test_d2_period_past_maxdist_is_never_matched():
    """A period of MAX_DIST + 1: the only copy is one byte too far, at every window, level and memLevel."""
    for key, ms in _d2("rnd+1").items():
        assert all(d <= (1 << key[0]) - 262 for d, _ in ms), key
    assert sum(len(ms) for ms in _d2("rnd-1").values()) > 1000   # (the walker does see matches: period MD - 1)


def literal_blocks(n, level, m):
    """The symbol counts of the blocks zlib cuts n literals into.  deflate_fast (levels 1-3) flushes when the
    tally reaches lit_bufsize - 1 (Z/deflate.h:323-339) and Z_FINISH adds a last block, empty if need be;
    deflate_slow tallies a literal one position late and its last, pending one without a flush check
    (Z/deflate.c:1801-1806), so a stream of exactly k (lit_bufsize - 1) literals ends in a full block."""
    full = (1 << (m + 6)) - 1
    k = n // full if level <= 3 else (n - 1) // full
    return [full] * k + [n - k * full]


def stored_blocks(n, w, m):
    """The LEN fields deflate_stored writes for n bytes given at once (Z/deflate.c:1469-1527 over fill_window,
    Z/deflate.c:1355-1457): a block ends at max_block_size, and whenever it has reached MAX_DIST; the window
    slides by wsize once strstart >= wsize + MAX_DIST."""
    wsize, big = 1 << w, E.stored_max(m)
    md = wsize - 262
    strstart = block_start = lookahead = 0
    avail, out = n, []
    while True:
        if lookahead <= 1:
            while True:
                more = 2 * wsize - lookahead - strstart
                if strstart >= wsize + md:
                    strstart -= wsize
                    block_start -= wsize
                    more += wsize
                if avail == 0:
                    break
                k = min(avail, more)
                avail -= k
                lookahead += k
                if lookahead >= 262 or avail == 0:
                    break
            if lookahead == 0:
                break
        strstart += lookahead
        lookahead = 0
        max_start = block_start + big
        if strstart == 0 or strstart >= max_start:
            lookahead = strstart - max_start
            strstart = max_start
            out.append(strstart - block_start)
            block_start = strstart
        if strstart - block_start >= md:
            out.append(strstart - block_start)
            block_start = strstart
    out.append(strstart - block_start)
    return out


def test_d3_block_ends():
    """uniq3 has no match at any level, and its blocks are zlib's: at levels 1-3 a stream of exactly
    lit_bufsize - 1 literals is a full block and an empty last one, from level 4 it is one block.  A full first
    block of random bytes is stored at windowBits 15; at windowBits 9 its start has slid out of the window for
    memLevel 5 and up, so it is dynamic -- as is the second full block at memLevel 9, windowBits 15, which starts
    one byte below the window after the slide.  Level 0: deflate_stored's cuts."""
    seen = set()
    for k, it in E.family("D3"):
        blocks = E.walk_symbols(streams()[k])
        n, m = len(it.data), it.memlevel
        assert [b.final for b in blocks] == [0] * (len(blocks) - 1) + [1]
        if it.level == 0:
            assert all(b.btype == 0 for b in blocks)
            assert [b.nlit for b in blocks] == stored_blocks(n, it.window, m), (n, it.window, m)
            continue
        assert not any(b.matches for b in blocks)
        assert [b.nlit for b in blocks] == literal_blocks(n, it.level, m), (n, it.level, it.window, m)
        L = 1 << (m + 6)
        seen.add((E.d3_lengths(m).index(n), it.level > 3, len(blocks)))
        if m >= 5:
            assert blocks[0].btype == (0 if it.window == 15 else 2), (n, it.level, it.window, m)
        if m == 9 and it.window == 15 and n >= 2 * (L - 1):
            assert blocks[1].btype == 2
        if blocks[-1].nlit <= 1:
            assert blocks[-1].btype == 1
    # (which of the six lengths, deflate_slow, blocks): the two rules differ at L - 1 and at 2 (L - 1)
    assert seen == {(i, slow, nb) for slow, counts in ((False, (1, 2, 2, 2, 3, 3)), (True, (1, 1, 2, 2, 2, 3)))
                    for i, nb in enumerate(counts)}


def test_d4_neighbours_continue_the_match():
    """The bytes after A (B's first) go on matching the source of A's last match; in the text pairs that match
    is A's last symbol, so it reaches A's last byte (zlib ends a run of zeros or of `abc` in a short match or in
    literals, as the lookahead runs out: there the stream's last symbols are whatever the length leaves)."""
    for tag, big, cut in E.d4_pairs():
        if tag == "text":
            assert big[cut:cut + 258] == big[cut - E.D4_BLOCK:cut - E.D4_BLOCK + 258]
        else:
            assert big[cut:cut + 258] == big[cut - 3:cut + 255]
    n = 0
    for k, it in E.family("D4"):
        if it.tag.endswith("A"):
            assert len(it.data) % 256 == 0
            blocks = E.walk_symbols(streams()[k])
            last = [b for b in blocks if b.nlit or b.matches][-1]
            assert last.matches and (last.tail or it.tag != "textA"), (it.tag, len(it.data))
            if it.tag == "textA":
                assert last.matches[-1][0] % E.D4_BLOCK == 0, (len(it.data), it.level, last.matches[-1])
            total = sum(b.nlit + sum(ln for _, ln in b.matches) for b in blocks)
            assert total == len(it.data)
            n += 1
    assert n == 21
    assert sum(it.level <= 3 for _, it in E.family("D4")) >= 14   # a fast level in every pair's three


def test_i1_copies_at_exactly_p():
    for i, (s, P) in enumerate(zip(inflate_streams(), E.DIST_PS)):
        assert P <= 32506 and any(d == P for d, _ in E.matches_of(s)), P
    assert set(range(4020, 4111)) <= set(E.DIST_PS)


def test_e2e_every_stream_is_recorded_exactly():
    """The oracle finds each stream the generator put in at its offset and reproduces it exactly
    (ident == comp_len, no diffs), with and without --brute-window, and the file stays ATZ1."""
    recs = e2e()["recs"]
    assert len(recs) == len(E.DIST_PS) + 3 * len(E.E2E_SIZES) + 2 * len(E.d4_pairs()) == 176
    for name in ("default", "brute"):
        atz, stats = e2e()[name]
        assert atz[:4] == b"ATZ\1"
        by = {s["offset"]: s for s in stats["streams"]}
        for off, length, tag, infl in recs:
            s = by[off]
            assert (s["comp_len"], s["infl_len"], s["recomp"], s["n_diff"]) == (length, infl, 1, 0), (name, tag)
            assert s["ident"] == s["comp_len"], (name, tag)
        assert len(stats["streams"]) == len(recs), name
        assert _libs.ora_reconstruct(atz) == (0, e2e()["data"])
