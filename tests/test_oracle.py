"""The oracle (CPU restatement, oracle/) pinned against the reference's golden vectors.

These run without a GPU.  They establish that oracle/ reproduces zlib 1.2.8 deflate bit-exactly
(G2, from the reference's vendored zlib) and the reference pipeline's .atz bytes (G1 = the
reference's own ZT vectors, G3-G5 = cases produced by the real reference binary).
"""
import functools
import hashlib
import json
import os
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import _libs
import deeptrees as DT
import golden_cases as G
import nearmiss as NM
import zstrat

GOLD = G.GOLD


def sha(b):
    return hashlib.sha256(b).hexdigest()


def test_deflate_kats_full_bytes():
    full = json.load(open(os.path.join(GOLD, "deflate_kat_text4k_w15.json")))
    d = open(os.path.join(GOLD, "kat", "text4k.bin"), "rb").read()
    for key, hexs in full.items():
        c, m = map(int, key.split("/"))
        out, hazard = _libs.ora_deflate(d, c, 15, m)
        assert out.hex() == hexs, key
        assert hazard == 0


@pytest.mark.parametrize("name", ["asd", "text4k", "rand5k", "input8k"])
def test_deflate_kats_all_params(name):
    kat = json.load(open(os.path.join(GOLD, "deflate_kat.json")))
    d = open(os.path.join(GOLD, "kat", name + ".bin"), "rb").read()
    assert sha(d) == kat["inputs"][name]
    for c in range(10):
        for w in range(9, 16):
            for m in range(1, 10):
                out, _ = _libs.ora_deflate(d, c, w, m)
                n, h = kat["results"]["%s/%d/%d/%d" % (name, c, w, m)]
                assert (len(out), sha(out)) == (n, h), (name, c, w, m)


def test_zt_kat_pipeline():
    data, meta = G.zt_kat()
    rc, atz, st = _libs.ora_precompress(data)
    assert rc == 0
    assert sha(atz) == meta["atz_sha256"]
    got = [(s["offset"], s["clevel"], s["window"], s["memlevel"]) for s in st["streams"]]
    want = [(s["offset"], s["clevel"], s["window"], s["memlevel"]) for s in meta["streams"]]
    assert got == want
    rc, rec = _libs.ora_reconstruct(atz)
    assert rc == 0 and rec == data


@pytest.mark.parametrize("case", G.cases(), ids=lambda c: c["name"])
def test_golden_case_pipeline(case):
    data = G.case_input(case)
    rc, atz, st = _libs.ora_precompress(data, **G.opts_kwargs(case["opts"]))
    assert rc == 0
    assert sha(atz) == case["atz_sha256"], case["name"]
    assert st["hazard"] == 0
    rc, rec = _libs.ora_reconstruct(atz)
    assert rc == 0 and rec == data


def test_inflate_roundtrip_and_truncation():
    r = random.Random(5)
    for k in range(200):
        d = _libs.text(r, r.randrange(0, 5000))
        s, _ = _libs.ora_deflate(d, r.randrange(0, 10), r.randrange(9, 16), r.randrange(1, 10))
        st, c, p = _libs.ora_inflate(s + b"junk")
        assert (st, c, p) == (0, len(s), len(d))
        cut = r.randrange(1, len(s))
        st, c, p = _libs.ora_inflate(s[:cut])
        assert st in (1, 2)
        if st == 2:
            assert c == cut


@pytest.mark.skipif(not _libs.have_zref(), reason="reference build (oracle/_ref) absent")
def test_live_reference_deflate_inflate_sample():
    r = random.Random(11)
    for k in range(150):
        d = _libs.text(r, r.randrange(1, 20000))
        c, w, m = r.randrange(0, 10), r.randrange(9, 16), r.randrange(1, 10)
        a, _ = _libs.ora_deflate(d, c, w, m)
        assert a == _libs.zref_deflate(d, c, w, m), (c, w, m)
        s = bytearray(a)
        s[r.randrange(2, len(s))] ^= 1 << r.randrange(8)
        s = bytes(s[:r.randrange(2, len(s) + 1)])
        st, cons, prod = _libs.ora_inflate(s)
        rf, tf, rl, ti, to, ai = _libs.zref_inflate_scan(s)
        assert cons == ti and tf == ti
        assert (st == 0) == (rl == 1)
        if st == 0:
            assert prod == to


MAXDIST_EDGE_SHA = "d75a2a586f840cd037952b7289852f11c4702d92dbefef4b6112824d68680f32"


def test_maxdist_edge_fixture_pinned():
    """tests/golden/maxdist_edge.bin: 11 streams of the C5 workload (windowBits 11, 13, 14; longer than
    MAX_DIST) whose parses hinge on a hash head at distance exactly MAX_DIST (walked as a head, not as
    a chain successor: Z/deflate.c:1227, 1660, 1766).  The expected ATZ1 SHA-256 was produced by the
    real reference (oracle/_ref/uncomp, with and without --brute-window: the same bytes); the oracle
    must agree."""
    data = open(os.path.join(G.GOLD, "maxdist_edge.bin"), "rb").read()
    for brute in (0, 1):
        rc, out, _ = _libs.ora_precompress(data, brute=brute)
        assert rc == 0 and hashlib.sha256(out).hexdigest() == MAXDIST_EDGE_SHA


def test_inflate_edge_fixtures_pinned():
    """tests/golden/inflate_edges.json: the real zlib 1.2.8's results (make_inflate_edges.py) on hand-built
    streams at k_inflate's fast-loop edges (fixed-code 286/287 and distance 30/31, far distances,
    incomplete dynamic distance trees, oversized HLIT/HDIST, all overlapping copies); the oracle agrees."""
    cases = json.load(open(os.path.join(G.GOLD, "inflate_edges.json")))["cases"]
    assert len(cases) > 400
    for c in cases:
        got = _libs.ora_inflate(bytes.fromhex(c["hex"]))
        assert got == (c["status"], c["consumed"], c["produced"]), c["family"]


def test_threshold_grid_near_pins_the_oracle():
    """The oracle's rule (main.cpp:454, 590, 671, 685-700) under non-default thresholds equals the real
    reference's ATZ1 on the `near` input (tests/golden/threshold_grid.json, tools/make_threshold_grid.py)."""
    from antiz_amd import datagen
    grid = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "threshold_grid.json")))
    data = datagen.gen_near(seed=71, n_streams=600)
    for e in (e for e in grid.values() if e["workload"] == "near"):
        assert sha(data) == e["input_sha256"]
        f = e["flags"]
        kw = {"brute": int("--brute-window" in f)}
        for name, key in (("--mismatch-tol", "tol"), ("--recomp-tresh", "recomp"), ("--sizediff-tresh", "sizediff"),
                          ("--shortcut-len", "shortcut")):
            if name in f:
                kw[key] = int(f[f.index(name) + 1])
        rc, atz, _ = _libs.ora_precompress(data, **kw)
        assert rc == 0 and sha(atz) == e["atz_sha256"], f


def test_fuzz_small_files_pin_the_oracle():
    """The seeded fuzz cases (small files, chunk sizes from 2 bytes, threshold variants): the oracle's
    ATZ1 equals the real reference's (tests/golden/fuzz_small.json, tools/make_fuzz_golden.py) on every
    case the reference completes; where it crashes (empty input, main.cpp:406 reads rBuffer[-1]) the
    oracle reports undefined behaviour instead of bytes."""
    fx = json.load(open(os.path.join(GOLD, "fuzz_small.json")))
    checked = 0
    for i, data, cs, opts in G.fuzz_cases():
        f = fx[str(i)]
        if sha(data) != f["input_sha256"]:   # another zlib build made different input streams
            continue
        rc, atz, _ = _libs.ora_precompress(data, chunksize=cs, **G.opts_kwargs(opts))
        if "atz_sha256" in f:
            assert rc == 0 and sha(atz) == f["atz_sha256"], (i, cs, opts)
        else:
            assert f["rc"] != 0 and rc != 0, (i, cs, opts, f["rc"], rc)
        checked += 1
    assert checked >= 150


# ---- near-miss streams (tests/nearmiss.py, tests/golden/nearmiss.json) ----------------------------------


@functools.lru_cache(maxsize=None)
def _nearmiss_default(name):
    rc, atz, st = _libs.ora_precompress(NM.files()[name][0])
    assert rc == 0
    return atz, st


@pytest.mark.parametrize("name", NM.NAMES)
def test_nearmiss_fixture_pins_the_oracle(name):
    """The oracle's ATZ1 on every near-miss file under every setting of tests/golden/nearmiss.json equals
    the real reference's (tools/make_nearmiss_golden.py): SHA-256, length and the recompressed count; under
    the default setting also the stream table (offset, comp_len, c, w, m, n_diff, first_diff of every
    recompressed stream).  Every ATZ1 reconstructs its input."""
    fx = NM.fixture()
    data, _ = NM.files()[name]
    NM.check_pinned(fx)
    assert fx["settings"] == NM.settings(fx["T"], fx["D"])

    def run(sname):
        if sname == "default":
            return _nearmiss_default(name)
        rc, atz, st = _libs.ora_precompress(data, **NM.flags_kwargs(fx["settings"][sname]))
        assert rc == 0
        return atz, st

    with ThreadPoolExecutor(8) as ex:     # the oracle runs outside the interpreter lock
        runs = dict(zip(fx["settings"], ex.map(run, fx["settings"])))
    for sname, flags in fx["settings"].items():
        atz, st = runs[sname]
        assert st["hazard"] == 0
        rc, rec = _libs.ora_reconstruct(atz)
        assert rc == 0 and rec == data, (name, sname)
        table = [[e[k] for k in ("offset", "comp_len", "c", "w", "m", "n_diff", "first_diff")] for e in NM.parse_atz1(atz)]
        mine = [[s["offset"], s["comp_len"], s["clevel"], s["window"], s["memlevel"], s["n_diff"],
                 s["first_diff"] if s["n_diff"] else -1] for s in st["streams"] if s["recomp"]]
        assert mine == table, (name, sname)       # the returned fields say what the ATZ1 says
        e = fx["files"][name]["runs"][sname]
        n_rec = sum(s["recomp"] for s in st["streams"])
        assert (sha(atz), len(atz), "recompressed:%d/%d" % (n_rec, len(st["streams"]))) == \
            (e["atz_sha256"], e["atz_bytes"], e["tail"]), (name, sname, flags)
        if sname == "default":
            assert table == fx["files"][name]["table"], name


def test_nearmiss_diff_positions_are_the_generators():
    """Independent of both implementations: the diff positions of a storedpad or mixed stream are exactly the
    bytes whose padding bits the generator set (values: the original's bytes), k <= 128 of them are
    recompressed and k > 128 are not; an eobpad stream's last diff is at C - 5, any other at offset 1 (the
    re-levelled header); a tailflush stream's list runs to its last byte."""
    seen = set()
    for name, (data, streams) in NM.files().items():
        _, st = _nearmiss_default(name)
        by = {s["offset"]: s for s in st["streams"]}
        for g in streams:
            o = by[g.offset]
            assert (o["comp_len"], o["infl_len"]) == (g.length, g.data_len), (name, g)
            orig = data[g.offset:g.offset + g.length]
            assert o["diff_val"] == bytes(orig[p] for p in o["diff_pos"])
            assert o["n_diff"] == (g.length - o["ident"] if o["recomp"] else 0)
            if g.family in ("storedpad", "mixed"):
                k = len(g.pads)
                assert g.length - o["ident"] == k and bool(o["recomp"]) == (k <= 128), (name, g)
                if o["recomp"]:
                    assert o["diff_pos"] == list(g.pads) and o["first_diff"] == g.pads[0], (name, g)
                    seen.add(k)
            elif g.family == "eobpad":
                assert o["recomp"] and o["diff_pos"] in ([g.length - 5], [1, g.length - 5]), (name, g)
            elif g.family == "tailflush":
                assert o["recomp"] and o["diff_pos"][-1] == g.length - 1 and o["n_trials"] >= 81, (name, g)
    assert seen == {k for k in NM.PAD_KS if k <= 128} | {5, 20}


def test_nearmiss_tolerance_stop_decides():
    """Independent of both implementations: a tolstop stream's first trial (level 5, memLevel 8) misses it
    by d0 bytes and a later one is exact.  With mismatch_tol >= d0 the sweep stops there (main.cpp:700:
    ident + tol >= C): level 5, d0 diffs, one trial; with mismatch_tol = d0 - 1 or less it goes on to a
    better trial.  d0 sits at the default tolerance, at T and T - 1 (the fixture's settings) and one to
    either side.  A wrongwin stream is recompressed only by the brute-window phase, with two diffs."""
    fx = NM.fixture()
    data, streams = NM.files()["tolstop"]
    seen = set()
    for sname, tol in (("default", 2), ("tol0", 0), ("tolT", fx["T"]), ("tolT-1", fx["T"] - 1)):
        assert NM.flags_kwargs(fx["settings"][sname]).get("tol", 2) == tol
        rc, _, st = _libs.ora_precompress(data, tol=tol)
        assert rc == 0
        by = {s["offset"]: s for s in st["streams"]}
        for g in streams:
            o, d0 = by[g.offset], int(g.tag[1:])
            if d0 <= tol:
                assert (o["clevel"], o["memlevel"], o["n_diff"], o["n_trials"]) == (5, 8, d0, 1), (sname, g)
            else:
                assert o["clevel"] < 5 and o["n_diff"] < d0 and o["n_trials"] > 1, (sname, g)
                assert o["n_diff"] == 0 or o["n_diff"] <= tol, (sname, g)
            seen.add((d0 - tol, d0 <= tol))
    assert {(0, True), (1, False), (-1, True)} <= seen      # at the tolerance, one above it, one below it
    data, streams = NM.files()["wrongwin"]
    for brute in (0, 1):
        rc, _, st = _libs.ora_precompress(data, brute=brute)
        by = {s["offset"]: s for s in st["streams"]}
        for g in streams:
            o = by[g.offset]
            assert (o["recomp"], o["diff_pos"]) == ((1, [0, 1]) if brute else (0, [])), (brute, g)
            assert not brute or o["window"] == int(g.tag[1:3])


def test_nearmiss_streams_inflate():
    """zlib ignores a stored block's padding bits and the bits after the last end-of-block code
    (Z/inflate.c: BYTEBITS()); so does the oracle's inflate on every mutated stream."""
    for s, n in NM.mutated_streams():
        assert _libs.ora_inflate(s + b"xy") == (0, len(s), n)


# ---- trees deeper than the length limit (tests/deeptrees.py, tests/golden/deeptrees.json) ------------------


@functools.lru_cache(maxsize=None)
def _deeptrees_default():
    return DT.run_counted(DT.default_items())


def test_deeptrees_fixture_pins_the_oracle():
    """The oracle's stream for every default-strategy item equals the real zlib 1.2.8's (length and SHA-256 in
    tests/golden/deeptrees.json, make_deeptrees.py), and its inflate gives zlib's (status, consumed, produced) on
    every stream and on the stream cut 1, 2, 5 and 9 bytes short -- the Z_RLE and Z_HUFFMAN_ONLY streams too,
    where the reference's zlib is there to make them."""
    fx = DT.fixture()
    assert set(fx["items"]) == {it.name for it in DT.items()} and tuple(fx["cuts"]) == DT.CUTS
    streams = dict(zip((it.name for it in DT.default_items()), _deeptrees_default()[0]))
    if os.path.exists(zstrat.Z128_SO):
        streams.update((it.name, DT.reference_stream(it)) for it in DT.items() if it.strategy)
    assert len(streams) >= len(DT.default_items()) >= 90
    for name, s in streams.items():
        e = fx["items"][name]
        assert [len(s), sha(s)] == e["deflate"], name
        assert len(e["inflate"]) == len(DT.cuts_of(s)) >= 4
        for (cut, part), want in zip(DT.cuts_of(s), e["inflate"]):
            assert _libs.ora_inflate(part) == tuple(want), (name, cut)


def test_deeptrees_reach_the_fixup():
    """What the inputs are for, counted by the oracle (atz_oracle.h ORA_CNT_*) over the default-strategy items:
    gen_bitlen's length-limit fix-up (Z/trees.c:531-564) on each of the three trees, with more than one turn
    of its loop (overflow > 2), on literal/length trees of more than 63 leaves and of at most 63 (k_deflate's
    LDS heap and register heap); both block-type ties; trees with forced codes; and streams that carry a
    15-bit literal/length code, a 15-bit distance code and a 7-bit code-length code.  The counts are the
    fixture's "_reach".

    overflow is never odd: gen_bitlen counts every node whose depth exceeds max_length, leaf or not
    (Z/trees.c:512-515 increments before the leaf test), a Huffman tree's nodes below the root come in sibling
    pairs of one depth, so the count is even and the loop ends at 0, never at -1.  The counter stays, at 0."""
    c = _deeptrees_default()[1]
    print("reach:", c)
    assert c == DT.fixture()["_reach"]
    assert c["fixup_bl"] >= 20 and c["fixup_multi_bl"] >= 5
    assert c["fixup_d"] >= 2 and c["fixup_multi_d"] >= 1
    assert c["fixup_l_large"] >= 4 and c["fixup_l_small"] >= 1
    assert c["fixup_l"] == c["fixup_l_large"] + c["fixup_l_small"] and c["fixup_multi_l"] >= 1
    assert c["fixup_odd_l"] + c["fixup_odd_d"] + c["fixup_odd_bl"] == 0
    assert c["tie_static"] >= 1 and c["tie_stored"] >= 1
    assert c["forced_l"] >= 1 and c["forced_d"] >= 1
    assert c["stored"] >= 1 and c["static"] >= 1 and c["dynamic"] >= 100
    assert c["maxlen_l"] >= 1 and c["maxlen_d"] >= 1 and c["maxlen_bl"] >= 1


def test_deeptrees_counters_leave_the_output_alone():
    """Reset and read between runs: the same bytes, and one run's counts add up."""
    it = next(i for i in DT.default_items() if i.name.startswith("l_deep_large"))
    a, ca = DT.run_counted([it])
    b, cb = DT.run_counted([it, it])
    assert a[0] == b[0] == b[1] and ca["fixup_l_large"] >= 1
    assert all(cb[k] == 2 * ca[k] for k in ca)
    assert ca["stored"] + ca["static"] + ca["dynamic"] >= 1


def test_deeptrees_huffman_only_blocks_are_deep():
    """Family huff_fib needs no search: under Z_HUFFMAN_ONLY a block's literal histogram is its bytes' (plus
    the end-of-block symbol), so the depth of its unlimited Huffman tree is computed here, not assumed:
    above 15 for the first block of every item, at least 19 for k = 20, with at most 63 leaves (the register
    heap) for the plain items and more for the ones over flat byte values (the LDS heap); the block after a
    deep one, where there is one, is shallow."""
    deep = DT.deep_block_items()
    assert len(deep) >= 12
    leaves = set()
    for it, blk, k in deep:
        assert it.strategy == DT.Z_HUFFMAN_ONLY
        hists = DT.literal_blocks(it.data, it.memlevel)
        depth = DT.huffman_depth(hists[blk])
        assert depth > 15 and (k < 20 or "flat" in it.name or depth >= 19), (it.name, depth)
        n = sum(1 for f in hists[blk] if f)
        assert (n > 63) == ("flat" in it.name or "then_text_m8" in it.name), (it.name, n)
        leaves.add(n > 63)
        if "then_text" in it.name:
            assert len(hists) == 2 and DT.huffman_depth(hists[1]) <= 15, it.name
        else:
            assert len(it.data) <= (1 << (it.memlevel + 6)) - 1, it.name
    assert leaves == {False, True}
    assert DT.huffman_depth(DT.fib_counts(16)) == 15     # the end-of-block symbol's 1 is the chain's last link
    assert [DT.huffman_depth(DT.chain_counts(k)) for k in (17, 18)] == [16, 17]
