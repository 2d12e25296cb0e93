"""Parity of the MI355X product (libatz_accel.so, HIP) with the oracle and the reference's golden vectors.

Run on the GPU box: python -m pytest tests -m gpu.  Every test calls through the C ABI
(include/atz_accel.h); integer/byte work must be bit-exact.
"""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import _libs
import golden_cases as G

pytestmark = pytest.mark.gpu

GOLD = G.GOLD
HDRS = [0x2815, 0x2853, 0x2891, 0x28cf, 0x3811, 0x384f, 0x388d, 0x38cb, 0x480d, 0x484b, 0x4889, 0x48c7,
        0x5809, 0x5847, 0x5885, 0x58c3, 0x6805, 0x6843, 0x6881, 0x68de, 0x7801, 0x785e, 0x789c, 0x78da]


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def atz():
    import antiz_amd
    from antiz_amd import build
    build.build()
    return antiz_amd


@pytest.fixture(scope="module")
def ctx(atz):
    c = atz.Context()
    yield c
    c.close()


def inflate_cases(seed=7, n=600):
    r = random.Random(seed)
    out = []
    for k in range(n):
        kind = r.randrange(6)
        if kind == 0:
            d = _libs.text(r, r.randrange(1, 6000))
            s, _ = _libs.ora_deflate(d, r.randrange(0, 10), r.randrange(10, 16), r.randrange(1, 10))
            s = s[:r.randrange(1, len(s) + 1)] if r.random() < 0.5 else s + bytes(r.getrandbits(8) for _ in range(r.randrange(0, 20)))
        elif kind == 1:
            d = _libs.text(r, r.randrange(1, 6000))
            s = bytearray(_libs.ora_deflate(d, r.randrange(1, 10), 15, 8)[0])
            for _ in range(r.randrange(1, 4)):
                p = r.randrange(2, len(s))
                s[p] ^= 1 << r.randrange(8)
            s = bytes(s)
        elif kind == 2:
            h = r.choice(HDRS)
            s = bytes([h >> 8, h & 255]) + bytes(r.getrandbits(8) for _ in range(r.randrange(0, 300)))
        elif kind == 3:
            d = bytes(r.getrandbits(8) for _ in range(r.randrange(1, 400)))
            s = _libs.ora_deflate(d, r.choice([0, 1, 9]), 15, r.randrange(1, 10))[0]
            s = s[:r.randrange(2, len(s))] + bytes(r.getrandbits(8) for _ in range(r.randrange(0, 50)))
        elif kind == 4:
            d = bytes(r.choice(b"\x00\x01\x02\xff") for _ in range(r.randrange(1, 70000 if k % 50 == 0 else 3000)))
            s = _libs.ora_deflate(d, r.randrange(0, 10), r.randrange(10, 16), r.randrange(1, 10))[0]
            if r.random() < 0.3:
                s = s[:r.randrange(1, len(s) + 1)]
        else:
            h = r.choice(HDRS)
            s = bytes([h >> 8, h & 255, r.choice([0x04, 0x05, 0x0c, 0x0d, 0x14, 0x15, 0xed, 0xec, 0x1d])]) + \
                bytes(r.getrandbits(8) for _ in range(r.randrange(0, 200)))
        out.append(s)
    return out


def test_inflate_matches_zlib_semantics(ctx):
    cases = inflate_cases()
    buf = bytearray()
    ranges = []
    for s in cases:
        pad = r_pad = (len(buf) * 7 + 3) % 5      # unaligned starts
        buf += bytes(pad)
        ranges.append((len(buf), len(s)))
        buf += s
    got = ctx.inflate_batch(bytes(buf), ranges)
    bad = []
    for i, s in enumerate(cases):
        want = _libs.ora_inflate(s)
        if tuple(got[i]) != tuple(want):
            bad.append((i, got[i], want, s[:8].hex()))
    assert not bad, bad[:10]


def test_inflate_edge_fixtures(ctx):
    """k_inflate's fast-loop edges against the real zlib 1.2.8's results (tests/golden/inflate_edges.json,
    made by make_inflate_edges.py from oracle/_ref/libzref.so): fixed-code symbols 286/287 and distance
    codes 30/31 deep in the input and inside its last 8 bytes (Z/inffast.c:288, 303; Z/inflate.c:1064,
    1100), distances past the output, incomplete one-code distance trees, oversized HLIT/HDIST, and one
    stream per distance d = 1..258 holding a match of every length 3..258 at that distance -- every
    (i, d) pair of the overlapping copy's v_rcp_f32 modulo (i < 320), whose bytes the Adler-32 trailer
    checks."""
    cases = json.load(open(os.path.join(GOLD, "inflate_edges.json")))["cases"]
    buf = bytearray()
    ranges = []
    for k, c in enumerate(cases):
        s = bytes.fromhex(c["hex"])
        buf += bytes(k % 3)   # unaligned starts
        ranges.append((len(buf), len(s)))
        buf += s
    got = ctx.inflate_batch(bytes(buf), ranges)
    bad = [(c["family"], k, tuple(got[k]), (c["status"], c["consumed"], c["produced"]))
           for k, c in enumerate(cases) if tuple(got[k]) != (c["status"], c["consumed"], c["produced"])]
    assert not bad, bad[:10]
    assert sum(c["family"] == "overlap" for c in cases) == 258


@pytest.mark.parametrize("name", ["asd", "text4k", "rand5k", "input8k"])
def test_deflate_kats_all_params(ctx, name):
    kat = json.load(open(os.path.join(GOLD, "deflate_kat.json")))
    d = open(os.path.join(GOLD, "kat", name + ".bin"), "rb").read()
    items, keys = [], []
    for c in range(10):
        for w in range(9, 16):
            for m in range(1, 10):
                items.append((0, len(d), c, w, m))
                keys.append("%s/%d/%d/%d" % (name, c, w, m))
    outs = ctx.deflate_batch(d, items)
    bad = [k for k, o in zip(keys, outs) if [len(o), sha(o)] != kat["results"][k]]
    assert not bad, bad[:20]


def test_deflate_random_vs_oracle(ctx):
    r = random.Random(99)
    rng = np.random.default_rng(99)
    from antiz_amd import datagen
    buf = bytearray()
    items = []
    for k in range(400):
        kind = k % 4
        if kind == 0:
            d = datagen.text(rng, r.randrange(1, 60000))
        elif kind == 1:
            d = bytes(r.choice(b"ab") for _ in range(r.randrange(1, 20000)))
        elif kind == 2:
            d = rng.integers(0, 256, size=r.randrange(1, 9000), dtype=np.uint8).tobytes()
        else:
            d = (b"\0" * r.randrange(0, 5000)) + datagen.text(rng, r.randrange(1, 9000)) + b"\xff" * r.randrange(0, 3000)
        items.append((len(buf), len(d), r.randrange(0, 10), r.randrange(9, 16), r.randrange(1, 10)))
        buf += d
    outs = ctx.deflate_batch(bytes(buf), items)
    bad = []
    for it, o in zip(items, outs):
        want, _ = _libs.ora_deflate(bytes(buf[it[0]:it[0] + it[1]]), it[2], it[3], it[4])
        if o != want:
            first = next((i for i in range(min(len(o), len(want))) if o[i] != want[i]), min(len(o), len(want)))
            bad.append((it[1:], len(o), len(want), first))
    assert not bad, bad[:10]


def test_long_streams_windowed_match_tables_vs_oracle(ctx):
    """Streams past one k_match_lds block's window (> 48 KiB: C3's PNG-like streams): the host cuts their
    match jobs into position ranges, each staging [p0 - MAX_DIST, p1 + 282) in LDS, with bucket
    predecessors below the window staged as chain ends.  Every level, windows 9-15, text and filtered-
    image-like data of 49-200 KB, bit-exact against the oracle."""
    r = random.Random(4242)
    rng = np.random.default_rng(4242)
    from antiz_amd import datagen
    buf = bytearray()
    items = []
    for k in range(120):
        n = r.randrange(49000, 200000 if k % 6 == 0 else 90000)
        if k % 3 == 2:   # PNG-like rows: small deltas, many zeros, long runs of short matches
            w = r.randrange(64, 512)
            img = np.cumsum(rng.integers(-3, 4, size=(n // (3 * w) + 1, 3 * w)), axis=1) % 256
            d = np.diff(img, axis=1, prepend=0).astype(np.uint8).tobytes()[:n]
        else:
            d = datagen.text(rng, n)
        items.append((len(buf), len(d), k % 10, 9 + (k // 10) % 7, 1 + (k * 7) % 9))
        buf += d
    outs = ctx.deflate_batch(bytes(buf), items)
    bad = []
    for it, o in zip(items, outs):
        want, _ = _libs.ora_deflate(bytes(buf[it[0]:it[0] + it[1]]), it[2], it[3], it[4])
        if o != want:
            first = next((i for i in range(min(len(o), len(want))) if o[i] != want[i]), min(len(o), len(want)))
            bad.append((it[1:], len(o), len(want), first))
    assert not bad, bad[:10]


def test_fast_levels_holes_vs_oracle(ctx):
    """deflate_fast (levels 1-3) on repetitive text: long matches leave many positions uninserted
    ("holes") and chains exhaust their budget, which exercises the hole-slot check, the visited-node
    insertion check (levels 1-2) and the exact fallback walk against the oracle, every memLevel."""
    r = random.Random(1234)
    words = [bytes(r.choice(b"abcdefgh") for _ in range(r.randrange(2, 7))) for _ in range(r.choice([5, 12, 40]))]
    buf = bytearray()
    items = []
    for k in range(216):
        vocab = words[:r.choice([3, 5, len(words)])]
        n = r.randrange(200, 40000)
        d = bytearray()
        while len(d) < n:
            d += r.choice(vocab) + (b" " if r.random() < 0.8 else b"\n")
        d = bytes(d[:n])
        items.append((len(buf), len(d), 1 + k % 3, 15 if k % 4 else r.randrange(9, 15), 1 + (k // 3) % 9))
        buf += d
    outs = ctx.deflate_batch(bytes(buf), items)
    bad = []
    for it, o in zip(items, outs):
        want, _ = _libs.ora_deflate(bytes(buf[it[0]:it[0] + it[1]]), it[2], it[3], it[4])
        if o != want:
            first = next((i for i in range(min(len(o), len(want))) if o[i] != want[i]), min(len(o), len(want)))
            bad.append((it[1:], len(o), len(want), first))
    assert not bad, bad[:10]


def test_zt_kat_precompress(atz):
    data, meta = G.zt_kat()
    with atz.Context() as c:
        out, st = c.precompress(data)
        assert sha(out) == meta["atz_sha256"]
        assert c.reconstruct(out) == data


@pytest.mark.parametrize("case", G.cases(), ids=lambda c: c["name"])
def test_golden_case(atz, case):
    data = G.case_input(case)
    o = case["opts"]
    with atz.Context(recomp_tresh=o.get("recomp_tresh", 128), sizediff_tresh=o.get("sizediff_tresh", 128),
                     shortcut_len=o.get("shortcut_len", 512), mismatch_tol=o.get("mismatch_tol", 2),
                     chunksize=o.get("chunksize", 524288), brute_window=bool(o.get("brute_window", 0))) as c:
        out, st = c.precompress(data)
        assert sha(out) == case["atz_sha256"], (case["name"], st)
        assert c.reconstruct(out) == data


def test_scan_and_sweep_tables_match_oracle(atz):
    from antiz_amd import datagen
    data = datagen.gen_c4(seed=123, n_streams=60, workers=1)
    rc, atz_bytes, st = _libs.ora_precompress(data, chunksize=65536)
    assert rc == 0
    with atz.Context(chunksize=65536) as c:
        recs = c.scan(data)
        want = [(s["offset"], s["type"], s["comp_len"], s["infl_len"]) for s in st["streams"]]
        assert [r[:4] for r in recs] == want
        res, diffs = c.sweep()
        got = [(r["clevel"], r["window"], r["memlevel"], r["ident"], r["recomp"]) for r in res]
        exp = [(s["clevel"], s["window"], s["memlevel"], s["ident"], s["recomp"]) for s in st["streams"]]
        assert got == exp
        # the diff lists (first_diff, n_diff, diff_index into diff_off / diff_val) of the recompressed streams
        for r, s, (pos, val) in zip(res, st["streams"], _libs.diff_lists(res, diffs)):
            assert (r["n_diff"], pos, val) == (s["n_diff"], s["diff_pos"], s["diff_val"]), s["offset"]
            if s["n_diff"]:
                assert r["first_diff"] == s["first_diff"]
        assert len(diffs[0]) == sum(s["n_diff"] for s in st["streams"])


def test_roundtrip_large_mixed(atz):
    """Size-independent property at a bigger size: -r restores the input bit-exactly."""
    from antiz_amd import datagen
    data = datagen.gen_c4(seed=77, n_streams=1500, workers=4) + datagen.gen_c3(seed=78, total=4_000_000, workers=4)
    with atz.Context() as c:
        out, st = c.precompress(data)
        assert st["n_streams"] > 1000
        assert c.reconstruct(out) == data


def test_far_history_and_ring_retry(atz):
    """The 4 KiB-ring decoder: matches beyond the ring read the job's HBM output; a stream longer than
    its 64 KiB arena slot loses that copy and is rerun on the 32 KiB ring.  Streams with long-distance
    matches (a repeated 20 KiB block) of 30 KiB .. 400 KiB output, at every window, must give the
    oracle's .atz bytes."""
    rng = random.Random(11)
    parts = []
    for k, (n, w) in enumerate([(30000, 15), (90000, 15), (400000, 15), (70000, 14), (50000, 13)]):
        block = _libs.text(rng, 20000)
        d = (block * (n // len(block) + 1))[:n]
        s, _ = _libs.ora_deflate(d, [6, 9, 1, 4, 6][k], w, 8)
        parts.append(bytes(rng.getrandbits(8) for _ in range(17)) + s)
    data = b"".join(parts)
    rc, ref, st_ref = _libs.ora_precompress(data, chunksize=1 << 22)
    assert rc == 0
    with atz.Context(chunksize=1 << 22) as c:
        out, st = c.precompress(data)
        assert st["n_streams"] == 5
        assert st["n_inflate_retries"] >= 1, st       # the 400 KiB stream overflowed its slot
        assert sha(out) == sha(ref)
        assert c.reconstruct(out) == data
    # direct batch inflate into exact destinations (far reads from the destination buffer)
    with atz.Context() as c:
        offs, lens, pos = [], [], 0
        for p in parts:
            offs.append(pos + 17); lens.append(len(p) - 17); pos += len(p)
        got = c.inflate_batch(data, list(zip(offs, lens)))
        for (rc2, cons, prod), l in zip(got, lens):
            assert rc2 == 0 and cons == l


def test_bucket_sort_matches_inorder_kernels(atz):
    """k_buckets_sort (LDS radix sort of the positions by hash) against the in-order bucket kernels,
    array for array and the deepest bucket it reports (ATZ_BUCKETS_VERIFY=1 rebuilds every job both ways
    and fails on any difference),
    over every memLevel and stream sizes from empty to past the sort's LDS limit; the deflates must
    still equal the oracle's."""
    from antiz_amd import datagen
    rng = np.random.default_rng(5)
    r = random.Random(5)
    buf = bytearray()
    items = []
    sizes = [0, 1, 2, 3, 4, 63, 64, 65, 1000, 4094, 4096, 4097, 8191, 12289, 16384, 20481, 25900, 25999, 30000,
             40000, 65400, 70000]
    for k, n in enumerate(sizes * 2):
        kind = k % 3
        if kind == 0:
            d = datagen.text(rng, n)
        elif kind == 1:
            d = bytes(r.choice(b"ab") for _ in range(n))
        else:
            d = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        for m in range(1, 10):
            items.append((len(buf), len(d), 1 + (k + m) % 9, 15, m))
        buf += d
    os.environ["ATZ_BUCKETS_VERIFY"] = "1"
    try:
        with atz.Context() as c:
            outs = c.deflate_batch(bytes(buf), items)
    finally:
        del os.environ["ATZ_BUCKETS_VERIFY"]
    bad = []
    for it, o in zip(items, outs):
        want, _ = _libs.ora_deflate(bytes(buf[it[0]:it[0] + it[1]]), it[2], it[3], it[4])
        if o != want:
            bad.append(it[1:])
    assert not bad, bad[:10]


def test_bench_config_slice_matches_oracle(atz):
    """Parity at the configuration bench.py times: the first 1 600 streams of the C4 workload itself
    (same generator and seed; > 768 streams, so the sweep runs on all 3 pipes with multi-trial
    speculative rounds), default options.  The .atz bytes, the stream table and every stream's
    chosen parameters, ident and recomp decision must equal the oracle's."""
    from antiz_amd import datagen
    data = datagen.gen_c4(seed=4, n_streams=1600, workers=4)
    rc, ref, st_ref = _libs.ora_precompress(data)
    assert rc == 0
    with atz.Context() as c:
        recs = c.scan(data)
        assert [r[:4] for r in recs] == [(s["offset"], s["type"], s["comp_len"], s["infl_len"]) for s in st_ref["streams"]]
        res, _ = c.sweep()
        got = [(r["clevel"], r["window"], r["memlevel"], r["ident"], r["recomp"]) for r in res]
        exp = [(s["clevel"], s["window"], s["memlevel"], s["ident"], s["recomp"]) for s in st_ref["streams"]]
        assert got == exp
        # the scan's first-block memLevel (candidate flags bits 2-5: a multi-block stream's first block
        # holds lit_bufsize - 1 symbols) names the memLevel the sweep found for every exactly
        # reproduced stream it is set for
        hinted = [((r[4] >> 2) & 15, s) for r, s in zip(recs, st_ref["streams"])]
        full = [(h, s["memlevel"]) for h, s in hinted if h and s["ident"] == s["comp_len"]]
        assert len(full) > 600 and all(h == m for h, m in full), [x for x in full if x[0] != x[1]][:10]
        out, st = c.precompress(data)
        assert st["n_streams"] > 1500 and st["n_recomp"] == st["n_streams"]
        assert sha(out) == sha(ref)


def test_c5_brute_window_slice_matches_oracle(atz):
    """BASELINE configs[4] (C5) as a parity case: the first 900 streams of `bench.py --workload c5`
    (windowBits U10-15, seed 5) with --brute-window, so the sweep runs every header window and, for
    streams left >= mismatch_tol short, the extra windows (main.cpp:590-600).  The scan table, each
    stream's chosen (clevel, window, memLevel), ident and recomp, and the .atz bytes must equal the
    oracle's."""
    from antiz_amd import datagen
    data = datagen.gen_c5(seed=5, n_streams=900, workers=4)
    rc, ref, st_ref = _libs.ora_precompress(data, brute=1)
    assert rc == 0
    with atz.Context(brute_window=True) as c:
        recs = c.scan(data)
        assert [r[:4] for r in recs] == [(s["offset"], s["type"], s["comp_len"], s["infl_len"]) for s in st_ref["streams"]]
        res, _ = c.sweep()
        got = [(r["clevel"], r["window"], r["memlevel"], r["ident"], r["recomp"]) for r in res]
        exp = [(s["clevel"], s["window"], s["memlevel"], s["ident"], s["recomp"]) for s in st_ref["streams"]]
        assert got == exp
        assert len({s["window"] for s in st_ref["streams"]}) == 6
        out, st = c.precompress(data)
        assert sha(out) == sha(ref)


MAXDIST_EDGE_SHA = "d75a2a586f840cd037952b7289852f11c4702d92dbefef4b6112824d68680f32"   # real reference


def test_maxdist_edge_streams(atz):
    """The MAX_DIST edge (tests/golden/maxdist_edge.bin, pinned by the real reference in
    test_oracle.py): deflate_fast walks a hash head at distance exactly MAX_DIST but later chain nodes
    only above it, so (a) a hole that is the table's head can hide such a node from the table walk
    (w11 stream, levels 1-3), and (b) symbol replays across memLevels are not exact for streams
    longer than MAX_DIST (w13/w14 streams).  One-shot deflates at every (clevel, memLevel) of each
    stream's window against the oracle, and the ATZ1 bytes with and without --brute-window."""
    import zlib
    data = open(os.path.join(GOLD, "maxdist_edge.bin"), "rb").read()
    with atz.Context() as c:
        recs = c.scan(data)
        assert len(recs) == 11
        bad = []
        for off, typ, cl, il in (r[:4] for r in recs):
            d = zlib.decompress(data[off:off + cl])
            w = 10 + typ // 4
            for lv in range(1, 10):
                for m in range(1, 10):
                    if c.deflate(d, lv, w, m) != _libs.ora_deflate(d, lv, w, m)[0]:
                        bad.append((off, lv, w, m))
        assert not bad, bad[:10]
    for brute in (False, True):
        with atz.Context(brute_window=brute) as c:
            out, _ = c.precompress(data)
            assert sha(out) == MAXDIST_EDGE_SHA


def test_reconstruct_rejects_crafted_atz(atz):
    """Size fields of an ATZ1 file are untrusted: counts and lengths that overflow, overlap or point
    past the file must give ATZ_E_FORMAT (the reference would abort or read out of bounds), never a
    crash or a huge allocation."""
    import struct
    data = open(os.path.join(GOLD, "zt", "input.bin"), "rb").read()[:3000]
    s, _ = _libs.ora_deflate(_libs.text(random.Random(3), 5000), 6, 15, 8)
    data = data + s + b"tail"
    with atz.Context() as c:
        good, _ = c.precompress(data)
        assert c.reconstruct(good) == data
        n = len(good)

        def fix(b):
            b = bytearray(b)
            b[4:12] = struct.pack("<Q", len(b))
            return bytes(b)
        bad = []
        b = bytearray(good); b[20:28] = struct.pack("<Q", 1 << 62); bad.append(bytes(b))              # stream count
        b = bytearray(good); b[28 + 16:28 + 24] = struct.pack("<Q", (1 << 64) - 30); bad.append(bytes(b))   # infl_len wraps
        b = bytearray(good); b[28 + 27:28 + 35] = struct.pack("<Q", 1 << 61); bad.append(bytes(b))    # diff count
        b = bytearray(good); b[28 + 8:28 + 16] = struct.pack("<Q", 1 << 63); bad.append(bytes(b))     # comp_len
        b = bytearray(good); b[28:36] = struct.pack("<Q", (1 << 64) - 1); bad.append(bytes(b))       # offset
        bad.append(fix(good[:n // 2]))                                                               # truncated
        for k, x in enumerate(bad):
            with pytest.raises(atz.AtzError):
                c.reconstruct(x)


def test_sweep_requires_its_scan(atz):
    """atz_sweep works only on the records of the context's previous call, atz_scan; any other call
    in between (here a deflate) replaces them, and the sweep is refused instead of reading stale
    state."""
    from antiz_amd import datagen
    data = datagen.gen_c2(seed=9, n=20)
    with atz.Context() as c:
        c.scan(bytes(data))              # a temporary: the scanned buffer may be released after the scan
        c.deflate(b"hello hello hello", 6, 15, 8)
        with pytest.raises(atz.AtzError):
            c.sweep()
        recs = c.scan(data)
        res, _ = c.sweep()
        assert len(res) == len(recs) == 20


def _atz1(orig_len, streams, residue):
    """ATZ1 bytes: streams = [(offset, comp_len, infl bytes, c, w, m, first_diff,
    deltas, values)]."""
    import struct
    body = b""
    for off, cl, infl, c, w, m, fd, deltas, vals in streams:
        body += struct.pack("<QQQBBBQ", off, cl, len(infl), c, w, m, len(deltas))
        if deltas:
            body += struct.pack("<Q", fd) + b"".join(struct.pack("<Q", d) for d in deltas) + bytes(vals)
        body += infl
    n = 28 + len(body) + len(residue)
    return b"ATZ\x01" + struct.pack("<QQQ", n, orig_len, len(streams)) + body + residue


def test_reconstruct_diffs_match_oracle(atz):
    """Diff patching (main.cpp:916-926) as the reference does it, sequentially: repeated positions
    (zero deltas) keep the last byte, positions past comp_len are dropped, a stream whose deflate is
    shorter than comp_len is zero-extended; every case against the oracle's reconstruct."""
    r = random.Random(11)
    text = _libs.text(r, 3000)
    real, _ = _libs.ora_deflate(text, 6, 15, 8)
    cl = len(real)
    cases = [
        (0, [0, 3, 0, 0, 7], [1, 2, 3, 4, 5]),                 # repeated positions: the last byte wins
        (5, [0, 1, 1, 1 << 40], [9, 8, 7, 6]),                  # a position far past comp_len
        (cl - 2, [0, 1, 5], [0xaa, 0xbb, 0xcc]),                # straddling the end of the stream
    ]
    with atz.Context() as c:
        for fd, deltas, vals in cases:
            for extra in (0, 9):                               # comp_len beyond the deflate output: zeros
                a = _atz1(cl + extra + 6, [(2, cl + extra, text, 6, 15, 8, fd, deltas, vals)], b"ab" + b"wxyz")
                rc, want = _libs.ora_reconstruct(a)
                assert rc == 0
                assert c.reconstruct(a) == want


def test_reconstruct_device_roundtrip(atz):
    """atz_reconstruct_device (ATZ1 resident in HBM) restores a C4 slice bit-exactly."""
    import ctypes
    from antiz_amd import datagen
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    data = datagen.gen_c4(seed=13, n_streams=300)
    with atz.Context() as c:
        a, _ = c.precompress(data)
        d = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(d), len(a) + 4096) == 0
        try:
            assert hip.hipMemcpy(d, a, len(a), 1) == 0                      # host to device
            p, n = c.reconstruct_device(d.value, a)
            assert n == len(data)
            out = ctypes.create_string_buffer(n)
            assert hip.hipMemcpy(out, p, n, 2) == 0                         # device to host
            assert out.raw == data
        finally:
            hip.hipFree(d)


def test_continuation_probe_rerun(atz):
    """A stored-block stream that crosses a chunk boundary decodes straight through the duplicated
    byte (main.cpp:207-217), past the continuation probe: the scan must redo it with the whole next
    buffer and end exactly where the reference does."""
    import zlib
    r = random.Random(5)
    noise = bytes(r.getrandbits(8) for _ in range(150000))
    payload = bytes(r.getrandbits(8) for _ in range(400000))
    for body in (zlib.compress(payload, 0), zlib.compress(payload[:120000], 0)):
        data = noise + body + b"tail" * 10
        for cs in (200000, 524288):
            rc, want, _ = _libs.ora_precompress(data, chunksize=cs)
            assert rc == 0
            with atz.Context(chunksize=cs) as c:
                got, _ = c.precompress(data)
            assert got == want


def test_symbol_replay_matches_oracle(atz):
    """Symbol replay (a trial reuses the symbol sequence another memLevel's trial of the stream saved
    at the same level and window, unchecked when both walks are budget-free, else after matching the
    saver's read table entries): streams whose parameters sit late in their trial lists, so most of
    their trials are replays, with text of a small vocabulary (deep buckets: checked replays) and of
    a large one (budget-free), blocks of every lit_bufsize, end-of-input literals, and windows that
    slide (never replayed); duplicate trials (outputs provably equal to an earlier trial's, same level
    or levels 7-9) are not launched.  The .atz bytes must equal the oracle's."""
    rng = random.Random(21)
    small = ["".join(rng.choice("etaoinshr") for _ in range(rng.randint(1, 5))) for _ in range(40)]
    parts = []
    params = [(2, 15, 1), (3, 15, 2), (4, 15, 1), (5, 15, 3), (3, 15, 1), (7, 15, 1), (8, 15, 2), (9, 15, 1),
              (6, 15, 1), (7, 15, 9), (2, 15, 9), (9, 12, 1), (4, 10, 2), (1, 15, 1)]
    for k in range(84):
        c, w, m = params[k % len(params)]
        n = rng.choice([300, 1500, 4000, 9000, 17000, 24000])
        if k % 2:
            d = " ".join(rng.choice(small) for _ in range(n // 3)).encode()[:n]
        else:
            d = _libs.text(rng, n)
        s, _ = _libs.ora_deflate(d, c, w, m)
        parts.append(bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 40))) + s)
    data = b"".join(parts)
    rc, ref, _ = _libs.ora_precompress(data)
    assert rc == 0
    with atz.Context() as c:
        out, st = c.precompress(data)
        assert st["n_trials_replayed"] > 100, st
        assert st["n_replay_checked"] > 0, st
        assert st["n_trials_duplicate"] > 0, st   # skipped: same-level single-block replays, levels 7-9 twins
        assert sha(out) == sha(ref)
        assert c.reconstruct(out) == data


CLI_CASES = [
    ("c1", []),                                        # precompress + the default verify
    ("c4s", ["--notest", "--chunksize", "65536"]),
    ("c5s", ["--notest", "--brute-window", "-o", "out.atz"]),
    ("c4s", ["--recomp-tresh", "16", "--shortcut-len", "256", "--mismatch-tol", "0"]),
    ("missing", []),                                   # error path: input file not found
]


@pytest.mark.skipif(not os.path.exists(_libs.REF_UNCOMP), reason="reference build (oracle/_ref) not present")
@pytest.mark.parametrize("inp,args", CLI_CASES, ids=lambda v: v if isinstance(v, str) else "_".join(v) or "default")
def test_cli_matches_reference(atz, tmp_path, inp, args):
    """The uncomp CLI (antiz_amd/csrc/uncomp.cpp) against the reference's own CLI
    (oracle/_ref/uncomp, main.cpp:1066-1231) on the same input in twin directories: the same stdout,
    exit code and output files (.atz, the .rec it leaves or deletes), then -r of the .atz."""
    import subprocess
    from antiz_amd import datagen, build
    mine = os.path.join(os.path.dirname(build.LIB), "uncomp")
    data = {"c1": lambda: datagen.gen_c1(), "c4s": lambda: datagen.gen_c4(seed=11, n_streams=150, workers=1),
            "c5s": lambda: datagen.gen_c5(seed=12, n_streams=120, workers=1), "missing": lambda: None}[inp]()
    runs = {}
    for who, exe in (("ref", _libs.REF_UNCOMP), ("mine", mine)):
        d = tmp_path / who
        d.mkdir()
        if data is not None:
            (d / "in.bin").write_bytes(data)
        r = subprocess.run([exe, "-i", "in.bin"] + args, cwd=d, capture_output=True, text=True, timeout=300)
        files = {f: (d / f).read_bytes() for f in sorted(os.listdir(d))}
        runs[who] = (r.returncode, r.stdout, files)
        if data is not None:
            atzname = "out.atz" if "-o" in args else "in.bin.atz"
            r2 = subprocess.run([exe, "-i", atzname, "-r"], cwd=d, capture_output=True, text=True, timeout=300)
            runs[who + "-r"] = (r2.returncode, r2.stdout, {f: (d / f).read_bytes() for f in sorted(os.listdir(d))})
    for k in ("", "-r"):
        if "ref" + k not in runs:
            continue
        rc_ref, out_ref, f_ref = runs["ref" + k]
        rc_me, out_me, f_me = runs["mine" + k]
        assert (rc_me, out_me) == (rc_ref, out_ref), (k, out_me, out_ref)
        assert sorted(f_me) == sorted(f_ref), k
        assert all(f_me[f] == f_ref[f] for f in f_ref), k


def test_speculative_scan_withdrawal(atz, monkeypatch):
    """The scan hands its records to the sweep before the first continuations are decoded, assuming
    each fails; the real ones then re-run the replay, and a different record list withdraws the sweep
    and restarts it.  ATZ_SPEC_ABORT_TEST=1 takes that path on every call: the ATZ1 bytes must still
    be the oracle's (golden chunk-boundary cases, and a 400-stream C4 slice over 3 pipes)."""
    from antiz_amd import datagen
    monkeypatch.setenv("ATZ_SPEC_ABORT_TEST", "1")
    cases = {c["name"]: c for c in G.cases()}
    for name in ("chunk_default", "chunk_4096", "chunk_777", "eof_multiple"):
        case = cases[name]
        with atz.Context(chunksize=case["opts"].get("chunksize", 524288)) as c:
            out, _ = c.precompress(G.case_input(case))
            assert sha(out) == case["atz_sha256"], name
    data = datagen.gen_c4(seed=21, n_streams=400, workers=2)
    rc, ref, _ = _libs.ora_precompress(data, chunksize=65536)
    assert rc == 0
    with atz.Context(chunksize=65536) as c:
        out, st = c.precompress(data)
        assert sha(out) == sha(ref) and st["n_continuations"] > 0


# What oracle/ora_pipeline.c returns where the reference's behaviour is undefined: chunksize < 2 (-2), a
# stream past EOF (-10), a re-inflate that fails (-11), the uint64 wrap in the residue copy (-20), an empty
# input (-21).  Its other codes (-1, -12: allocation or deflate failures) are failures of the oracle itself.
ORACLE_UB_CODES = (-2, -10, -11, -20, -21)


@pytest.mark.parametrize("n,seed", [(160, 20261018), (800, 7)], ids=["pinned", "wide"])
def test_fuzz_small_files_vs_oracle(atz, n, seed):
    """Seeded random small files (tests/golden_cases.py fuzz_cases) under chunk sizes from 2 bytes up
    (streams cross chunk boundaries, pending streams refill many times, main.cpp:205-246 and 405-415),
    default and non-default thresholds: the ATZ1 bytes (or the error code) equal the oracle's, which
    tests/golden/fuzz_small.json pins to the real reference's on the first seed's 160 cases (the wide
    seed's 800 against the oracle alone; 1 500 passed once, gpurun_out/fuzz); every ATZ1 reconstructs its input."""
    for i, data, cs, opts in G.fuzz_cases(n, seed):
        rc, want, _ = _libs.ora_precompress(data, chunksize=cs, **G.opts_kwargs(opts))
        with atz.Context(chunksize=cs, **opts) as c:
            if rc != 0:   # the oracle's reference-UB codes (its own numbering): the library must fail too
                assert rc in ORACLE_UB_CODES, (i, len(data), cs, opts, rc)   # any other failure is the oracle's own
                with pytest.raises(atz.AtzError) as ei:
                    c.precompress(data)
                assert ei.value.code == -6, (i, len(data), cs, opts)   # ATZ_E_REF_UB
                continue
            got, _ = c.precompress(data)
            assert got == want, (i, len(data), cs, opts)
            assert c.reconstruct(got) == data, (i, len(data), cs, opts)


def test_reconstruct_fuzzed_atz_rejected_or_equal_to_oracle(atz):
    """ATZ1 files are untrusted input: seeded single-byte mutations and truncations of valid files
    (fuzz cases with streams and diffs) must either be refused with AtzError or reconstruct exactly what
    the oracle's ATZ1 reader (the reference's reconstructATZ restated) makes of them -- never a crash.
    Mutations land mostly in the header and the stream descriptors (offsets, lengths, parameters, diff
    lists), the rest in the payloads."""
    import struct
    r = random.Random(4242)
    files = []
    for i, data, cs, opts in G.fuzz_cases(400, 99):
        if len(files) == 30:
            break
        rc, want, st = _libs.ora_precompress(data, chunksize=cs, **G.opts_kwargs(opts))
        if rc == 0 and len(want) > 40 and st["streams"]:
            files.append((data, want, opts))
    assert len(files) >= 20
    accepted = refused = 0
    with atz.Context() as c:
        for data, good, opts in files:
            assert c.reconstruct(good) == data
            for _ in range(25):
                b = bytearray(good)
                if r.random() < 0.15:
                    b = b[:r.randrange(28, len(b))]
                    b[4:12] = struct.pack("<Q", len(b))   # keep the length field consistent
                else:
                    hi = min(len(b), 28 + 43 * 3) if r.random() < 0.8 else len(b)
                    at = r.randrange(12, hi)             # past the magic and the length field
                    b[at] = r.randrange(256) if r.random() < 0.5 else b[at] ^ (1 << r.randrange(8))
                b = bytes(b)
                try:
                    got = c.reconstruct(b)
                except atz.AtzError:
                    refused += 1
                    continue
                rc, want = _libs.ora_reconstruct(b)   # only files the library accepted reach the oracle
                assert rc == 0 and got == want
                accepted += 1
    assert accepted > 0 and refused > 0
