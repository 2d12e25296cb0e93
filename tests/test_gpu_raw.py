"""The container extension on the GPU: the anchor kernel against the Python model, raw
deflate against the reference's zlib 1.2.8, the scan's raw records against the model, the opt-in raw walk end
to end, its rule on near-miss bodies, the caps, the ATZ3 reader, the CLI and the shard refusal.

Every expected deflate byte comes from oracle/_ref/libz128.so (zstrat / zraw); the containers are built by
hand (zraw.zip_entry, zraw.gzip_member).  Without the library these tests fail, they do not skip.
"""
import ctypes as C
import hashlib
import os
import random
import struct
import subprocess
import sys

import pytest

import _libs
import zraw
import zstrat
from test_gpu_strategy import dev_copy, gradient, hip, padded, parse_atz, rnd, runs, txt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = ("zip", "gzip")
STRATS = ("filtered", "rle", "huffman")


@pytest.fixture(scope="module")
def ctx():
    import antiz_amd
    with antiz_amd.Context(device=0, containers=BOTH) as c:
        yield c


# ---- 1. anchors ------------------------------------------------------------------------------------
ZIP_FIXED = struct.pack("<4sHHHHHIIIHH", b"PK\3\4", 20, 0, 8, 0x6000, 0x5521, 0x11111111, 77, 99, 0, 0)
GZIP_FIXED = struct.pack("<3sBIBB", b"\x1f\x8b\x08", 0, 0x5f000000, 0, 3)
CHECKED = {zraw.ZIP: (0, 1, 2, 3, 6, 7, 8, 9), zraw.GZIP: (0, 1, 2, 3)}   # header bytes the kernel tests


def anchor_file(variant):
    """About 64 KiB with fixed headers of both kinds, each exactly once, whose magic starts at the edges of a
    lane's 16-byte load, a wave's 1 KiB, a 4 KiB step, the block segment (36 864 here), the file's start and
    its end; `variant` swaps which kind sits where.  Plus near-misses and a 4 KiB stretch of ZIP headers."""
    n = 65536 + 77
    r = random.Random(variant)
    b = bytearray(x if x not in (0x50, 0x1f) else 0x51 for x in r.randbytes(n))
    owned = set()

    def put(p, kind, hdr=None):
        hdr = hdr or (ZIP_FIXED if kind == zraw.ZIP else GZIP_FIXED)
        mine = {p + k for k in CHECKED[kind] if p + k < n}
        assert not mine & owned, p
        for k, x in enumerate(hdr):
            if p + k < n and p + k not in owned:
                b[p + k] = x
        owned.update(mine)

    seg = 36864
    spots = ([0, 16 * 10 + 13, 16 * 14 + 14, 16 * 18 + 15, 1024 * 2 - 1, 1024 * 3 - 2, 1024 * 5 - 3, 4096 * 3 - 1,
              4096 * 4 - 2, 4096 * 5 - 3, seg - 1],
             [16 * 30 + 13, 16 * 32 + 14, 16 * 34 + 15, 1024 * 6 - 1, 1024 * 7 - 2, 1024 * 9 - 3, 4096 * 6 - 1,
              4096 * 7 - 2, 4096 * 10 - 3, 4096 * 11 - 2])
    first, second = (zraw.ZIP, zraw.GZIP) if variant == 0 else (zraw.GZIP, zraw.ZIP)
    for p in spots[0]:
        put(p, first)
    for p in spots[1]:
        put(p, second)
    # the file's end: the last position at which each kind still counts, the first at which it no longer does,
    # and a magic cut off by the end
    if variant == 0:
        put(n - 30, zraw.ZIP)
        put(n - 17, zraw.GZIP)
        put(n - 3, zraw.ZIP)
    else:
        put(n - 29, zraw.ZIP)
        put(n - 18, zraw.GZIP)
        put(n - 3, zraw.GZIP)
    # one step with more than 100 hits across all four waves
    for k in range(4096 // 30):
        put(4096 * 12 + 30 * k, zraw.ZIP)
    # near-misses
    at = 56000
    for hdr in (ZIP_FIXED[:8] + b"\0\0" + ZIP_FIXED[10:],            # method 0 (stored)
                ZIP_FIXED[:8] + b"\x09\0" + ZIP_FIXED[10:],          # method 9 (Deflate64)
                ZIP_FIXED[:8] + b"\x08\x01" + ZIP_FIXED[10:],        # method 0x108
                ZIP_FIXED[:6] + b"\x01\0" + ZIP_FIXED[8:],           # encrypted
                b"PK\3\5" + ZIP_FIXED[4:], b"PK\4\4" + ZIP_FIXED[4:], b"PL\3\4" + ZIP_FIXED[4:],
                b"\x51K\3\4" + ZIP_FIXED[4:]):
        b[at:at + 30] = hdr
        at += 64
    for hdr in (GZIP_FIXED[:3] + b"\x20" + GZIP_FIXED[4:], GZIP_FIXED[:3] + b"\x40" + GZIP_FIXED[4:],
                GZIP_FIXED[:3] + b"\x80" + GZIP_FIXED[4:], b"\x1f\x8b\x09" + GZIP_FIXED[3:],
                b"\x1f\x8c\x08" + GZIP_FIXED[3:], b"\x1e\x8b\x08" + GZIP_FIXED[3:]):
        b[at:at + 10] = hdr
        at += 64
    # (valid ones beside them: flag bits other than bit 0, FLG bits below 0x20)
    put(at, zraw.ZIP, ZIP_FIXED[:6] + b"\x0e\x08" + ZIP_FIXED[8:])
    put(at + 64, zraw.GZIP, GZIP_FIXED[:3] + b"\x1f" + GZIP_FIXED[4:])
    return bytes(b)


@pytest.mark.parametrize("variant", [0, 1])
def test_anchors_match_the_model(ctx, variant):
    data = anchor_file(variant)
    n = len(data)
    want = zraw.anchors(data, 3)
    pos = {p for p, _ in want}
    # the file is what it claims to be
    assert sum(1 for p, _ in want if 4096 * 12 <= p < 4096 * 13) > 100
    assert 0 in pos and 36863 in pos and (n - 30 in pos) == (variant == 0) and (n - 18 in pos) == (variant == 1)
    assert n - 29 not in pos and n - 17 not in pos and n - 3 not in pos
    assert not any(56000 <= p < 56000 + 64 * 14 for p in pos) and 56000 + 64 * 14 in pos and 56000 + 64 * 15 in pos
    assert {k for _, k in want} == {0, 1}
    for mask in (1, 2, 3):
        got = ctx.container_anchors(data, mask)
        assert got == zraw.anchors(data, mask), mask
    assert len(ctx.container_anchors(data, 3)) == len(want) > 150
    assert ctx.container_anchors(data, 0) == []


def test_anchors_in_tiny_files(ctx):
    for data in (GZIP_FIXED + bytes(7), GZIP_FIXED + bytes(8), b"\x1f\x8b\x08", b"PK\3", ZIP_FIXED, ZIP_FIXED[:29],
                 b"x" + ZIP_FIXED, b"x"):
        for mask in (1, 2, 3):
            assert ctx.container_anchors(data, mask) == zraw.anchors(data, mask), (len(data), mask)
    assert ctx.container_anchors(GZIP_FIXED + bytes(8), 2) == [(0, 1)]
    assert ctx.container_anchors(ZIP_FIXED, 1) == [(0, 0)]


# ---- 2. raw deflate --------------------------------------------------------------------------------
def test_raw_deflate_kats(ctx):
    import antiz_amd
    ins = [b"", b"q"] + [b"x" + b"a" * L for L in (3, 4, 257, 258, 259, 517)] + [txt(7, 4096)]
    big = txt(17, 70000)   # window slides at windowBits 9; stored blocks longer than memLevel 1's pending buffer
    buf, offs = bytearray(), []
    for d in ins + [big]:
        offs.append(len(buf))
        buf += d
        buf += b"\0" * (-len(buf) % 16)
    items, want = [], []
    for strat in range(4):
        for lv in range(1 if strat >= 2 else 0, 10):
            for m in (1, 8, 9):
                for w in (9, 15):
                    for i, d in enumerate(ins):
                        items.append((offs[i], len(d), lv, w, m, strat, True))
                        want.append(zstrat.deflate(d, lv, -w, m, strat))
    for lv in range(10):
        for m in (1, 8):
            items.append((offs[len(ins)], len(big), lv, 9, m, 0, True))
            want.append(zstrat.deflate(big, lv, -9, m, 0))
    items.append((offs[len(ins)], len(big), 0, 15, 1, 0, True))
    want.append(zstrat.deflate(big, 0, -15, 1, 0))
    # the wrapped stream beside its body in one batch
    items.append((offs[len(ins) - 1], len(ins[-1]), 6, 15, 8, 0, False))
    want.append(zstrat.deflate(ins[-1], 6, 15, 8, 0))
    got = ctx.deflate_batch(bytes(buf), items)
    bad = [items[k] for k in range(len(items)) if got[k] != want[k]]
    print("raw kats: %d items, %d differ" % (len(items), len(bad)))
    assert not bad, bad[:20]
    assert ctx.deflate(ins[-1], 9, 15, 9, raw=True) == zstrat.deflate(ins[-1], 9, -15, 9)
    assert ctx.deflate(ins[-1], 9, 15, 9, raw=True) == ctx.deflate(ins[-1], 9, 15, 9)[2:-4]
    with pytest.raises(antiz_amd.AtzError) as e:   # an unknown bit of the params word
        prm = (C.c_uint32 * 1)((1 << 29) | (6 << 16) | (15 << 8) | 8)
        z = (C.c_uint64 * 1)(0)
        one = (C.c_uint64 * 1)(1)
        cap = (C.c_uint64 * 1)(64)
        out = C.create_string_buffer(64)
        antiz_amd._check(antiz_amd.lib().atz_deflate_batch_ex(ctx.h, b"a", 1, z, one, prm, 1, out, z, cap, one))
    assert e.value.code == -1


# ---- 3. the scan -------------------------------------------------------------------------------------
def far_payload(seed, nbytes, dist=6000):
    """Random chunks of `dist` bytes, each written twice: every match reaches `dist` bytes back."""
    out, k = bytearray(), 0
    while len(out) < nbytes:
        x = rnd(seed + k, dist)
        out += x + x
        k += 1
    return bytes(out[:nbytes])


def scan_file():
    """-> (file, {name: offset of the body}) over the cases of the scan."""
    r = random.Random(77)
    parts, at, pos = [], {}, 0

    def put(name, blob, body_at):
        nonlocal pos
        fill = txt(r.randrange(1 << 30), r.randrange(50, 300))
        parts.append(fill)
        pos += len(fill)
        at[name] = pos + body_at
        parts.append(blob)
        pos += len(blob)

    def zipped(case, payload, body=None, lv=6, m=8, **kw):
        body = zraw.raw_deflate(payload, lv, m) if body is None else body
        e = zraw.zip_entry(body, kw.pop("usize", len(payload)), **kw)
        put(case, e, 30 + len(kw.get("name", b"")) + len(kw.get("extra", b"")))

    def gzipped(case, payload, lv=6, m=8, **kw):
        body = zraw.raw_deflate(payload, lv, m)
        e = zraw.gzip_member(body, payload, **kw)
        put(case, e, len(e) - len(body) - 8)

    t = [txt(200 + k, 2000 + 300 * k) for k in range(20)]
    zipped("zip plain", t[0])
    zipped("zip name extra", t[1], name=b"dir/file.txt", extra=b"UT\5\0\3abcd", flags=zraw.ZIP_HINT_BITS[zraw.HINT_MAX])
    zipped("zip descriptor", t[2], descriptor=True, flags=zraw.ZIP_HINT_BITS[zraw.HINT_FAST])
    zipped("zip descriptor name", t[3], descriptor=True, name=b"x")
    zipped("zip sizes zero", t[4], csize=0, usize=0)                       # bit 3 clear: usize 0 is stated, and wrong
    zipped("zip usize unknown", t[5], usize=0xffffffff, csize=0xffffffff)
    b6 = zraw.raw_deflate(t[6], 6, 8)
    zipped("zip wrong csize", t[6], body=b6 + b"\0", csize=len(b6) + 1)
    zipped("zip wrong usize", t[7], usize=len(t[7]) + 1)
    b8 = zraw.raw_deflate(t[8], 6, 8)
    zipped("zip truncated", t[8], body=b8[:len(b8) // 2])
    gzipped("gzip plain", t[9])
    gzipped("gzip extra", t[10], extra=b"\1\2\3\4\5", xfl=2)
    gzipped("gzip name", t[11], name=b"file.txt", xfl=4)
    gzipped("gzip comment", t[12], comment=b"a comment")
    gzipped("gzip hcrc", t[13], hcrc=True)
    gzipped("gzip all", t[14], extra=b"xy", name=b"n", comment=b"c", hcrc=True)
    gzipped("gzip wrong isize", t[15], isize=len(t[15]) + 1)
    # a zlib stream inside a stored body: the reference records it, and the raw candidate around it is dropped
    inner = zstrat.deflate(t[16], 6, 15, 8, 0)
    zipped("zip around zlib", txt(1, 500) + inner + txt(2, 500), lv=0)
    # a ZIP entry inside another's stored body: both decode, the outer one starts first and is kept
    nested = zraw.zip_entry(zraw.raw_deflate(t[17], 6, 8), len(t[17]), name=b"inner")
    zipped("zip outer", txt(3, 400) + nested + txt(4, 400), lv=0, name=b"outer")
    at["zip inner"] = at["zip outer"] + 5 + 400 + 35
    # matches further back than the 4 KiB ring; an output past the 64 KiB slot, which loses it: ring retry
    zipped("zip far", far_payload(300, 20000))
    gzipped("gzip long far", far_payload(400, 100000), name=b"big")
    zipped("zip long text", txt(500, 90000), descriptor=True)
    # a name that runs past the end of the file
    parts.append(txt(5, 100))
    parts.append(b"\x1f\x8b\x08\x08" + GZIP_FIXED[4:] + b"name-without-an-end" * 2)
    return b"".join(parts), at


def ref_records(data):
    rc, _, stats = _libs.ora_precompress(data)
    assert rc == 0
    return [(s["offset"], s["comp_len"], s["infl_len"], s["type"]) for s in stats["streams"]]


@pytest.mark.parametrize("mask", [1, 2, 3])
def test_scan_matches_the_model(mask):
    import antiz_amd
    data, at = scan_file()
    ref = ref_records(data)
    raw = zraw.raw_records(data, mask, [(o, cl) for o, cl, _, _ in ref])
    names = [w for w, k in antiz_amd.CONTAINERS.items() if mask >> k & 1]
    with antiz_amd.Context(device=0, containers=names) as c:
        got = [(o, cl, il, ty) for o, ty, cl, il, _ in c.scan(data)]
        res, _ = c.sweep()
    assert got == sorted(ref + raw)
    assert len(res) == len(got)
    # the model sees the cases as they were meant
    kept = {o: ty for o, _, _, ty in raw}
    accepted = ["zip plain", "zip name extra", "zip descriptor", "zip descriptor name", "zip usize unknown", "zip outer",
                "zip far", "zip long text"] if mask & 1 else []
    accepted += ["gzip plain", "gzip extra", "gzip name", "gzip comment", "gzip hcrc", "gzip all",
                 "gzip long far"] if mask & 2 else []
    assert sorted(kept) == sorted(at[k] for k in accepted)
    if mask & 1:
        assert kept[at["zip name extra"]] == 26 and kept[at["zip descriptor"]] == 25 and kept[at["zip plain"]] == 24
        inner = [o for o, cl, _, _ in ref if at["zip around zlib"] < o < at["zip around zlib"] + 600]
        assert inner, "the reference records the zlib stream inside the stored body"
    if mask & 2:
        assert kept[at["gzip extra"]] == 26 and kept[at["gzip name"]] == 25
    # every raw record of this file is a (6, 8) or stored body: recorded exactly, at its container's first hit
    by = {o: k for k, (o, _, _, _) in enumerate(got)}
    for o, cl, il, ty in raw:
        x = res[by[o]]
        want = zraw.rule(data[o:o + cl], zraw.inflate_raw(data[o:o + cl])[1], ty - 24)
        assert (x["recomp"], x["clevel"], x["window"], x["memlevel"], x["ident"], x["n_diff"]) == \
               (1, 0x40 | want["level"], 15, want["memlevel"], cl, 0), o


# ---- 4. end to end -----------------------------------------------------------------------------------
RAW_PARAMS = [(6, 8), (1, 8), (9, 9), (3, 1), (0, 8), (7, 2)]


def build_file(seed=5, containers=True):
    """-> (file, [(offset, comp bytes, payload, kind)]): kind 'd' default zlib stream, 1..3 a strategy stream,
    ('z' | 'g', hint) a raw body in a ZIP entry / gzip member."""
    r = random.Random(seed)
    parts, recs, pos = [], [], 0

    def put(blob, body_at, comp, payload, kind):
        nonlocal pos
        fill = txt(r.randrange(1 << 30), r.randrange(20, 400))
        parts.append(fill)
        pos += len(fill)
        recs.append((pos + body_at, comp, payload, kind))
        parts.append(blob)
        pos += len(blob)

    items = []
    for k, (lv, sz) in enumerate([(6, 4000), (9, 12000), (1, 3000), (6, 900), (4, 7000), (2, 5000)]):
        p = txt(100 + k, sz)
        items.append((zstrat.deflate(p, lv, 15, 8, 0), 0, None, p, "d"))
    for k, (st, lv, m, p) in enumerate([(1, 6, 8, gradient(201, 6000)), (1, 9, 9, gradient(202, 9000)),
                                        (3, 6, 8, runs(203, 3000)), (2, 6, 1, runs(204, 1500))]):
        items.append((zstrat.deflate(p, lv, 15, m, st), 0, None, p, st))
    if containers:
        sizes = [5000, 9000, 3000, 14000, 2500, 7000]
        k = 0
        for wrap in "zg":
            for j, (lv, m) in enumerate(RAW_PARAMS):
                hint = (j + (wrap == "g")) % 3
                p = txt(300 + k, sizes[j])
                body = zraw.raw_deflate(p, lv, m)
                if wrap == "z":
                    e = zraw.zip_entry(body, len(p), name=b"f%d.txt" % k, flags=zraw.ZIP_HINT_BITS[hint], descriptor=bool(j & 1))
                    items.append((e, 30 + len(b"f%d.txt" % k), body, p, ("z", hint)))
                else:
                    e = zraw.gzip_member(body, p, name=b"g%d" % k if j & 1 else None, xfl=zraw.GZIP_XFL[hint])
                    items.append((e, 10 + (len(b"g%d" % k) + 1 if j & 1 else 0), body, p, ("g", hint)))
                k += 1
        p = txt(400, 40)
        body = zraw.raw_deflate(p, 6, 8)
        items.append((zraw.zip_entry(body, 40, name=b"tiny"), 34, body, p, ("z", 0)))
        p = txt(401, 300000)   # the large-stream path
        body = zraw.raw_deflate(p, 6, 8)
        items.append((zraw.gzip_member(body, p), 10, body, p, ("g", 0)))
    r.shuffle(items)
    for blob, body_at, body, p, kind in items:
        put(blob, body_at, blob if body is None else body, p, kind)
    parts.append(txt(9, 333))
    return b"".join(parts), recs


@pytest.fixture(scope="module")
def e2e():
    import antiz_amd
    data, recs = build_file()
    with antiz_amd.Context(device=0) as c:
        off, _ = c.precompress(data)
    with antiz_amd.Context(device=0, containers=BOTH) as c:
        on, st = c.precompress(data)
    with antiz_amd.Context(device=0, containers=BOTH, strategies=STRATS) as c:
        both, _ = c.precompress(data)
    with antiz_amd.Context(device=0, strategies=STRATS) as c:
        strat, _ = c.precompress(data)
    rc, ref, stats = _libs.ora_precompress(data)
    assert rc == 0
    return dict(data=data, recs=recs, off=off, on=on, both=both, strat=strat, ref=ref, ora=stats, st=st)


def test_end_to_end(e2e):
    import antiz_amd
    data, recs = e2e["data"], e2e["recs"]
    assert e2e["off"][:4] == b"ATZ\1" and e2e["off"] == e2e["ref"]   # mask off: the reference's bytes
    ver, origlen, on = parse_atz(e2e["on"])
    _, _, off = parse_atz(e2e["off"])
    assert e2e["on"][:4] == b"ATZ\3" and ver == 3 and origlen == len(data)
    on_by, off_by = {d["off"]: d for d in on}, {d["off"]: d for d in off}
    for o, d in off_by.items():   # every reference-recorded descriptor, byte for byte
        assert on_by[o]["raw"] == d["raw"], o
    n_raw = 0
    for pos, comp, payload, kind in recs:
        if not isinstance(kind, tuple):
            assert (pos in on_by) == (pos in off_by)
            continue
        assert pos not in off_by
        want = zraw.rule(comp, payload, kind[1])
        assert want is not None and want["diff_pos"] == [], (pos, kind)
        d = on_by[pos]
        assert (d["c"], d["w"], d["m"], d["cl"], d["il"], d["nd"]) == \
               (antiz_amd.pack_clevel(0, want["level"], raw=True), 15, want["memlevel"], len(comp), len(payload), 0), pos
        n_raw += 1
    assert n_raw == 14 and len(on) == len(off) + n_raw
    # the 300 000 B body outgrew its 64 KiB slot: decoded again with the 32 KiB ring, re-inflated as a record
    assert e2e["st"]["n_inflate_retries"] >= 1 and e2e["st"]["n_reinflated"] >= 1
    # both masks: the same, plus the strategy extension's records
    assert e2e["strat"][:4] == b"ATZ\2"
    ver, _, both = parse_atz(e2e["both"])
    _, _, strat = parse_atz(e2e["strat"])
    assert ver == 3
    both_by = {d["off"]: d for d in both}
    for d in on + strat:
        assert both_by[d["off"]]["raw"] == d["raw"], d["off"]
    assert len(both) == len(on) + len(strat) - len(off) and len(strat) > len(off)
    with antiz_amd.Context(device=0) as c:
        for atz in (e2e["on"], e2e["both"]):
            assert c.reconstruct(atz) == data
            with dev_copy(atz) as d:
                p, n = c.reconstruct_device(d, atz)
                out = C.create_string_buffer(n)
                assert hip().hipMemcpy(out, p, n, 2) == 0   # device to host
                assert out.raw == data


def test_no_containers_stays_atz1():
    import antiz_amd
    data, _ = build_file(seed=6, containers=False)
    with antiz_amd.Context(device=0) as c:
        off, _ = c.precompress(data)
    with antiz_amd.Context(device=0, containers=BOTH) as c:
        on, _ = c.precompress(data)
    assert on == off and on[:4] == b"ATZ\1"


# ---- 5. the rule against the model ------------------------------------------------------------------
OPTS = [dict(), dict(mismatch_tol=0), dict(recomp_tresh=0), dict(sizediff_tresh=0)]


def nearmiss_file():
    """Raw bodies at memLevel 1 whose payload has a long random middle (stored blocks, one ignored padding field
    each), each as made and with 1, 3 and 140 bytes altered (on the wrapped stream, then unwrapped), in ZIP
    entries and gzip members with every hint.  -> (file, [(offset, body, payload, hint)])"""
    r = random.Random(31)
    base = [(9, txt(501, 5000) + rnd(1, 20000) + txt(502, 4000)), (6, txt(503, 6000) + rnd(2, 19000) + txt(504, 3000)),
            (1, txt(505, 5000) + rnd(3, 20000) + txt(506, 4000)), (4, txt(507, 4000) + rnd(4, 20000) + txt(508, 3000))]
    parts, recs, pos, k = [], [], 0, 0
    for lv, payload in base:
        good = zstrat.deflate(payload, lv, 15, 1, 0)
        assert good[2:-4] == zraw.raw_deflate(payload, lv, 1)
        for alt in (0, 1, 3, 140):
            body = (padded(good, alt) if alt else good)[2:-4]
            hint = k % 3
            if k & 1:
                blob = zraw.gzip_member(body, payload, xfl=zraw.GZIP_XFL[hint])
                body_at = 10
            else:
                blob = zraw.zip_entry(body, len(payload), flags=zraw.ZIP_HINT_BITS[hint], descriptor=bool(k & 2))
                body_at = 30
            fill = txt(r.randrange(1 << 30), 100)
            parts += [fill, blob]
            recs.append((pos + len(fill) + body_at, body, payload, hint))
            pos += len(fill) + len(blob)
            k += 1
    parts.append(txt(3, 200))
    return b"".join(parts), recs


@pytest.mark.parametrize("opts", OPTS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "defaults")
def test_rule_matches_the_model(opts):
    import antiz_amd
    data, recs = nearmiss_file()
    with antiz_amd.Context(device=0, containers=BOTH, **opts) as c:
        scanned = c.scan(data)
        res, diffs = c.sweep()
    lists = _libs.diff_lists(res, diffs)
    by = {s[0]: k for k, s in enumerate(scanned)}
    n_rec = 0
    for pos, body, payload, hint in recs:
        k = by[pos]
        assert scanned[k][1:4] == (24 + hint, len(body), len(payload))
        want = zraw.rule(body, payload, hint, **opts)
        if want is None:
            assert res[k]["recomp"] == 0, pos
            continue
        n_rec += 1
        assert res[k]["recomp"] == 1, pos
        assert (res[k]["clevel"], res[k]["window"], res[k]["memlevel"], res[k]["ident"]) == \
               (0x40 | want["level"], want["window"], want["memlevel"], want["ident"]), pos
        assert lists[k][0] == want["diff_pos"] and bytes(lists[k][1]) == want["diff_val"], pos
    print("rule %s: %d of %d recorded" % (opts, n_rec, len(recs)))
    # four bodies, each exact and 1, 3 and 140 bytes off: 140 > recomp_tresh is never recorded, and with
    # recomp_tresh 0 only the exact ones are
    assert n_rec == (4 if opts.get("recomp_tresh") == 0 else 12)


# ---- 6. caps --------------------------------------------------------------------------------------
CAPS = r"""
import hashlib, sys
sys.path.insert(0, %r)
import antiz_amd
data = open(sys.argv[1], "rb").read()
with antiz_amd.Context(device=0, containers=("zip", "gzip")) as c:
    out, st = c.precompress(data)
    back = c.reconstruct(out)
print(int(back == data))
print(hashlib.sha256(out).hexdigest())
""" % ROOT


@pytest.mark.parametrize("div", ["4096", "1000000000"])
def test_caps_keep_the_bytes(e2e, tmp_path, div):
    path = str(tmp_path / "f.bin")
    with open(path, "wb") as f:
        f.write(e2e["data"])
    r = subprocess.run([sys.executable, "-c", CAPS, path], env=dict(os.environ, ATZ_CAP_DIV=div),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2] == "1"
    assert lines[-1] == hashlib.sha256(e2e["on"]).hexdigest()


# ---- 7. the ATZ3 reader -----------------------------------------------------------------------------
def test_atz3_reader_survives_mutations(e2e):
    import antiz_amd
    good = e2e["on"]
    origlen = struct.unpack_from("<Q", good, 12)[0]
    r = random.Random(2025)
    hot = 28 + 43 * 40   # half the bit flips go to the front, where the first descriptors are
    accepted = refused = 0
    with antiz_amd.Context(device=0) as c:
        for k in range(200):
            b = bytearray(good)
            if k % 4 == 3:
                b = b[:r.randrange(0, len(b))]
            else:
                at = r.randrange(0, hot) if k % 2 else r.randrange(0, len(b))
                b[at] ^= 1 << r.randrange(8)
            try:
                out = c.reconstruct(bytes(b))
            except antiz_amd.AtzError:
                refused += 1
                continue
            accepted += 1
            assert len(out) == origlen
        assert accepted > 0 and refused > 0, (accepted, refused)
        # the same descriptors under an older magic: bit 6 of a clevel byte is invalid there
        for magic in (b"ATZ\1", b"ATZ\2"):
            with pytest.raises(antiz_amd.AtzError):
                c.reconstruct(magic + good[4:])
        # bit 7 of a raw descriptor's clevel byte
        _, _, descs = parse_atz(good)
        at, first_raw = 28, None
        for d in descs:
            if d["c"] & 0x40 and first_raw is None:
                first_raw = at + 24
            at += len(d["raw"])
        b = bytearray(good)
        b[first_raw] |= 0x80
        with pytest.raises(antiz_amd.AtzError):
            c.reconstruct(bytes(b))
        assert c.reconstruct(good) == e2e["data"]


# ---- 8. CLI -----------------------------------------------------------------------------------------
def test_cli_containers(e2e, tmp_path):
    import antiz_amd
    f = str(tmp_path / "f")
    with open(f, "wb") as fh:
        fh.write(e2e["data"])
    env = dict(os.environ, ATZ_CONTAINERS="zip,gzip", ATZ_DEVICE="0")
    r = subprocess.run([antiz_amd.CLI_PATH, "-i", f], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    assert "OK! Restoration is bit by bit identical" in r.stdout
    assert open(f + ".atz", "rb").read() == e2e["on"]
    r = subprocess.run([antiz_amd.CLI_PATH, "-r", "-i", f + ".atz", "-o", f + ".back"], env=dict(os.environ, ATZ_DEVICE="0"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    assert open(f + ".back", "rb").read() == e2e["data"]
    r = subprocess.run([antiz_amd.CLI_PATH, "-i", f], env=dict(env, ATZ_CONTAINERS="zip,rar"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 1 and "ATZ_CONTAINERS: unknown container rar" in r.stderr


# ---- 9. shard refusal -------------------------------------------------------------------------------
def test_shard_scan_refuses_a_mask():
    import antiz_amd
    data = txt(1, 4096) + zstrat.deflate(txt(2, 3000), 6, 15, 8, 0)
    with antiz_amd.Context(device=0, containers=("zip",)) as c:
        with dev_copy(data) as d:
            with pytest.raises(antiz_amd.AtzError) as e:
                c.shard_scan(d, data, 0, 1)
            assert e.value.code == -1
        with pytest.raises(antiz_amd.AtzError) as e:   # an unknown bit of the mask
            antiz_amd._check(antiz_amd.lib().atz_set_containers(c.h, 4))
        assert e.value.code == -1
    with antiz_amd.Context(device=0) as c:
        with dev_copy(data) as d:
            assert c.shard_scan(d, data, 0, 1)
