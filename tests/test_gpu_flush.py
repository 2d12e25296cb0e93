"""The segment extension on the GPU: the marker kernel and the segment decoder against the model
(tests/zflush.py), the exact deflate's flush end against the reference's zlib 1.2.8 driven with Z_FULL_FLUSH, the
split end to end (scan, walk, ATZ6 file, reconstruct, CLI, probe, GNU trials), the switch's off state, near misses,
the reader and the limits."""
import hashlib
import os
import random
import subprocess
import sys
import zlib

import pytest

import zflush
import zgnu
import zraw
import zstrat
from test_gpu_strategy import dev_copy, parse_atz, txt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = ("zip", "gzip")
FLUSH = ("flush",)
M = zflush.MARKER


def rnd(seed, n):
    return random.Random(seed).randbytes(n)


def filler(seed, n):
    """random bytes that hold no marker and start no container or zlib stream worth a record"""
    d = bytearray(rnd(seed, n))
    for q in zflush.markers(bytes(d)):
        d[q] = 1
    return bytes(d)


@pytest.fixture(scope="module")
def plain():
    import antiz_amd
    with antiz_amd.Context(device=0) as c:
        yield c


# ---- 1. markers ----------------------------------------------------------------------------------------
def planted(n=70000):
    """Markers at every seam of the 16-byte load and of the 4 KiB step, across the two blocks' segment boundary
    (36 864 for this length), overlapping, and up to the end."""
    d = bytearray(filler(1, n))
    seg = ((n + 1) // 2 + 4095) & ~4095
    for base in (16, 4096, 8192, seg, 2 * 4096 + 16 * 255):
        for k, delta in enumerate(range(-5, 3)):
            at = base + 64 * k + delta   # (one marker per 64 bytes: each seam offset on its own load)
            d[at:at + 4] = M
    for delta in range(-4, 1):           # straddling the seams themselves
        at = {0: 4096 * 3, -1: 4096 * 4, -2: 4096 * 5, -3: seg + 4096, -4: 160}[delta] + delta
        d[at:at + 4] = M
    d[1000:1008] = M + M                 # overlapping patterns: 00 00 FF FF 00 00 FF FF
    d[2000:2006] = b"\x00\x00" + M       # 00 00 00 00 FF FF
    d[n - 4:n] = M                       # q + 4 == n
    return bytes(d)


def test_markers_equal_the_model(plain):
    d = planted()
    want = zflush.markers(d)
    assert len(want) >= 48 and want[-1] == len(d) - 4
    assert plain.flush_markers(d) == want
    for cut in (1, 2, 3):                # the last marker cut off at n - 1, n - 2, n - 3
        assert plain.flush_markers(d[:-cut]) == want[:-1]
    for n in (0, 1, 2, 3):
        assert plain.flush_markers(M[:n]) == []
    assert plain.flush_markers(M) == [0] and plain.flush_markers(b"\x00" + M) == [1]
    dense = M * 3000 + b"\x00\x00\xff"   # 4-byte period over three 4 KiB steps: every lane counts
    assert plain.flush_markers(dense) == list(range(0, 12000, 4))
    short = d[:36864 + 3]                # one block whose last marker would need bytes past n
    assert plain.flush_markers(short) == zflush.markers(short)


# ---- 2. the segment decoder -----------------------------------------------------------------------------
def test_segment_decode_equals_the_model(plain):
    t = txt(3, 5000)
    big = txt(4, 200000)                 # over the 64 KiB slot: the slot is lost, far matches rerun on the full ring
    sync, se = zflush.flush_stream([t, t], 6, 8, -15, zflush.Z_SYNC_FLUSH)
    tail = zraw.raw_deflate(txt(5, 700), 6, 8)
    cases = {
        "dynamic": zflush.flushed_deflate(t, 6, 8) + tail,
        "fixed": zflush.flushed_deflate(b"abcabcabc", 6, 8) + tail,
        "stored": zflush.flushed_deflate(rnd(6, 900), 6, 8) + tail,
        "level0": zflush.flushed_deflate(t, 0, 8) + tail,
        "first": b"\x00" + M + tail,                                              # a marker as the very first block
        "payload": zflush.flushed_deflate(rnd(7, 500) + M, 0, 8) + tail,         # a stored payload that ends in the pattern
        "payload-final": zraw.raw_deflate(rnd(7, 500) + M, 0, 8),
        "final-empty": b"\x01" + M + tail,                                        # a final empty stored block
        "no-flush": tail,
        "cut1": zflush.flushed_deflate(t, 6, 8)[:-1],
        "cut3": zflush.flushed_deflate(t, 6, 8)[:-3],
        "cut4": zflush.flushed_deflate(t, 6, 8)[:-4],
        "bad-nlen": zflush.flushed_deflate(t, 6, 8)[:-1] + b"\xfe",
        "sync-history": sync[se[0]:],                                             # matches reach before the start
        "retry": zflush.flushed_deflate(big, 6, 8) + tail,
    }
    names = list(cases)
    buf, ranges = b"", []
    for k in names:
        ranges.append((len(buf), len(cases[k])))
        buf += cases[k] + b"\x55" * 7
    got = plain.inflate_segments(buf, ranges)
    for k, (st, consumed, produced, am) in zip(names, got):
        wst, wcons, wout, wam = zflush.seg_inflate(cases[k])
        assert (st, am) == (wst, wam), k
        if wst == zflush.END:
            assert (consumed, produced) == (wcons, len(wout)), k
    by = dict(zip(names, got))
    assert by["dynamic"][1:] == (len(cases["dynamic"]) - len(tail), 5000, True)
    assert by["first"] == (0, 5, 0, True) and by["final-empty"] == (0, 5, 0, False)
    assert by["payload"][2:] == (504, True) and by["payload-final"][2:] == (504, False)
    assert by["cut1"][0] == by["cut4"][0] == 2 and by["bad-nlen"][0] == 1 and by["sync-history"][0] == 1
    assert by["retry"][2:] == (200000, True)


# ---- 3. the exact deflate's flush end ------------------------------------------------------------------
def deflate_inputs(level):
    r = rnd(9, 126)
    ins = [rnd(10, 1), rnd(11, 2), rnd(12, 3), rnd(1, 127), rnd(2, 254), rnd(3, 255), r + r[1:4], txt(13, 300),
           txt(14, 5000), rnd(4, 16383), rnd(5, 32767), txt(15, 70000)]
    if level == 0:
        ins += [txt(7, 65535), txt(8, 65536)]
    return ins


@pytest.mark.parametrize("level", range(10))
def test_flush_deflate_equals_zlib(plain, level):
    ins = deflate_inputs(level)
    buf, items, want, at = b"".join(ins), [], [], 0
    for d in ins:
        for m in (1, 8, 9):
            items.append((at, len(d), level, 15, m, 0, True, None, True))
            want.append(zflush.flushed_deflate(d, level, m))
        at += len(d)
    items.append((at - 70000 if level else at - 70000 - 65535 - 65536, 70000, level, 9, 8, 0, True, None, True))
    want.append(zflush.flushed_deflate(txt(15, 70000), level, 8, 9))
    got = plain.deflate_batch(buf, items)
    for it, g, w in zip(items, got, want):
        assert g == w, (it[1:5], len(g), len(w))


def test_flush_deflate_argument_errors(plain):
    import antiz_amd
    p = txt(16, 2000)
    # (offset, length, level, window, memLevel, strategy, raw, deflater, flush)
    for item in ((0, 2000, 6, 15, 8, 0, False, None, True), (0, 2000, 6, 15, 8, 0, True, "gnu", True),
                 (0, 2000, 6, 15, 8, 1, True, None, True), (0, 2000, 6, 15, 8, 3, True, None, True),
                 (0, 2000, 6, 8, 8, 0, True, None, True), (0, 2000, 6, 15, 0, 0, True, None, True),
                 (0, 2000, 10, 15, 8, 0, True, None, True)):
        with pytest.raises(antiz_amd.AtzError) as e:
            plain.deflate_batch(p, [item])
        assert e.value.code == -1, item
    assert plain.deflate(p, 6, 15, 8, raw=True, flush=True) == zflush.flushed_deflate(p, 6, 8)


MW = r"""
import hashlib, random, sys
sys.path.insert(0, %r)
import antiz_amd
data = open(sys.argv[1], "rb").read()
items = [(0, n, lv, 15, m, 0, True, None, True) for n in (127, 129, 5000, len(data)) for lv in (1, 6) for m in (1, 2, 4, 9)]
with antiz_amd.Context(device=0) as c:
    outs = c.deflate_batch(data, items)
print(hashlib.sha256(b"".join(outs)).hexdigest())
""" % ROOT


def test_flush_deflate_on_multi_wave_trials(tmp_path):
    r = rnd(9, 126)
    data = r + r[1:4] + txt(17, 30000)   # 127 literals (level 1) and 126 + a match (level 6): the absent last block
    path = str(tmp_path / "mw.bin")
    with open(path, "wb") as f:
        f.write(data)
    want = b"".join(zflush.flushed_deflate(data[:n], lv, m) for n in (127, 129, 5000, len(data)) for lv in (1, 6)
                    for m in (1, 2, 4, 9))
    for mw in ("9", "0"):
        run = subprocess.run([sys.executable, "-c", MW, path], env=dict(os.environ, ATZ_MW=mw), capture_output=True,
                             text=True, timeout=240)
        assert run.returncode == 0, run.stderr[-2000:]
        assert run.stdout.strip().splitlines()[-1] == hashlib.sha256(want).hexdigest(), mw


# ---- 4. end to end -------------------------------------------------------------------------------------
def build_file():
    """A gzip member of 3 segments at level 6, a ZIP entry of 2 at level 9 and a zlib-wrapped stream of 2 at window
    15 and level 1, filler between -> (file, [(segment offset, body, payload, level, flush-terminated)])"""
    parts, segs = [], []

    def put(pre, stream, ends, datas, level, body_at):
        at = sum(len(p) for p in parts) + len(pre) + body_at
        lo = 0
        for i, (e, d) in enumerate(zip(ends, datas)):
            segs.append((at + lo, stream[lo:e], d, level, i < len(datas) - 1))
            lo = e
        parts.append(pre)

    g = [txt(21, 300), txt(22, 5000), txt(23, 70000)]
    gs, ge = zflush.flush_stream(g, 6, 8, -15)
    put(filler(24, 333), gs, ge, g, 6, 10)
    parts.append(zraw.gzip_member(gs, b"".join(g)))
    z = [txt(25, 2000), txt(26, 3000)]
    zs, ze = zflush.flush_stream(z, 9, 8, -15)
    put(filler(27, 200), zs, ze, z, 9, 30 + 5)
    parts.append(zraw.zip_entry(zs, 5000, name=b"a.txt", flags=zraw.ZIP_HINT_BITS[zraw.HINT_MAX]))
    w = [txt(28, 1500), txt(29, 2500)]
    ws, we = zflush.flush_stream(w, 1, 8, 15)
    put(filler(30, 150), ws[2:-4], [e - 2 for e in we[:-1]] + [len(ws) - 6], w, 1, 2)
    parts.append(ws)
    parts.append(filler(31, 99))
    return b"".join(parts), segs


def swept(c, data):
    recs = c.scan(data)
    res, diffs = c.sweep()
    return recs, {r[0]: (r, q) for r, q in zip(recs, res)}


@pytest.fixture(scope="module")
def e2e():
    import antiz_amd
    data, segs = build_file()
    out = dict(data=data, segs=segs)
    with antiz_amd.Context(device=0, containers=BOTH, segments=FLUSH) as c:
        out["on"], out["st_on"] = c.precompress(data)
        out["recs_on"], out["res_on"] = swept(c, data)
    with antiz_amd.Context(device=0, containers=BOTH, segments=()) as c:
        out["off"], _ = c.precompress(data)
        out["recs_off"], out["res_off"] = swept(c, data)
    return out


def test_scan_equals_the_model(e2e):
    data = e2e["data"]
    assert len(e2e["recs_off"]) == 3
    want = zflush.split(data, e2e["recs_off"])
    assert e2e["recs_on"] == want and len(want) == 7
    assert [(r[0], r[2], r[3], bool(r[4] & 128)) for r in want] == \
        [(at, len(body), len(d), fl) for at, body, d, _, fl in e2e["segs"]]
    assert [r[1] for r in want] == [24] * 3 + [26] * 2 + [25] * 2   # no hint, ZIP's max, FLEVEL 0 -> fast
    for r in e2e["recs_off"]:   # mask off: the streams are found whole and nothing records them
        assert e2e["res_off"][r[0]][1]["recomp"] == 0


def test_segments_are_recorded_exactly(e2e, plain):
    data, on = e2e["data"], e2e["on"]
    assert on[:4] == b"ATZ\6" and e2e["off"][:4] == b"ATZ\1"
    ver, origlen, descs = parse_atz(on)
    assert ver == 6 and origlen == len(data) and len(descs) == 7
    by = {d["off"]: d for d in descs}
    for at, body, payload, level, fl in e2e["segs"]:
        rec, res = e2e["res_on"][at]
        want = zflush.rule(body, payload, rec[1] - 24, fl)
        assert want is not None and want["diff_pos"] == []
        assert (res["recomp"], res["n_diff"], res["clevel"], res["memlevel"]) == (1, 0, 0x40 | want["level"], want["memlevel"])
        assert res["window"] == (0x8f if fl else 15), (at, fl)
        assert want["memlevel"] == 8 and (want["level"] == level or len(payload) < 4000)   # (small inputs: levels coincide)
        d = by[at]
        assert (d["cl"], d["il"], d["nd"], d["c"], d["w"], d["m"]) == (len(body), len(payload), 0, res["clevel"], res["window"], 8)
    assert plain.reconstruct(on) == data


def test_cli_round_trip(e2e, tmp_path):
    import antiz_amd
    f = str(tmp_path / "f")
    with open(f, "wb") as fh:
        fh.write(e2e["data"])
    env = dict(os.environ, ATZ_CONTAINERS="zip,gzip", ATZ_SEGMENTS="flush", ATZ_DEVICE="0")
    r = subprocess.run([antiz_amd.CLI_PATH, "-i", f], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    assert "OK! Restoration is bit by bit identical" in r.stdout
    assert open(f + ".atz", "rb").read() == e2e["on"]
    r = subprocess.run([antiz_amd.CLI_PATH, "-i", f], env=dict(env, ATZ_SEGMENTS="flush,sync"), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 1 and "ATZ_SEGMENTS: unknown segment kind sync" in r.stderr


def test_context_reads_the_environment(e2e, monkeypatch):
    import antiz_amd
    monkeypatch.setenv("ATZ_SEGMENTS", "flush")
    monkeypatch.setenv("ATZ_CONTAINERS", "zip,gzip")
    with antiz_amd.Context(device=0) as c:
        assert c.precompress(e2e["data"])[0] == e2e["on"]


def test_the_probe_finds_an_unanchored_chain():
    import antiz_amd
    segs = [txt(41, 5000), txt(42, 3000), txt(43, 4000)]
    stream, ends = zflush.flush_stream(segs, 6, 8, -15)
    assert (stream[0] >> 1) & 3 == 2
    pre = filler(44, 777)
    data = pre + stream + filler(45, 333)
    with antiz_amd.Context(device=0, probe=("deflate",)) as c:
        whole = c.scan(data)
    assert [(r[0], r[2], r[3]) for r in whole] == [(len(pre), len(stream), 12000)]
    with antiz_amd.Context(device=0, probe=("deflate",), segments=FLUSH) as c:
        recs = c.scan(data)
        assert recs == zflush.split(data, whole) and len(recs) == 3
        res, _ = c.sweep()
        assert all(q["recomp"] == 1 and q["n_diff"] == 0 for q in res)
        atz, _ = c.precompress(data)
        assert atz[:4] == b"ATZ\6" and c.reconstruct(atz) == data


def test_gnu_trials_on_the_last_segment_only():
    import antiz_amd
    e = [x for x in zgnu.fixtures()["entries"] if x["class"] == "b" and x["level"] == 6][0]
    tail = zlib.decompress(e["body"], -15)
    head = txt(46, 40000)
    first = zflush.flushed_deflate(head, 6, 9)   # memLevel 9: behind the memLevel-8 group, where GNU's nine would stand
    data = filler(47, 100) + zraw.gzip_member(first + e["body"], head + tail) + filler(48, 60)
    with antiz_amd.Context(device=0, containers=BOTH, segments=FLUSH, deflaters=("gnu",)) as c:
        recs, res = swept(c, data)
        assert [(r[2], r[3], r[4]) for r in recs] == [(len(first), 40000, 128), (len(e["body"]), len(tail), 0)]
        a, b = res[recs[0][0]][1], res[recs[1][0]][1]
        # 10 candidates at memLevel 8, then memLevel 9's first (level 6, no hint): no GNU candidate in between
        assert (a["recomp"], a["n_diff"], a["clevel"], a["window"], a["memlevel"], a["n_trials"]) == (1, 0, 0x46, 0x8f, 9, 11)
        assert (b["recomp"], b["n_diff"], b["clevel"], b["window"], b["memlevel"]) == (1, 0, 0x46, 15, 0)
        atz, _ = c.precompress(data)
        assert atz[:4] == b"ATZ\6" and c.reconstruct(atz) == data
    with antiz_amd.Context(device=0, containers=BOTH, segments=FLUSH) as c:   # without the deflater mask: the same 11
        recs, res = swept(c, data)
        assert res[recs[0][0]][1]["n_trials"] == 11 and res[recs[1][0]][1]["memlevel"] != 0


# ---- 5. nothing else moves -----------------------------------------------------------------------------
def test_mask_zero_is_no_mask(e2e):
    import antiz_amd
    assert "ATZ_SEGMENTS" not in os.environ
    with antiz_amd.Context(device=0, containers=BOTH) as c:
        unset, _ = c.precompress(e2e["data"])
        assert c.scan(e2e["data"]) == e2e["recs_off"]
    assert unset == e2e["off"]
    L = antiz_amd.lib()
    with antiz_amd.Context(device=0, containers=BOTH, segments=FLUSH) as c:   # set and cleared again
        antiz_amd._check(L.atz_set_segments(c.h, 0))
        assert c.precompress(e2e["data"])[0] == e2e["off"]


def test_files_without_a_chain_stay_as_they_are():
    import antiz_amd
    a, b = txt(51, 3000), txt(52, 4000)
    plain_streams = b"".join(filler(53 + i, 80) + zstrat.deflate(txt(60 + i, 2500), lv, 15, 8) for i, lv in enumerate((1, 6, 9)))
    assert zflush.markers(plain_streams) == []
    sync = zraw.gzip_member(zflush.flush_stream([a, a], 6, 8, -15, zflush.Z_SYNC_FLUSH)[0], a + a)
    w14 = zflush.flush_stream([a, b], 6, 8, 14)[0]
    doubled = zflush.flushed_deflate(a, 6, 8) + b"\x00" + M + zraw.raw_deflate(b, 6, 8)   # a zero-length segment
    for name, data in (("no marker", plain_streams), ("sync flush", filler(70, 50) + sync + filler(71, 50)),
                       ("window 14", filler(72, 50) + w14 + filler(73, 50)),
                       ("zero-length segment", filler(74, 50) + zraw.gzip_member(doubled, a + b) + filler(75, 50))):
        with antiz_amd.Context(device=0, containers=BOTH) as c:
            off, _ = c.precompress(data)
            recs_off = c.scan(data)
        with antiz_amd.Context(device=0, containers=BOTH, segments=FLUSH) as c:
            on, _ = c.precompress(data)
            recs_on = c.scan(data)
        assert recs_off and recs_on == recs_off == zflush.split(data, recs_off), name
        assert on == off, name


# ---- 6. near misses ------------------------------------------------------------------------------------
def padded(seg, ks):
    """a level-6 memLevel-1 segment of random bytes is all stored blocks: the five padding bits of the k-th block's
    header byte are set for k in ks (the decode ignores them; a trial writes zeros) -> (segment, positions)"""
    out, pos, at, k = bytearray(seg), [], 0, 0
    while at < len(seg) - 5:
        n = seg[at + 1] | (seg[at + 2] << 8)
        assert seg[at] & 7 == 0 and n ^ 0xffff == seg[at + 3] | (seg[at + 4] << 8)
        if k in ks:
            out[at] |= 0xf8
            pos.append(at)
        at += 5 + n
        k += 1
    assert at == len(seg) - 5 or at == len(seg)
    return bytes(out), pos


def test_near_misses_follow_the_rule():
    """A marker byte that is changed leaves no decodable parent (LEN and NLEN no longer agree), so the record that
    'stays whole' there is none at all: the scan under the mask must equal the scan without it.  The chain that
    breaks under a parent that still decodes is the zero-length segment of test_files_without_a_chain_stay_as_they_are."""
    import antiz_amd
    r1, r2, t3 = rnd(81, 2000), rnd(82, 40000), txt(83, 3000)
    s1, p1 = padded(zflush.flushed_deflate(r1, 6, 1), {7})                    # one byte, deep inside
    s2, p2 = padded(zflush.flushed_deflate(r2, 6, 1), set(range(20, 160)))   # 140 bytes: past recomp_tresh
    s3 = zraw.raw_deflate(t3, 6, 1)
    assert len(p1) == 1 and len(p2) == 140
    pre = filler(84, 64)
    data = pre + zraw.gzip_member(s1 + s2 + s3, r1 + r2 + t3) + filler(85, 64)
    at1 = len(pre) + 10
    with antiz_amd.Context(device=0, containers=BOTH, segments=FLUSH) as c:
        recs = c.scan(data)
        assert [(r[0], r[2], r[3], r[4]) for r in recs] == [(at1, len(s1), 2000, 128), (at1 + len(s1), len(s2), 40000, 128),
                                                           (at1 + len(s1) + len(s2), len(s3), 3000, 0)]
        res, (doff, dval) = c.sweep()
        want = [zflush.rule(s, p, 0, fl) for s, p, fl in ((s1, r1, True), (s2, r2, True), (s3, t3, False))]
        assert want[0]["diff_pos"] == p1 and want[1] is None and want[2]["diff_pos"] == []
        assert (res[0]["recomp"], res[0]["n_diff"], res[0]["first_diff"], res[0]["window"]) == (1, 1, p1[0], 0x8f)
        assert dval[res[0]["diff_index"]] == s1[p1[0]] == 0xf8
        assert res[1]["recomp"] == 0
        assert (res[2]["recomp"], res[2]["n_diff"], res[2]["memlevel"]) == (1, 0, 1)
        atz, st = c.precompress(data)
        assert atz[:4] == b"ATZ\6" and st["n_recomp"] == 2 and c.reconstruct(atz) == data
    bad = bytearray(data)
    bad[at1 + len(s1) - 1] = 0xfe    # the first marker's last byte
    bad = bytes(bad)
    with antiz_amd.Context(device=0, containers=BOTH) as c:
        off = c.scan(bad)
        atz_off, _ = c.precompress(bad)
    with antiz_amd.Context(device=0, containers=BOTH, segments=FLUSH) as c:
        assert c.scan(bad) == off == zflush.split(bad, off)
        assert c.precompress(bad)[0] == atz_off


# ---- 7. the reader -------------------------------------------------------------------------------------
def test_reader_checks_flush_descriptors(e2e, plain):
    import antiz_amd
    on = e2e["on"]
    _, _, descs = parse_atz(on)
    at, first = 28, None
    for d in descs:
        if d["w"] == 0x8f and first is None:
            first = at
        at += len(d["raw"])
    assert first is not None
    for magic in (b"ATZ\5", b"ATZ\4", b"ATZ\3", b"ATZ\1", b"ATZ\7"):   # window 0x8F under another magic
        with pytest.raises(antiz_amd.AtzError):
            plain.reconstruct(magic + on[4:])

    def mutated(off, val):
        b = bytearray(on)
        b[first + off] = val
        return bytes(b)

    c0 = on[first + 24]
    assert c0 == 0x46
    for off, val in ((24, c0 & 0x3f), (24, c0 | 0x10), (24, c0 | 0x30), (24, c0 | 0x80), (24, 0x4a), (25, 0x8e), (25, 0x89),
                     (25, 0xcf), (26, 0), (26, 10)):
        with pytest.raises(antiz_amd.AtzError):   # not raw, a strategy, stitched, level 10, other windows, memLevel 0 / 10
            plain.reconstruct(mutated(off, val))
    for cut in (1, 5, len(on) // 2, len(on) - 30):
        with pytest.raises(antiz_amd.AtzError):
            plain.reconstruct(on[:-cut])
    assert plain.reconstruct(mutated(25, 15)) != e2e["data"]   # read as a finished body: other bytes, no error
    assert plain.reconstruct(on) == e2e["data"]


# ---- 8. limits -----------------------------------------------------------------------------------------
def test_limits():
    import antiz_amd
    L = antiz_amd.lib()
    with antiz_amd.Context(device=0, segments=FLUSH) as c:
        for bad in (2, 3, 1 << 31):
            with pytest.raises(antiz_amd.AtzError) as e:
                antiz_amd._check(L.atz_set_segments(c.h, bad))
            assert e.value.code == -1
        data = txt(1, 4096) + zstrat.deflate(txt(2, 3000), 6, 15, 8, 0)
        with dev_copy(data) as d:
            with pytest.raises(antiz_amd.AtzError) as e:
                c.shard_scan(d, data, 0, 1)
            assert e.value.code == -1
            with pytest.raises(antiz_amd.AtzError) as e:
                c.shard_sweep(d, data, [b""])
            assert e.value.code == -1
        antiz_amd._check(L.atz_set_segments(c.h, 0))
        with dev_copy(data) as d:
            assert c.shard_scan(d, data, 0, 1)
    with pytest.raises(ValueError):
        antiz_amd.Context(device=0, segments=("sync",))


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


def test_a_small_cap_keeps_the_bytes(e2e, tmp_path):
    path = str(tmp_path / "f.bin")
    with open(path, "wb") as f:
        f.write(e2e["data"])
    r = subprocess.run([sys.executable, "-c", CAPS, path], env=dict(os.environ, ATZ_CAP_DIV="4096", ATZ_SEGMENTS="flush"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2] == "1" and lines[-1] == hashlib.sha256(e2e["on"]).hexdigest()
