"""The stitch extension on the GPU: the IDAT anchor pass against the Python model, the scan's
stitched records and their pieces against the model, the walk of a stitched stream against the walk of the same
stream in one chunk (the flat twin, whose expected results are the oracle's), the ATZ4 file end to end, the caps,
the ATZ4 reader, the CLI and the shard refusal.

The PNG files are built by hand (zpng.png: every chunk length is stated); expected deflate bytes come from
oracle/_ref/libz128.so (zstrat).  Without the library these tests fail, they do not skip.
"""
import ctypes as C
import functools
import hashlib
import os
import random
import struct
import subprocess
import sys
import zlib

import pytest

import _libs
import nearmiss
import zpng
import zraw
import zstrat
from test_gpu_strategy import dev_copy, gradient, hip, txt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PNG = ("png",)
STRATS = ("filtered", "rle", "huffman")
STRAT_MASK = 14
STITCHED = 64   # atz_cand_t.flags bit 6


@pytest.fixture(scope="module")
def ctx():
    import antiz_amd
    with antiz_amd.Context(device=0, stitch=PNG) as c:
        yield c


# ---- 1. anchors ------------------------------------------------------------------------------------
SEG = 53248   # the anchor kernel's block segment for the file below (4 blocks)


def field(length):
    return struct.pack(">I", length) + b"IDAT"


def anchor_file(shift):
    """192 KiB + 77 with length + type fields whose 'I' stands at 4095, 4096 or 4097 (by `shift`: the fields
    would overlap in one file), around a lane's 16-byte load, a wave's 1 KiB and the block segment (the length
    in the block before the 'I', the type cut by the boundary), a 4 KiB stretch of fields, and the ones the rule
    refuses: the top bit of the length set, a CRC that ends one byte past the file, a type below offset 4."""
    n = 3 * 65536 + 77
    r = random.Random(shift)
    b = bytearray(x if x != 0x49 else 0x4a for x in r.randbytes(n))
    want = []

    def put(a, length, ok=True):
        b[a - 4:a + 4] = field(length)
        if ok:
            want.append(a)

    for a in (4095, 16 * 40 + 13, 16 * 50 + 14, 16 * 60 + 15, 1024 * 2 - 1, 1024 * 3, 1024 * 5 + 1, 4096 * 3 - 1,
              SEG - 1, 2 * SEG + 1, 3 * SEG - 3, 4096 * 20 + 2):
        put(a + shift, 7 + 3 * shift)
    put(2 * SEG - 4096 + shift, n - (2 * SEG - 4096 + shift) - 8)        # the CRC ends with the file
    put(2 * SEG - 8192 + shift, n - (2 * SEG - 8192 + shift) - 7, False)   # ... one byte past it
    put(3 * SEG + 4096 + shift, 0x80000000 + shift, False)               # the top bit of the length
    put(3 * SEG + 8192 + shift, 0x7fffffff, False)
    put(3 * SEG + 12288 + shift, 0)
    b[shift:shift + 4] = b"IDAT"                                          # a < 4
    for k in range(512):                                                  # a step with 512 hits in all four waves
        put(4096 * 30 + 8 * k + 4, k)
    for k, bad in enumerate((b"IDAU", b"JDAT", b"IdAT", b"IDA")):         # near-misses
        at = 4096 * 44 + 64 * k
        b[at - 4:at + 4] = struct.pack(">I", 5) + (bad + b"\0")[:4]
    put(n - 8, 0)                                                         # the last position that counts
    b[n - 4:n] = b"IDAT"
    return bytes(b), sorted(want)


@pytest.mark.parametrize("shift", [0, 1, 2])
def test_anchors_match_the_model(ctx, shift):
    data, want = anchor_file(shift)
    n = len(data)
    model = zpng.anchors(data)
    # the file is what it claims to be
    assert model == want and len(want) > 520
    assert 4095 + shift in want and {SEG - 1 + shift, 2 * SEG + 1 + shift, 3 * SEG - 3 + shift} <= set(want)
    assert n - 8 in want and n - 4 not in want and shift not in want
    assert data.count(b"IDAT") == len(want) + 5
    assert (n + 65535) // 65536 == 4 and (((n + 3) // 4 + 4095) & ~4095) == SEG
    got = ctx.stitch_anchors(data)
    assert got == [(a, 2) for a in want]
    assert ctx.stitch_anchors(data, 0) == []
    # the container pass does not see them, and keeps refusing the internal bit
    import antiz_amd
    assert ctx.container_anchors(data, 3) == zraw.anchors(data, 3)
    with pytest.raises(antiz_amd.AtzError):
        ctx.container_anchors(data, 4)


def test_anchors_in_tiny_files(ctx):
    whole = field(0) + bytes(4)          # 12 bytes: the smallest file with an anchor
    for k in range(13):
        assert ctx.stitch_anchors(whole[:k]) == [(a, 2) for a in zpng.anchors(whole[:k])], k
    assert ctx.stitch_anchors(whole) == [(4, 2)] and ctx.stitch_anchors(whole[:11]) == []
    for data in (field(1) + bytes(4), field(1) + bytes(5), b"IDAT" + field(0) + bytes(4), b"IDAT" + bytes(8),
                 b"\0" + whole, field(0x80000000) + bytes(4)):
        assert ctx.stitch_anchors(data) == [(a, 2) for a in zpng.anchors(data)], data
    assert ctx.stitch_anchors(field(1) + bytes(5)) == [(4, 2)] and ctx.stitch_anchors(field(1) + bytes(4)) == []


# ---- 2. the scan against the model ---------------------------------------------------------------------
def sized_stream(size, level=6):
    """A zlib stream of exactly `size` bytes."""
    for n in range(size, 4 * size):
        s = zstrat.deflate(txt(77, n), level, 15, 8, 0)
        if len(s) == size:
            return s
    raise AssertionError(size)


def wrap(parts):
    """Text, then each part behind 200 bytes of text."""
    out = [txt(1, 300)]
    for k, p in enumerate(parts):
        out += [p, txt(50 + k, 200)]
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> file: one chain each (zpng.png states every chunk length)."""
    out = {}
    s = {lv: zstrat.deflate(txt(10 + lv, 9000), lv, 15, 8, 0) for lv in (1, 6, 9)}
    n6 = len(s[6])
    out["head_split"] = wrap([zpng.png(s[6], [1, n6 - 1])[0]])
    out["trailer_1_3"] = wrap([zpng.png(s[1], [len(s[1]) - 3, 3])[0]])
    out["trailer_2_2"] = wrap([zpng.png(s[6], [n6 - 2, 2])[0]])
    out["trailer_3_1"] = wrap([zpng.png(s[9], [len(s[9]) - 1, 1])[0]])
    out["zero_middle"] = wrap([zpng.png(s[6], [1000, 0, n6 - 1000])[0]])
    out["zero_lead"] = wrap([zpng.png(s[9], [0, 700, len(s[9]) - 700])[0]])
    out["early_end"] = wrap([zpng.png(s[1] + bytes(range(57)), [900, len(s[1]) - 900 + 57])[0]])
    out["ones"] = wrap([zpng.png(sized_stream(300), [1] * 300)[0]])
    ring = zstrat.deflate(txt(20, 120000), 6, 15, 8, 0)
    assert 60000 < len(ring) < 80000
    out["ring"] = wrap([zpng.png(ring, zpng.split(len(ring), 8192))[0]])
    big = zstrat.deflate(txt(21, 80000), 1, 15, 8, 0)
    out["past_64k"] = wrap([zpng.png(big, zpng.split(len(big), 4096))[0]])
    out["first_chunk_end"] = wrap([zpng.png(s[6] + bytes(25), [n6 + 5, 20])[0]])
    # a stored stream whose payload holds a whole zlib stream inside the second chunk: the reference records
    # that one, and the chain's hull meets it
    inner = zstrat.deflate(txt(22, 700), 6, 15, 8, 0)
    outer = zstrat.deflate(txt(23, 2000) + inner + txt(24, 2000), 0, 15, 8, 0)
    out["hull_meets"] = wrap([zpng.png(outer, [1000, len(outer) - 1000])[0]])
    return out


CASE_NAMES = ["head_split", "trailer_1_3", "trailer_2_2", "trailer_3_1", "zero_middle", "zero_lead", "early_end", "ones",
              "ring", "past_64k", "first_chunk_end", "hull_meets"]
DROPPED = {"hull_meets": 1}           # accepted candidates the hull rule drops
NOT_STITCHED = ("first_chunk_end", "hull_meets")


@functools.lru_cache(maxsize=None)
def reference(data, **opts):
    rc, atz, stats = _libs.ora_precompress(data, **opts)
    assert rc == 0
    return atz, stats["streams"]


def expected_scan(data):
    """-> (the merged record list [(offset, type, comp_len, infl_len, stitched)], stitched model records, dropped):
    the reference's records are the oracle's scan of the same bytes."""
    ref = [(s["offset"], s["type"], s["comp_len"], s["infl_len"], False) for s in reference(data)[1]]
    kept, dropped = zpng.stitched_records(data, [(o, cl) for o, _, cl, _, _ in ref])
    merged = sorted(ref + [(x["offset"], x["type"], x["comp_len"], x["infl_len"], True) for x in kept])
    return merged, kept, dropped


def check_scan(c, data):
    """scan `data` on context c (left ready for its sweep) against the model; -> (records, stitched model records)"""
    merged, kept, dropped = expected_scan(data)
    got = c.scan(data)
    assert [(o, t, cl, il, bool(f & STITCHED)) for o, t, cl, il, f in got] == merged
    by = {x["offset"]: x for x in kept}
    for k, (o, _, _, _, f) in enumerate(got):
        assert c.stitch_pieces(k) == (by[o]["pieces"] if f & STITCHED else [])
    return got, kept


def test_premises_of_the_cases():
    """On the CPU: the reference records none of the stitched heads, and no stitched candidate is dropped but the
    one built for it."""
    assert list(cases()) == CASE_NAMES
    for name, data in cases().items():
        merged, kept, dropped = expected_scan(data)
        (ch, _), = zpng.candidates(data)
        head = next(o for o, n in ch if n)
        ref_offsets = {o for o, _, _, _, st in merged if not st}
        assert len(dropped) == DROPPED.get(name, 0), name
        assert len(kept) == (0 if name in NOT_STITCHED else 1), name
        assert (head in ref_offsets) == (name == "first_chunk_end"), name
        if kept:
            lo, hi = kept[0]["offset"], kept[0]["offset"] + zpng.hull(kept[0]["pieces"])
            assert not any(lo <= o < hi for o in ref_offsets), name
            assert kept[0]["comp_len"] > kept[0]["pieces"][0][1]
    c = cases()
    assert len(expected_scan(c["ones"])[1][0]["pieces"]) == 300
    assert expected_scan(c["early_end"])[1][0]["pieces"][-1][1] == zpng.chains(c["early_end"])[0][-1][1] - 57
    assert expected_scan(c["past_64k"])[1][0]["infl_len"] > 65536
    assert [n for _, n in expected_scan(c["zero_middle"])[1][0]["pieces"]][1] == 0
    assert expected_scan(c["zero_lead"])[1][0]["pieces"][0][1] == 700


@pytest.mark.parametrize("name", CASE_NAMES)
def test_scan_matches_the_model(ctx, name):
    data = cases()[name]
    got, kept = check_scan(ctx, data)
    assert len(kept) == (0 if name in NOT_STITCHED else 1)
    # the same file on a context without the mask: the reference's records alone
    import antiz_amd
    with antiz_amd.Context(device=0) as c:
        assert [r[:4] for r in c.scan(data)] == [(s["offset"], s["type"], s["comp_len"], s["infl_len"])
                                                 for s in reference(data)[1]]


# ---- 3. the flat twin ----------------------------------------------------------------------------------
def check_twin(c, data, opts):
    """Every stitched record of `data` walks as the same stream in one chunk does: the oracle's result on the twin."""
    got, kept = check_scan(c, data)
    res, diffs = c.sweep()
    lists = _libs.diff_lists(res, diffs)
    twin, where = zpng.flat_twin(data)
    ora = {s["offset"]: s for s in reference(twin, **opts)[1]}
    n = 0
    for k, (o, _, cl, il, f) in enumerate(got):
        if not f & STITCHED:
            continue
        s, r, (pos, val) = ora[where[o]], res[k], lists[k]
        assert (s["comp_len"], s["infl_len"]) == (cl, il)
        assert (r["clevel"], r["window"], r["memlevel"], r["ident"], r["recomp"], r["n_trials"], r["n_diff"], pos, bytes(val)) == \
               (s["clevel"], s["window"], s["memlevel"], s["ident"], s["recomp"], s["n_trials"], s["n_diff"], s["diff_pos"],
                s["diff_val"]), (o, opts)
        if s["n_diff"]:
            assert r["first_diff"] == s["first_diff"]
        n += 1
    assert n == len(kept)
    return n, [res[k] for k, g in enumerate(got) if g[4] & STITCHED], kept


ORA_OPTS = {"recomp_tresh": "recomp", "sizediff_tresh": "sizediff", "shortcut_len": "shortcut", "mismatch_tol": "tol"}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_flat_twin_default_streams(ctx, name):
    n, res, _ = check_twin(ctx, cases()[name], {})
    assert n == (0 if name in NOT_STITCHED else 1)
    assert all(r["recomp"] == 1 and r["n_diff"] == 0 for r in res)   # levels 1, 6 and 9 at memLevel 8: exact


@functools.lru_cache(maxsize=None)
def nearmiss_file():
    """Near-miss streams (nearmiss.storedpad: k stored-block header bytes altered; nearmiss.tailflush: the original
    outlasts every trial) cut so that an altered byte is the last byte of a piece and the next altered byte the
    first byte of a piece."""
    r = random.Random(41)
    parts = []
    for k in (3, 5, 140):
        s, _, _, pads = nearmiss.storedpad(r, k)
        a, b = pads[0], pads[1]
        lens = [a + 1, b - a - 1, len(s) - b]          # pads[0] ends piece 0, pads[1] starts piece 2
        assert min(lens) > 0 and zlib.decompress(s)
        parts.append(zpng.png(s, lens)[0])
    s, _, _, _ = nearmiss.tailflush(r, "sync")
    parts.append(zpng.png(s, [len(s) - 6, 3, 3])[0])   # the flush marker's and the trailer's bytes in small pieces
    s, _, _, pads = nearmiss.eobpad(r, False)
    parts.append(zpng.png(s, [pads[0], 1, len(s) - pads[0] - 1])[0])   # the altered byte a piece of its own
    return wrap(parts)


@pytest.mark.parametrize("opts", [dict(), dict(mismatch_tol=0, recomp_tresh=4)],
                         ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "defaults")
def test_flat_twin_near_misses(opts):
    import antiz_amd
    with antiz_amd.Context(device=0, stitch=PNG, **opts) as c:
        n, res, _ = check_twin(c, nearmiss_file(), {ORA_OPTS[k]: v for k, v in opts.items()})
    assert n == 5
    recorded = [r for r in res if r["recomp"]]
    assert any(r["n_diff"] for r in recorded) and len(recorded) < 5   # 140 altered bytes are never recorded


@functools.lru_cache(maxsize=None)
def filtered_file():
    """Z_FILTERED streams of scanline data at levels 6 and 9 (what a PNG writer makes), in 2 KiB IDAT chunks."""
    parts, streams = [], []
    for k, (lv, m, size) in enumerate([(6, 8, 9000), (9, 8, 12000), (6, 9, 5000), (9, 7, 7000)]):
        p = gradient(300 + k, size)
        s = zstrat.deflate(p, lv, 15, m, zstrat.Z_FILTERED)
        parts.append(zpng.png(s, zpng.split(len(s), 2048))[0])
        streams.append((s, p))
    return wrap(parts), streams


def test_flat_twin_filtered_streams_with_strategies():
    import antiz_amd
    data, streams = filtered_file()
    twin, where = zpng.flat_twin(data)
    with antiz_amd.Context(device=0, stitch=PNG, strategies=STRATS) as c:
        got, kept = check_scan(c, data)
        res, diffs = c.sweep()
        flat = c.scan(twin)
        fres, fdiffs = c.sweep()
    lists, flists = _libs.diff_lists(res, diffs), _libs.diff_lists(fres, fdiffs)
    fby = {g[0]: k for k, g in enumerate(flat)}
    keys = ("clevel", "window", "memlevel", "ident", "recomp", "first_diff", "n_diff")
    st = [k for k, g in enumerate(got) if g[4] & STITCHED]
    assert len(st) == len(kept) == len(streams)
    for k, (s, p) in zip(st, streams):
        assert (got[k][2], got[k][3]) == (len(s), len(p))
        j = fby[where[got[k][0]]]
        assert not flat[j][4] & STITCHED
        assert [res[k][x] for x in keys] == [fres[j][x] for x in keys] and lists[k] == flists[j]
        want = zstrat.rule(s, p, STRAT_MASK)   # the reference walk records none of them; the strategy walk's model
        assert want is not None and want["diff_pos"] == []
        assert (res[k]["recomp"], res[k]["clevel"], res[k]["window"], res[k]["memlevel"], res[k]["ident"], res[k]["n_diff"]) == \
               (1, antiz_amd.pack_clevel(want["strategy"], want["level"]), want["window"], want["memlevel"], want["ident"], 0)
    # without the strategy mask the reference walk leaves them unrecorded, as it leaves their twins (the oracle)
    with antiz_amd.Context(device=0, stitch=PNG) as c:
        n, res, _ = check_twin(c, data, {})
    assert n == len(streams) and not any(r["recomp"] for r in res)


# ---- 4. end to end -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e2e_file():
    """Text, a stitched PNG, a ZIP entry, a single-chunk PNG, a stitched PNG with trailing junk in its last chunk, a
    plain zlib stream (and a stitched one that outgrows its 64 KiB arena slot)."""
    a = zstrat.deflate(txt(31, 20000), 6, 15, 8, 0)
    body = zraw.raw_deflate(txt(32, 6000), 6, 8)
    b = zstrat.deflate(txt(33, 5000), 9, 15, 8, 0)
    c = zstrat.deflate(txt(34, 12000), 1, 15, 8, 0)
    d = zstrat.deflate(txt(35, 4000), 6, 15, 8, 0)
    e = zstrat.deflate(txt(36, 100000), 6, 15, 9, 0)
    return wrap([zpng.png(a, zpng.split(len(a), 1000))[0], zraw.zip_entry(body, 6000, name=b"a.txt"), zpng.png(b, [len(b)])[0],
                 zpng.png(c + bytes(range(40)), zpng.split(len(c), 4096)[:-1] + [len(c) % 4096 + 40])[0], d,
                 zpng.png(e, zpng.split(len(e), 8192))[0]])


def model_atz4(data, plain_descs, stitched):
    """The ATZ4 file: plain_descs = raw descriptor bytes by offset (the reference's), stitched = [(record, clevel,
    window, memlevel)] (exact ones)."""
    descs = dict(plain_descs)
    ranges = []
    for rec, cl, w, m in stitched:
        descs[rec["offset"]] = zpng.descriptor(rec, cl, w, m)
        ranges += rec["pieces"]
    body = b"".join(descs[o] for o in sorted(descs))
    return descs, ranges, body


@pytest.fixture(scope="module")
def e2e():
    import antiz_amd
    data = e2e_file()
    out = dict(data=data)
    for name, kw in (("off", {}), ("on", dict(stitch=PNG)), ("zip", dict(containers=("zip",))),
                     ("both", dict(stitch=PNG, containers=("zip",)))):
        with antiz_amd.Context(device=0, **kw) as c:
            out[name], out["st_" + name] = c.precompress(data)
    return out


def test_end_to_end(e2e):
    import antiz_amd
    data = e2e["data"]
    ref_atz, ref_streams = reference(data)
    # stitch off: the parent's bytes, which are the reference's
    with antiz_amd.Context(device=0, stitch=()) as c:
        assert c.precompress(data)[0] == e2e["off"] == ref_atz and ref_atz[:4] == b"ATZ\1"
    _, kept, dropped = expected_scan(data)
    assert len(kept) == 3 and not dropped
    twin, where = zpng.flat_twin(data)
    ora = {s["offset"]: s for s in reference(twin)[1]}
    stitched = []
    for rec in kept:
        s = ora[where[rec["offset"]]]
        assert s["recomp"] == 1 and s["n_diff"] == 0
        stitched.append((rec, s["clevel"], s["window"], s["memlevel"]))
    ver, origlen, off_descs, off_res = zpng.parse_atz(e2e["off"])
    plain = {d["off"]: d["raw"] for d in off_descs}
    assert len(plain) == 2   # the single-chunk PNG's stream and the plain one
    descs, ranges, body = model_atz4(data, plain, stitched)
    ranges += [(d["off"], d["cl"]) for d in off_descs]
    res = zpng.residue(data, ranges)
    want = b"ATZ\4" + struct.pack("<QQQ", 28 + len(body) + len(res), len(data), len(descs)) + body + res
    assert e2e["on"] == want
    ver, origlen, on_descs, on_res = zpng.parse_atz(e2e["on"])
    assert ver == 4 and origlen == len(data) and on_res == res
    assert [d["pieces"] for d in on_descs if d["pieces"]] == [[n for _, n in rec["pieces"]] for rec in kept]
    # the trailing junk stays in the residue: the last piece ends where the stream does
    assert kept[1]["pieces"][-1][1] + 40 == zpng.chains(data)[2][-1][1]
    # the 100 000 B stream outgrew its arena slot: decoded with the 32 KiB ring from the stitch buffer, and
    # inflated again from it as a record
    assert e2e["st_on"]["n_inflate_retries"] >= 1 and e2e["st_on"]["n_reinflated"] >= 1
    assert e2e["st_on"]["n_streams"] == 5 and e2e["st_on"]["n_recomp"] == 5
    # with the container mask too: the ZIP body beside them
    ver, _, both, _ = zpng.parse_atz(e2e["both"])
    _, _, zdescs, _ = zpng.parse_atz(e2e["zip"])
    assert ver == 4 and e2e["zip"][:4] == b"ATZ\3" and len(both) == 6
    both_by = {d["off"]: d for d in both}
    for d in on_descs + zdescs:
        assert both_by[d["off"]]["raw"] == d["raw"], d["off"]
    assert sum(1 for d in both if d["c"] & 0x40) == 1 and sum(1 for d in both if d["c"] & 0x80) == 3
    with antiz_amd.Context(device=0) as c:
        for atz in (e2e["on"], e2e["both"], e2e["off"]):
            assert c.reconstruct(atz) == data
            with dev_copy(atz) as d:
                p, n = c.reconstruct_device(d, atz)
                out = C.create_string_buffer(n)
                assert hip().hipMemcpy(out, p, n, 2) == 0   # device to host
                assert out.raw == data


def test_no_recorded_stitched_stream_keeps_the_version():
    """Chains whose streams the walk does not reproduce: the file is what a context without the mask writes."""
    import antiz_amd
    data, _ = filtered_file()
    data += zstrat.deflate(txt(3, 3000), 6, 15, 8, 0)
    for kw, magic in ((dict(), b"ATZ\1"), (dict(containers=("zip",)), b"ATZ\1")):
        with antiz_amd.Context(device=0, **kw) as c:
            off, _ = c.precompress(data)
        with antiz_amd.Context(device=0, stitch=PNG, **kw) as c:
            on, st = c.precompress(data)
        assert on == off and on[:4] == magic and st["n_streams"] == 5 and st["n_recomp"] == 1
    # and with the strategy mask they are recorded
    with antiz_amd.Context(device=0, stitch=PNG, strategies=STRATS) as c:
        on, st = c.precompress(data)
        assert on[:4] == b"ATZ\4" and st["n_recomp"] == 5 and c.reconstruct(on) == data
    with antiz_amd.Context(device=0, strategies=STRATS) as c:
        assert c.precompress(data)[0][:4] == b"ATZ\1"


# ---- 5. caps -------------------------------------------------------------------------------------------
CAPS = r"""
import hashlib, sys
sys.path.insert(0, %r)
import antiz_amd
data = open(sys.argv[1], "rb").read()
with antiz_amd.Context(device=0, stitch=("png",)) as c:
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


# ---- 6. the ATZ4 reader --------------------------------------------------------------------------------
def test_atz4_reader_survives_mutations(e2e):
    import antiz_amd
    good = e2e["on"]
    origlen = struct.unpack_from("<Q", good, 12)[0]
    _, _, descs, _ = zpng.parse_atz(good)
    lists, at = [], 28   # where the piece lists are: a third of the bit flips go there
    for d in descs:
        if d["pieces"]:
            lists.append((at + len(d["raw"]) - 4 - 4 * len(d["pieces"]), at + len(d["raw"])))
        at += len(d["raw"])
    r = random.Random(2026)
    accepted = refused = 0
    with antiz_amd.Context(device=0) as c:
        for k in range(200):
            b = bytearray(good)
            if k % 4 == 3:
                b = b[:r.randrange(0, len(b))]
            else:
                where = r.randrange(*lists[k % len(lists)]) if k % 3 == 0 else r.randrange(28, 28 + 35) if k % 3 == 1 else \
                    r.randrange(0, len(b))
                b[where] ^= 1 << r.randrange(8)
            try:
                out = c.reconstruct(bytes(b))
            except antiz_amd.AtzError:
                refused += 1
                continue
            accepted += 1
            assert len(out) == origlen
        assert accepted > 0 and refused > 0, (accepted, refused)
        for magic in (b"ATZ\1", b"ATZ\2", b"ATZ\3"):   # bit 7 of a clevel byte is invalid there
            with pytest.raises(antiz_amd.AtzError):
                c.reconstruct(magic + good[4:])
        assert c.reconstruct(good) == e2e["data"]


def test_atz4_reader_refuses_bad_piece_lists():
    """Hand-written files around one stitched stream: each breaks one rule of the piece list."""
    import antiz_amd
    data = cases()["trailer_2_2"]
    _, (rec,), _ = expected_scan(data)
    n = rec["comp_len"]

    def atz(recs, origlen=len(data), clevel=6):
        body = b"".join(zpng.descriptor(x, clevel, 15, 8)[:24] + bytes([x.get("c", 0x80 | clevel)]) +
                        zpng.descriptor(x, clevel, 15, 8)[25:] for x in recs)
        res = zpng.residue(data, [p for x in recs for p in x["pieces"]])
        return b"ATZ\4" + struct.pack("<QQQ", 28 + len(body) + len(res), origlen, len(recs)) + body + res

    o = rec["offset"]
    one = dict(rec, pieces=[(o, n)])
    short = dict(rec, pieces=[(o, n - 3), (o + n + 9, 2)])
    empty_first = dict(rec, pieces=[(o, 0), (o + 12, n)])
    empty_last = dict(rec, pieces=[(o, n), (o + n + 12, 0)])
    late = dict(rec, offset=len(data) - n - 11)   # the hull ends one byte past the original
    second = dict(rec, offset=o + n + 5, pieces=rec["pieces"])   # starts inside the first one's hull
    both_bits = dict(rec, c=0xc6)
    with antiz_amd.Context(device=0) as c:
        assert c.reconstruct(atz([rec])) == data
        for name, bad in (("k = 1", atz([one])), ("sum != comp_len", atz([short])), ("empty first piece", atz([empty_first])),
                          ("empty last piece", atz([empty_last])), ("hull past origlen", atz([late])),
                          ("hull past a smaller origlen", atz([rec], origlen=o + n + 11)),
                          ("next offset inside the hull", atz([rec, second])), ("bits 6 and 7", atz([both_bits]))):
            with pytest.raises(antiz_amd.AtzError):
                c.reconstruct(bad)
                pytest.fail("accepted: " + name)
        # (the hull's last byte may be the original's last: the same record, the original cut there)
        cut = o + zpng.hull(rec["pieces"])
        res = zpng.residue(data[:cut], rec["pieces"])
        body = zpng.descriptor(rec, 6, 15, 8)
        assert c.reconstruct(b"ATZ\4" + struct.pack("<QQQ", 28 + len(body) + len(res), cut, 1) + body + res) == data[:cut]


# ---- 7. CLI and the switch -----------------------------------------------------------------------------
def test_cli_stitch(e2e, tmp_path):
    import antiz_amd
    f = str(tmp_path / "f")
    with open(f, "wb") as fh:
        fh.write(e2e["data"])
    env = dict(os.environ, ATZ_STITCH="png", ATZ_DEVICE="0")
    r = subprocess.run([antiz_amd.CLI_PATH, "-i", f], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    assert "OK! Restoration is bit by bit identical" in r.stdout
    assert open(f + ".atz", "rb").read() == e2e["on"]
    r = subprocess.run([antiz_amd.CLI_PATH, "-r", "-i", f + ".atz", "-o", f + ".back"], env=dict(os.environ, ATZ_DEVICE="0"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    assert open(f + ".back", "rb").read() == e2e["data"]
    r = subprocess.run([antiz_amd.CLI_PATH, "-i", f], env=dict(env, ATZ_STITCH="png,apng"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 1 and "ATZ_STITCH: unknown stitcher apng" in r.stderr


def test_switch_and_shard_refusal():
    import antiz_amd
    data = txt(1, 4096) + zstrat.deflate(txt(2, 3000), 6, 15, 8, 0)
    with antiz_amd.Context(device=0, stitch=PNG) as c:
        with dev_copy(data) as d:
            with pytest.raises(antiz_amd.AtzError) as e:
                c.shard_scan(d, data, 0, 1)
            assert e.value.code == -1
        for mask in (2, 3, 1 << 31):   # an unknown bit of the mask
            with pytest.raises(antiz_amd.AtzError) as e:
                antiz_amd._check(antiz_amd.lib().atz_set_stitch(c.h, mask))
            assert e.value.code == -1
        with pytest.raises(antiz_amd.AtzError):   # the container mask keeps its two bits
            antiz_amd._check(antiz_amd.lib().atz_set_containers(c.h, 4))
        antiz_amd._check(antiz_amd.lib().atz_set_stitch(c.h, 0))
        with dev_copy(data) as d:
            assert c.shard_scan(d, data, 0, 1)
