"""antiz_amd/csrc/atz_scanext.h on the CPU: the job step and the accept step of the scan's four opt-in extensions
against the tests' Python models (zraw, zpng, zprobe, zflush).  tests/scanext_check.cpp (stand-alone, includes only
that header) is built with -fsanitize=address,undefined and run directly as a child process; it holds the file in a
heap buffer of exactly its length.  The position lists are the models' restatements of the list kernels, each printed
job is decoded by the models' own decoders (what k_inflate does on the GPU), and the records the accept step makes
must equal the models'."""
import os
import random
import struct
import subprocess
import zlib

import pytest

import _libs
import zflush
import zpng
import zprobe
import zraw
import zstrat

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "antiz_amd", "csrc")
E_INTERNAL = -8                  # include/atz_accel.h
END, ERROR = 0, 1                # InfRes.status
ARENA_OUT, NO_OUT, SLOT = -2, -1, 65536
NOSHORT, MLEV_SHIFT, AT_MARKER = 1 << 31, 27, 1 << 26   # InfRes.err
HINTS = NOSHORT | (5 << MLEV_SHIFT)                       # what every test result carries: only stitched records keep it


def rec(offset, comp_len, infl_len=1, typ=22, flags=0, arena=-1, stitch=-1, pk=0):
    """A record made before, as scanext_check reads it"""
    return (offset, comp_len, infl_len, typ, flags, arena, stitch, pk)


class Check:
    def __init__(self, exe, tmp):
        self.exe, self.tmp, self.n = exe, tmp, 0

    def path(self, data):
        self.n += 1
        p = os.path.join(self.tmp, "f%d" % self.n)
        with open(p, "wb") as f:
            f.write(data)
        return p

    def run(self, ext, cmd, data, pos, recs=(), res=None, cap=None):
        """-> (rc, {tag: [the integer fields of each line with that tag]})"""
        text = ["pos %d" % len(pos)] + [str(p) for p in pos] + ["recs %d" % len(recs)] + \
            [" ".join(str(v) for v in r) for r in recs]
        if res is not None:
            text += ["res %d" % len(res)] + [" ".join(str(v) for v in r) for r in res]
        if cap is not None:
            text.append("cap %d" % cap)
        r = subprocess.run([self.exe, ext, cmd, self.path(data), self.path("\n".join(text).encode())],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])   # (ASan / UBSan silent)
        lines = [ln.split() for ln in r.stdout.splitlines()]
        assert lines[0][0] == "rc"
        rc, out = int(lines[0][1]), {}
        assert rc == 0 or len(lines) == 1
        for t in lines[1:]:
            out.setdefault(t[0], []).append([int(x) for x in t[1:]])
        return rc, out


@pytest.fixture(scope="module")
def sc(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scanext")
    exe = str(tmp / "scanext_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(HERE, "scanext_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    return Check(exe, str(tmp))


def test_header_compiles_alone(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "atz_scanext.h"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + CSRC, str(src)],
                   check=True, timeout=120)


def txt(seed, n):
    t = _libs.text(random.Random(seed), n + 64)[:n]
    assert len(t) == n
    return t


def rnd(seed, n):
    return random.Random(seed).randbytes(n)


def spliced(recs, kept):
    """R lines: the records made before and the kept ones, in file order"""
    return sorted([list(r[:6]) + [0, 0, r[6], 0, r[7]] for r in recs] + kept)


# ---- containers ----------------------------------------------------------------------------------------------
def run_raw(sc, data, ref=(), mask=3):
    """ref: the records made before, [(offset, comp_len)] -> the kept records [(offset, comp_len, infl_len, type)],
    checked against zraw at every step"""
    anch = zraw.anchors(data, mask)
    pos = [(p << 5) | kind for p, kind in anch]
    recs = [rec(o, cl) for o, cl in ref]
    rc, out = sc.run("raw", "jobs", data, pos, recs)
    assert rc == 0
    want = [(p, c) for p, kind in anch for c in [zraw.parse(data, p, kind)] if c is not None]
    assert [(c[0], c[1], c[2], c[4]) for c in out.get("C", [])] == [(p, c["d"], c["limit"], c["hint"]) for p, c in want]
    jobs = out.get("J", [])
    assert jobs == [[c["d"], c["limit"], ARENA_OUT, SLOT] for _, c in want]
    res = []
    for off, ln, _, _ in jobs:
        r = zraw.inflate_raw(data[off:off + ln])
        res.append((END, HINTS, r[0], len(r[1])) if r else (ERROR, 0, 0, 0))
    rc, out = sc.run("raw", "accept", data, pos, recs, res)
    assert rc == 0
    kept = out.get("K", [])
    got = [tuple(k[:4]) for k in kept]
    assert got == zraw.raw_records(data, mask, list(ref))
    by_off = {}
    for k, j in enumerate(jobs):
        by_off.setdefault(j[0], k)   # (two candidates with one body: the lower anchor's)
    for k in kept:   # flags, the job's arena slot, no hints, not stitched
        assert k[4:] == [0, SLOT * by_off[k[0]], 0, 0, -1, 0, 0]
    assert out.get("R", []) == spliced(recs, kept)
    return got


def payload_body(seed, n=600, lv=6, m=8):
    p = txt(seed, n)
    return p, zraw.raw_deflate(p, lv, m)


def test_zip_entries(sc):
    p, b = payload_body(1)
    e = zraw.zip_entry
    entries = [e(b, len(p), name=b"a/b.txt", extra=b"\1\2\3\4", flags=zraw.ZIP_HINT_BITS[zraw.HINT_MAX]),   # sizes stated
               e(b, len(p), descriptor=True, flags=zraw.ZIP_HINT_BITS[zraw.HINT_FAST]),
               e(b, len(p), csize=0), e(b, len(p), csize=0xffffffff),
               e(b, len(p), csize=len(b) + 1), e(b, len(p), csize=len(b) - 1), e(b, len(p) + 1),   # wrong csize, usize
               e(b, 0xffffffff)]
    data = b"--".join(entries) + b"tail"
    got = run_raw(sc, data)
    # every body but the three with a wrong size; 0xffffffff and a data descriptor state nothing, so the decoder runs
    # to the stream's own end
    assert [g[1:] for g in got] == [(len(b), len(p), t) for t in (26, 25, 24, 24, 24)]
    assert run_raw(sc, data, mask=1) == got and run_raw(sc, data, mask=2) == []


@pytest.mark.parametrize("tail", [0, 1, 2])
def test_zip_name_and_extra_reach_the_end(sc, tail):
    # d = n, n - 1 (one byte is offered) and n - 2 (an empty final block: no output)
    data = b"xx" + zraw.zip_entry(b"", 0, name=b"n" * 5, extra=b"e" * 3) + b"\x03\x00"[:tail]
    assert run_raw(sc, data) == []
    # name and extra lengths that point past the end
    cut = zraw.zip_entry(b"", 0, name=b"n" * 5)
    assert run_raw(sc, cut[:26] + struct.pack("<HH", 0xffff, 0xffff) + cut[30:]) == []


def test_gzip_every_flag_combination(sc):
    members = []
    for flg in range(16):
        p, b = payload_body(100 + flg, 300)
        members.append(zraw.gzip_member(b, p, extra=b"ab\0d" if flg & 1 else None, name=b"file" if flg & 2 else None,
                                        comment=b"note" if flg & 4 else None, hcrc=bool(flg & 8),
                                        xfl=zraw.GZIP_XFL[flg % 3]))
    data = b"".join(members)   # (the last member's trailer ends the file)
    got = run_raw(sc, data)
    assert [g[2:] for g in got] == [(300, 24 + flg % 3) for flg in range(16)]


def test_gzip_headers_that_run_out(sc):
    fixed = struct.pack("<3sBIBB", b"\x1f\x8b\x08", 8, 0x5f010203, 0, 3)
    assert run_raw(sc, b"pad" + fixed + b"an-unterminated-name") == []
    extra = struct.pack("<3sBIBB", b"\x1f\x8b\x08", 4, 0x5f010203, 0, 3)
    assert run_raw(sc, extra + struct.pack("<H", 0xffff) + b"12345678") == []     # FEXTRA runs past the end
    assert run_raw(sc, extra[:3] + b"\x06" + extra[4:] + struct.pack("<H", 6) + b"123456") == []   # FHCRC does
    assert run_raw(sc, extra + b"1234567") == []   # (p + 18 > n: no anchor)
    assert run_raw(sc, extra + b"12345678") == []   # (p + 18 == n; the FEXTRA length points past the end)


@pytest.mark.parametrize("left", [8, 9, 10])
def test_gzip_header_ends_near_the_end(sc, left):
    # the header ends at n - left: the trailer alone, one body byte, an empty final block (no output)
    plain = struct.pack("<3sBIBB", b"\x1f\x8b\x08", 0, 0x5f010203, 0, 3)
    data = plain + (b"\x03\x00" if left == 10 else bytes(left - 8)) + bytes(8)
    assert len(data) == 10 + left and run_raw(sc, data) == []


def test_gzip_isize(sc):
    p, b = payload_body(7)
    good, bad = zraw.gzip_member(b, p), zraw.gzip_member(b, p, isize=len(p) + 1)
    assert run_raw(sc, bad + good + bad) == [(len(bad) + 10, len(b), len(p), 24)]


def test_overlapping_bodies(sc):
    p, b = payload_body(8)
    # a stored body that holds a whole entry: the inner body lies inside the outer one, which starts first
    inner = zraw.zip_entry(b, len(p))
    outer_body = zraw.raw_deflate(b"lead" + inner + b"trail", 0, 8)
    data = zraw.zip_entry(outer_body, len(inner) + 9, descriptor=True) + b"end"
    assert len(zraw.anchors(data, 3)) == 2
    assert run_raw(sc, data) == [(30, len(outer_body), len(inner) + 9, 24)]
    # two anchors with one body (a header inside the other's extra field): the lower anchor's record
    hdr = zraw.zip_entry(b"", len(p), flags=zraw.ZIP_HINT_BITS[zraw.HINT_MAX], csize=len(b))
    data = zraw.zip_entry(b, len(p), extra=hdr) + b"end"
    assert [a[0] for a in zraw.anchors(data, 3)] == [0, 30]
    assert run_raw(sc, data) == [(60, len(b), len(p), 24)]


def test_raw_meets_a_record_made_before(sc):
    p, b = payload_body(9)
    data = b"abc" + zraw.zip_entry(b, len(p)) + b"--" + zraw.gzip_member(b, p) + b"tail"
    both = run_raw(sc, data)
    assert len(both) == 2
    d = both[0][0]
    assert run_raw(sc, data, [(d, 1)]) == both[1:]                  # at its first byte
    assert run_raw(sc, data, [(d + len(b) - 1, 5)]) == both[1:]     # at its last byte
    assert run_raw(sc, data, [(d - 4, 4), (d + len(b), 3)]) == both   # touching it from outside


# ---- stitching -----------------------------------------------------------------------------------------------
def run_stitch(sc, data, prior=()):
    """prior: the records made before, [(offset, length in the file)] -> the kept records as zpng.stitched_records
    gives them, checked against zpng at every step"""
    anch = zpng.anchors(data)
    pos = [(a << 5) | 2 for a in anch]
    recs = [rec(o, n) for o, n in prior]
    rc, out = sc.run("stitch", "jobs", data, pos, recs)
    assert rc == 0
    cands, pcs, segs, jobs = out.get("C", []), out.get("P", []), out.get("G", []), out.get("J", [])
    want = zpng.candidates(data, anch)
    assert [([tuple(x) for x in pcs[c[2]:c[2] + c[3]]], c[4]) for c in cands] == want
    assert [c[1] for c in cands] == [sum(n for _, n in ch) for ch, _ in want]
    at = 0
    for c in cands:   # runs 256-byte aligned, side by side
        assert c[0] == at
        at += (c[1] + 255) & ~255
    assert out["B"] == [[at]] and at <= len(data) + 256 * len(cands)
    assert jobs == [[c[0], c[1], ARENA_OUT, SLOT] for c in cands]
    buf, filled = bytearray(at), 0
    for src, so, do, ln in segs:   # what k_gather does
        assert src == 2 and ln > 0 and so + ln <= len(data) and do + ln <= at
        buf[do:do + ln] = data[so:so + ln]
        filled += ln
    assert filled == sum(c[1] for c in cands) == zpng.gathered_bytes(data, anch)
    res = []
    for off, ln, _, _ in jobs:
        r = zpng.inflate(bytes(buf[off:off + ln]))
        res.append((END, HINTS, r[0], len(r[1])) if r else (ERROR, 0, 0, 0))
    rc, out = sc.run("stitch", "accept", data, pos, recs, res)
    assert rc == 0
    kept, pieces = out.get("K", []), [tuple(t) for t in out.get("T", [])]
    model, dropped = zpng.stitched_records(data, list(prior))
    assert [tuple(k[:4]) for k in kept] == [(m["offset"], m["comp_len"], m["infl_len"], m["type"]) for m in model]
    assert pieces == [pc for m in model for pc in m["pieces"]]   # (a dropped record's pieces are rolled back)
    runs = {pcs[c[2]][0]: (c[0], k) for k, c in enumerate(cands)}
    p0 = 0
    for k, m in zip(kept, model):   # flags, the job's arena slot, the hints, the run, the pieces
        run, job = runs[m["offset"]]
        assert k[4:] == [0, SLOT * job, 1, 5, run, p0, len(m["pieces"])]
        assert bytes(buf[run:run + m["comp_len"]]) == m["stream"]
        p0 += len(m["pieces"])
    assert out.get("R", []) == spliced(recs, kept)
    return model, dropped


@pytest.fixture(scope="module")
def zstream():
    payload = txt(4, 4000)
    stream = zstrat.deflate(payload, 6, 15, 8, 0)
    assert len(stream) > 1100
    return payload, stream


def test_stitch_chains(sc, zstream):
    payload, stream = zstream
    n = len(stream)
    for lens, junk in (([n], 0), ([400, n - 400], 0), (zpng.split(n, (n + 4) // 5), 0),   # 1, 2 and 5 chunks
                       ([0, 0, 700, n - 700], 0), ([1000, 0, n - 1000], 0),                # empty chunks
                       ([1, n - 1], 0), ([0, 1, 0, n - 1], 0),                             # the header in two chunks
                       ([n + 5, 20], 25), ([n, 20], 20),                                   # ends in / at the first chunk's end
                       ([500, n - 500, 30], 30), ([500, n - 500 + 7, 30], 37)):            # ends at / in the second's
        data, first = zpng.png(stream + bytes(junk), lens)
        kept, dropped = run_stitch(sc, data)
        stitched = len([x for x in lens if x]) >= 2 and [x for x in lens if x][0] < n
        assert len(kept) == int(stitched) and not dropped, lens
        if stitched:
            assert (kept[0]["comp_len"], kept[0]["payload"]) == (n, payload)
            assert sum(ln for _, ln in kept[0]["pieces"]) == n
    assert len(zpng.split(n, (n + 4) // 5)) == 5


def test_stitch_no_candidate(sc, zstream):
    payload, stream = zstream
    n = len(stream)
    for data in (zpng.png(b"\x78\x9d" + stream[2:], [5, n - 5])[0],                       # no zlib header
                 zpng.png(stream[:-1] + bytes([stream[-1] ^ 1]), [5, n - 5])[0],          # a broken Adler-32
                 zpng.png(b"\x78", [0, 1, 0])[0], zpng.png(b"", [0, 0])[0]):              # fewer than two bytes
        assert run_stitch(sc, data) == ([], [])


def test_stitch_chain_met_by_a_record_made_before(sc, zstream):
    payload, stream = zstream
    n = len(stream)
    pngs = [zpng.png(stream, lens)[0] for lens in ([300, n - 300], [500, 100, n - 600], [n - 9, 9])]
    data = pngs[0] + pngs[1] + pngs[2]
    kept, dropped = run_stitch(sc, data)
    assert len(kept) == 3
    mid = kept[1]["pieces"]
    # inside the framing between the middle record's pieces: it leaves, and its pieces with it
    kept, dropped = run_stitch(sc, data, [(mid[1][0] - 6, 3)])
    assert len(kept) == 2 and len(dropped) == 1
    # at its hull's first and last byte; touching it from outside
    assert len(run_stitch(sc, data, [(mid[0][0], 1)])[0]) == 2
    assert len(run_stitch(sc, data, [(mid[2][0] + mid[2][1] - 1, 4)])[0]) == 2
    assert len(run_stitch(sc, data, [(mid[0][0] - 4, 4), (mid[2][0] + mid[2][1], 4)])[0]) == 3


def test_stitch_stray_anchors_below_the_cursor(sc):
    r = random.Random(11)
    inner = bytearray(r.randbytes(1500))
    spots = list(range(100, 1400, 97))
    for k, at in enumerate(spots):   # fake type fields inside a payload, each claiming chunks far behind it
        inner[at:at + 8] = struct.pack(">I", 1200 - k) + b"IDAT"
    stream = zstrat.deflate(bytes(inner), 0, 15, 8, 0)   # stored: the fake fields survive into the stream
    tail = zstrat.deflate(txt(12, 3000), 6, 15, 8, 0)
    data = zpng.png(stream, zpng.split(len(stream), 512))[0] + zpng.png(tail, zpng.split(len(tail), 300))[0] + bytes(1500)
    anch = zpng.anchors(data)
    assert len([a for a in anch if struct.unpack_from(">I", data, a - 4)[0] > 1000]) >= 8
    assert sum(struct.unpack_from(">I", data, a - 4)[0] for a in anch) > len(data)
    kept, dropped = run_stitch(sc, data)
    assert [x["comp_len"] for x in kept] == [len(stream), len(tail)] and not dropped


# ---- probe ---------------------------------------------------------------------------------------------------
def run_probe(sc, data, prior=()):
    """prior: the records made before, [(offset, comp_len, pieces)] (pieces 0: not stitched) -> the kept records
    [(offset, comp_len, infl_len, 24)], checked against zprobe at every step"""
    pos = zprobe.positions(data)
    recs = [rec(o, cl, stitch=0 if pk else -1, pk=pk) for o, cl, pk in prior]
    hulls = [(o, cl + (12 * (pk - 1) if pk else 0)) for o, cl, pk in prior]
    rc, out = sc.run("probe", "jobs", data, pos, recs)
    assert rc == 0
    jobs = out.get("J", [])
    assert jobs == [[p, len(data) - p, ARENA_OUT, SLOT] for p in zprobe.pre_drop(pos, hulls)]
    res = []
    for off, ln, _, _ in jobs:
        r = zraw.inflate_raw(data[off:off + ln])
        res.append((END, HINTS, r[0], len(r[1])) if r else (ERROR, 0, 0, 0))
    rc, out = sc.run("probe", "accept", data, pos, recs, res)
    assert rc == 0
    kept, stats = out.get("K", []), {}
    got = [tuple(k[:4]) for k in kept]
    assert got == zprobe.probe_records(data, hulls, stats)
    assert (len(pos), len(jobs), out["N"][0]) == (stats["survivors"], stats["decoded"], [stats["accepted"], stats["kept"]])
    slot = {j[0]: SLOT * k for k, j in enumerate(jobs)}
    for k in kept:
        assert k[4:] == [0, slot[k[0]], 0, 0, -1, 0, 0]
    assert out.get("R", []) == spliced(recs, kept)
    return got


def dyn_body(nbytes, seed=1):
    payload = zprobe.skewed(seed, nbytes)
    body = zraw.raw_deflate(payload, 6, 8)
    assert (body[0] >> 1) & 3 == 2, "first block must be dynamic"
    return body


def test_probe_minimum_output(sc):
    for nbytes in (255, 256):
        body = dyn_body(nbytes, seed=nbytes)
        f = bytes(40) + body + bytes(40)
        assert 40 in zprobe.positions(f)
        assert run_probe(sc, f) == ([(40, len(body), 256, 24)] if nbytes == 256 else [])


def test_probe_and_the_records_made_before(sc):
    body = dyn_body(3000)
    f = bytes(100) + body + bytes(100)
    want = [(100, len(body), 3000, 24)]
    assert run_probe(sc, f) == want
    # a survivor inside a record's hull is not decoded: an ordinary record's bytes, a stitched one's last framing byte
    assert run_probe(sc, f, [(90, 20, 0)]) == []
    assert run_probe(sc, f, [(50, 27, 3)]) == [] and run_probe(sc, f, [(50, 26, 3)]) == want
    # the stream meets a record made before: inside it, at its last byte; touching it from outside
    assert run_probe(sc, f, [(150, 10, 0)]) == []
    assert run_probe(sc, f, [(100 + len(body) - 1, 5, 0)]) == []
    assert run_probe(sc, f, [(50, 50, 0), (100 + len(body), 30, 0)]) == want


def test_probe_greedy_pick(sc):
    a, b = zprobe.skewed(1, 2000), zprobe.skewed(2, 2000)
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    first = z.compress(a) + z.flush(zlib.Z_FULL_FLUSH)
    whole = first + z.compress(b) + z.flush()
    f = bytes(64) + whole + bytes(64)
    assert zprobe.accept(f, 64 + len(first)) == (len(whole) - len(first), 2000)   # a stream of its own, inside the first
    assert run_probe(sc, f) == [(64, len(whole), 4000, 24)]
    one, two = dyn_body(1500, 3), dyn_body(1600, 4)
    f = bytes(10) + one + two + bytes(10)
    assert run_probe(sc, f) == [(10, len(one), 1500, 24), (10 + len(one), len(two), 1600, 24)]


def test_probe_without_survivors(sc):
    assert run_probe(sc, bytes(3000)) == [] and run_probe(sc, b"") == []
    assert run_probe(sc, bytes(3000), [(10, 100, 0)]) == []


# ---- segments ------------------------------------------------------------------------------------------------
def run_seg(sc, data, recs5, arena=-1):
    """recs5: the records made before, [(offset, type, comp_len, infl_len, flags)] (flags bit 6: stitched) -> the
    records after the step in that form, checked against zflush at every step"""
    ms = zflush.markers(data)
    recs = [rec(o, cl, il, t, fl & ~64, arena, 0 if fl & 64 else -1, 2 if fl & 64 else 0) for o, t, cl, il, fl in recs5]
    rc, out = sc.run("seg", "jobs", data, ms, recs)
    assert rc == 0
    el, jobs = out.get("E", []), out.get("J", [])
    want_el = []
    for k, r in enumerate(recs5):
        b = zflush.body_of(data, r)
        if b is not None and not r[4] & 64 and r[0] + r[2] <= len(data) and any(b[0] <= q and q + 4 < b[1] for q in ms):
            want_el.append((k, b[0], b[1]))
    assert [tuple(e[:3]) for e in el] == want_el
    want_jobs = []
    for _, b0, b1 in want_el:
        want_jobs += [[s, b1 - s, NO_OUT, 0] for s in [b0] + [q + 4 for q in ms if b0 <= q and q + 4 < b1]]
    assert jobs == want_jobs and (not el or (el[0][3] == 0 and el[-1][4] == len(jobs)))
    res = []
    for off, ln, _, _ in jobs:
        st, consumed, o, am = zflush.seg_inflate(data[off:off + ln])
        res.append((st, HINTS | (AT_MARKER if am else 0), consumed, len(o)))
    rc, out = sc.run("seg", "accept", data, ms, recs, res)
    assert rc == 0
    after = out.get("R", [])
    got = [(r[0], r[3], r[1], r[2], r[4] | (64 if r[8] != -1 else 0)) for r in after]
    want = zflush.split(data, [r for r in recs5])
    assert got == want
    made = [r for r in want if r not in [tuple(x) for x in recs5]]
    assert out["N"][0][1] == len(made)
    for r in after:   # no hints; a segment's arena range lies in its parent's, the outputs side by side
        assert r[6:8] == [0, 0]
    if arena >= 0:
        for o, t, cl, il, fl in recs5:
            inside = [r for r in after if o <= r[0] < o + cl]
            assert [r[5] for r in inside] == [arena + sum(x[2] for x in inside[:k]) for k in range(len(inside))]
    return got


SEGS = None


def segments():
    global SEGS
    if SEGS is None:
        SEGS = [txt(21, 300), txt(22, 2000), txt(23, 1500)]
    return SEGS


def test_seg_parents(sc):
    segs, pre = segments(), rnd(24, 100)
    stream, ends = zflush.flush_stream(segs, 6, 8, -15)
    data = pre + stream + rnd(25, 50)
    at = [100] + [100 + e for e in ends[:-1]]
    want = [(at[0], 26, ends[0], 300, 128), (at[1], 26, ends[1] - ends[0], 2000, 128), (at[2], 26, ends[2] - ends[1], 1500, 0)]
    assert run_seg(sc, data, [(100, 26, len(stream), 3800, 0)]) == want
    assert run_seg(sc, data, [(100, 26, len(stream), 3800, 0)], arena=7 * SLOT) == want
    assert run_seg(sc, data, [(100, 27, len(stream), 3800, 0)]) == [(100, 27, len(stream), 3800, 0)]   # no raw type
    for level, typ in ((1, 25), (2, 25), (6, 24), (9, 26)):   # a zlib parent's FLEVEL
        zs, ze = zflush.flush_stream(segs, level, 8, 15)
        parent = (100, 20 + (zs[1] >> 6), len(zs), 3800, 0)
        got = run_seg(sc, pre + zs, [(10, 22, 50, 9, 0), parent])
        assert [(r[1], r[3], r[4]) for r in got[1:]] == [(typ, 300, 128), (typ, 2000, 128), (typ, 1500, 0)]
        assert got[0] == (10, 22, 50, 9, 0) and got[1][0] == 102 and got[-1][0] + got[-1][2] == len(pre + zs) - 4
        # stitched: skipped
        assert run_seg(sc, pre + zs, [parent[:4] + (64,)]) == [parent[:4] + (64,)]
    z14, _ = zflush.flush_stream(segs, 6, 8, 14)   # another window: skipped
    assert run_seg(sc, z14, [(0, 16 + (z14[1] >> 6), len(z14), 3800, 0)]) == [(0, 16 + (z14[1] >> 6), len(z14), 3800, 0)]
    # a record that reaches past the file's end (the reference's scan can make one) is left alone
    assert run_seg(sc, data, [(100, 26, len(data), 3800, 0)]) == [(100, 26, len(data), 3800, 0)]


def test_seg_marker_places(sc):
    a, b = txt(31, 1200), txt(32, 900)
    # a marker at body_start: a job at body_start + 4, and no chain
    junk = zflush.MARKER + rnd(33, 200)
    assert run_seg(sc, junk, [(0, 24, len(junk), 500, 0)]) == [(0, 24, len(junk), 500, 0)]
    zj = b"\x78\x9c" + junk
    assert run_seg(sc, zj, [(0, 22, len(zj), 500, 0)]) == [(0, 22, len(zj), 500, 0)]
    # q + 4 == body_end: that marker makes no job; alone, it leaves the record ineligible
    fa = zflush.flushed_deflate(a, 6, 8)
    assert zflush.markers(fa) == [len(fa) - 4]
    assert run_seg(sc, fa, [(0, 24, len(fa), 1200, 0)]) == [(0, 24, len(fa), 1200, 0)]
    two = fa + zflush.flushed_deflate(b, 6, 8)
    assert run_seg(sc, two, [(0, 24, len(two), 2100, 0)]) == [(0, 24, len(two), 2100, 0)]   # (no final block follows)
    # a final segment without output makes no record
    fin = fa + b"\x03\x00"
    assert run_seg(sc, fin, [(0, 24, len(fin), 1200, 0)]) == [(0, 24, len(fa), 1200, 128)]
    # a middle segment without output breaks the chain
    mid = fa + b"\x00" + zflush.MARKER + zraw.raw_deflate(b, 6, 8)
    assert run_seg(sc, mid, [(0, 24, len(mid), 2100, 0)]) == [(0, 24, len(mid), 2100, 0)]


def test_seg_false_markers_and_broken_chains(sc):
    a, b = rnd(41, 600) + zflush.MARKER, rnd(42, 300) + zflush.MARKER + rnd(43, 300)
    stream, ends = zflush.flush_stream([a, b], 0, 8, -15)   # stored: the pattern survives into the stream
    assert len(zflush.markers(stream)) == 3
    whole = (0, 24, len(stream), 1208, 0)
    assert run_seg(sc, stream, [whole]) == [(0, 24, ends[0], 604, 128), (ends[0], 24, ends[1] - ends[0], 604, 0)]
    bad = bytearray(stream)   # the true marker changed: the false ones keep the record eligible, the chain breaks
    bad[ends[0] - 1] = 0xfe
    assert run_seg(sc, bytes(bad), [whole]) == [whole]
    assert run_seg(sc, stream, [(0, 24, len(stream), 1209, 0)]) == [(0, 24, len(stream), 1209, 0)]   # the outputs' sum
    # k = 1: a stored block whose payload holds the pattern makes the record eligible, and no more
    one = zraw.raw_deflate(rnd(44, 500) + zflush.MARKER + rnd(45, 500), 0, 8)
    assert zflush.markers(one) and run_seg(sc, one, [(0, 24, len(one), 1004, 0)]) == [(0, 24, len(one), 1004, 0)]
    # sync flush: the second segment's matches reach into the first
    t = txt(46, 1500)
    sync, se = zflush.flush_stream([t, t], 6, 8, -15, zflush.Z_SYNC_FLUSH)
    assert run_seg(sc, sync, [(0, 24, len(sync), 3000, 0)]) == [(0, 24, len(sync), 3000, 0)]


# ---- the contract with the kernels -------------------------------------------------------------------------------
def internal(sc, ext, cmd, data, pos, recs=(), res=None, cap=None):
    rc, out = sc.run(ext, cmd, data, pos, recs, res, cap)
    assert rc == E_INTERNAL and not out
    return True


def test_contract_anchor_lists(sc):
    zipf = b"ab" + zraw.zip_entry(b"\x03\x00", 0) + bytes(40)
    assert sc.run("raw", "jobs", zipf, [(2 << 5) | 0])[0] == 0
    for ext in ("raw", "stitch"):   # a list that is not ascending
        assert internal(sc, ext, "jobs", zipf, [(2 << 5) | 0, (2 << 5) | 0])
        assert internal(sc, ext, "jobs", zipf, [(9 << 5) | 1, (2 << 5) | 0])
    n = len(zipf)
    assert sc.run("raw", "jobs", zipf, [((n - 30) << 5) | 0, ((n - 18) << 5) | 1])[0] == 0
    assert internal(sc, "raw", "jobs", zipf, [((n - 29) << 5) | 0])    # a ZIP anchor with p + 30 > n
    assert internal(sc, "raw", "jobs", zipf, [((n - 17) << 5) | 1])    # a gzip anchor with p + 18 > n
    assert internal(sc, "raw", "jobs", zipf, [((1 << 57) << 5) | 0]) and internal(sc, "raw", "jobs", b"", [0])
    png = bytes(3) + zpng.chunk(b"IDAT", b"\x78\x9c12345")
    assert sc.run("stitch", "jobs", png, [(7 << 5) | 2])[0] == 0
    idat = lambda lead, length, tail: bytes(lead) + struct.pack(">I", length) + b"IDAT" + bytes(tail)
    assert internal(sc, "stitch", "jobs", b"\0\0\0IDAT" + bytes(20), [(3 << 5) | 2])             # p < 4
    assert sc.run("stitch", "jobs", idat(0, 5, 9), [(4 << 5) | 2])[0] == 0
    assert internal(sc, "stitch", "jobs", idat(0, 5, 8), [(4 << 5) | 2])                         # p + 8 + L > n
    assert internal(sc, "stitch", "jobs", idat(0, 1 << 31, 20), [(4 << 5) | 2])                  # L >= 2^31
    assert internal(sc, "stitch", "jobs", idat(0, 0xffffffff, 20), [(4 << 5) | 2])
    assert internal(sc, "stitch", "jobs", idat(0, 0, 3), [(4 << 5) | 2])                         # p + 8 > n
    assert internal(sc, "stitch", "jobs", idat(0, 0, 3), [(11 << 5) | 2, (12 << 5) | 2])         # p >= n


def test_contract_position_lists(sc):
    data = bytes(100)
    assert sc.run("probe", "jobs", data, [5, 99])[0] == 0
    assert internal(sc, "probe", "jobs", data, [100]) and internal(sc, "probe", "jobs", data, [5, 5])
    assert internal(sc, "probe", "jobs", data, [7, 5]) and internal(sc, "probe", "jobs", b"", [0])
    r = [rec(0, 100, 10, 24)]
    assert sc.run("seg", "jobs", data, [5, 96], r)[0] == 0
    assert internal(sc, "seg", "jobs", data, [97], r) and internal(sc, "seg", "jobs", data, [1 << 62], r)   # q + 4 > F
    assert internal(sc, "seg", "jobs", data, [9, 9], r) and internal(sc, "seg", "jobs", data, [9, 5], r)


def contract_cases():
    p, b = payload_body(50)
    gz = zraw.gzip_member(b, p)
    _, stream = txt(51, 2000), zstrat.deflate(txt(51, 2000), 6, 15, 8, 0)
    png = zpng.png(stream, [300, len(stream) - 300])[0]
    body = dyn_body(1000)
    fl, _ = zflush.flush_stream([txt(52, 500), txt(53, 500)], 6, 8, -15)
    return [("raw", gz, [(p_ << 5) | k for p_, k in zraw.anchors(gz, 3)], []),
            ("stitch", png, [(a << 5) | 2 for a in zpng.anchors(png)], []),
            ("probe", bytes(8) + body, zprobe.positions(bytes(8) + body), []),
            ("seg", fl, zflush.markers(fl), [rec(0, len(fl), 1000, 24)])]


def test_contract_results(sc):
    for ext, data, pos, recs in contract_cases():
        rc, out = sc.run(ext, "jobs", data, pos, recs)
        jobs = out["J"]
        assert rc == 0 and jobs
        ok = [(ERROR, 0, 0, 0)] * len(jobs)
        assert sc.run(ext, "accept", data, pos, recs, ok)[0] == 0
        # a result list of the wrong length
        assert internal(sc, ext, "accept", data, pos, recs, ok[1:]) and internal(sc, ext, "accept", data, pos, recs, ok + ok[:1])
        # a decode that ended behind what its job offered (a gzip body's ISIZE would be read past the file's end)
        last = jobs[-1]
        assert sc.run(ext, "accept", data, pos, recs, ok[:-1] + [(END, 0, last[1], 300)])[0] == 0
        assert internal(sc, ext, "accept", data, pos, recs, ok[:-1] + [(END, 0, last[1] + 1, 300)])
        # (a decode that did not end says nothing of its input)
        assert sc.run(ext, "accept", data, pos, recs, ok[:-1] + [(ERROR, 0, last[1] + 1, 300)])[0] == 0


def test_records_keep_their_capacity(sc):
    p, b = payload_body(60)
    data = zraw.gzip_member(b, p) + bytes(20)
    pos = [(p_ << 5) | k for p_, k in zraw.anchors(data, 3)]
    recs = [rec(len(data) - 10, 5)]
    res = [(END, 0, len(b), len(p))]
    rc, out = sc.run("raw", "accept", data, pos, recs, res, cap=2)
    assert rc == 0 and len(out["R"]) == 2
    assert internal(sc, "raw", "accept", data, pos, recs, res, cap=1)   # it would grow
    fl, ends = zflush.flush_stream([txt(61, 500), txt(62, 500)], 6, 8, -15)
    ms, parent = zflush.markers(fl), [rec(0, len(fl), 1000, 24)]
    res = [(END, AT_MARKER, ends[0], 500), (END, 0, ends[1] - ends[0], 500)]
    assert sc.run("seg", "accept", fl, ms, parent, res, cap=2)[0] == 0
    assert internal(sc, "seg", "accept", fl, ms, parent, res, cap=1)
