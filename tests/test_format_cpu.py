"""antiz_amd/csrc/atz_format.h on the CPU: the ATZ reader, the reconstruct plan and the writer.  tests/format_check.cpp
(stand-alone, includes only that header) is built with -fsanitize=address,undefined and run directly as a child
process; it executes the plans' segments and patches with memcpy after checking every range against its buffer, and
exits non-zero on a violation.

What a rebuilt file must equal: the oracle's ATZ1 reader (oracle/ora_pipeline.c, the reference's reconstructATZ
restated) where the file is an ATZ1, else a Python model of the piece placement.  The deflate
outputs the plan places are the oracle's for oracle-checked files and arbitrary seeded bytes elsewhere: the plan does
not look at them."""
import os
import random
import struct
import subprocess

import pytest

import _libs
import atzfile
import golden_cases as G
import zpng

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "antiz_amd", "csrc")
GOLD = os.path.join(HERE, "golden")
E_REF_ABORT, E_REF_UB, E_FORMAT = -5, -6, -7   # include/atz_accel.h


class Check:
    def __init__(self, exe, tmp):
        self.exe, self.tmp, self.n = exe, tmp, 0

    def path(self, data=None):
        self.n += 1
        p = os.path.join(self.tmp, "f%d" % self.n)
        if data is not None:
            with open(p, "wb") as f:
                f.write(data)
        return p

    def run(self, *args):
        r = subprocess.run([self.exe] + list(args), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
        return [ln.split() for ln in r.stdout.splitlines()]

    def parse(self, files):
        """-> per file (rc, version, origlen, [descriptor fields off cl il c w m nd fd k ipos])"""
        out = []
        for t in self.run("parse", *[self.path(a) for a in files]):
            if t[0] == "P":
                out.append((int(t[1]), int(t[2]), int(t[3]), []))
            else:
                assert t[0] == "D"
                out[-1][3].append([int(x) for x in t[1:]])
        assert len(out) == len(files)
        return out

    def rebuild(self, jobs):
        """jobs: [(atz, [each stream's deflate output])] -> per job (rc, the rebuilt bytes or None, [the streams'
        level window memlevel strategy raw gnu flush address])"""
        args, outs = [], []
        for atz, streams in jobs:
            blob = b"".join(struct.pack("<Q", len(s)) + s for s in streams)
            args += [self.path(atz), self.path(blob), self.path()]
        res, specs = [], []
        for t in self.run("rebuild", *args):
            if t[0] == "P":
                specs = []
            elif t[0] == "S":
                specs.append([int(x) for x in t[1:]])
            elif t[0] == "R":
                res.append((int(t[1]), specs))
        assert len(res) == len(jobs)
        for k, (rc, specs) in enumerate(res):
            back = None
            if rc == 0:
                with open(args[3 * k + 2], "rb") as f:
                    back = f.read()
            outs.append((rc, back, specs))
        return outs

    def write(self, table, orig):
        """table: [dict(off, cl, il, recomp, c, w, m, first_diff, pos, val, pieces [(offset, length)], payload)]
        -> (rc, the ATZ bytes or None)"""
        lines = [str(len(table))]
        for x in table:
            pc = x.get("pieces") or []
            lines.append(" ".join(str(v) for v in [x["off"], x["cl"], x["il"], int(x["recomp"]), x["c"], x["w"], x["m"],
                                                    x["first_diff"], len(x["pos"]), len(pc)] + list(x["pos"]) +
                                  [bytes(x["val"]).hex() or "-"] + [o for o, _ in pc] + [n for _, n in pc] +
                                  [x["payload"].hex() or "-"]))
        out = self.path()
        (t,) = self.run("write", self.path("\n".join(lines).encode()), self.path(orig), out)
        assert t[0] == "W"
        if int(t[1]):
            return int(t[1]), None
        with open(out, "rb") as f:
            atz = f.read()
        assert len(atz) == int(t[2])
        return 0, atz


@pytest.fixture(scope="module")
def fc(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("format")
    exe = str(tmp / "format_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(HERE, "format_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    return Check(exe, str(tmp))


def test_header_compiles_alone(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "atz_format.h"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + CSRC, str(src)],
                   check=True, timeout=120)


# ---- helpers ---------------------------------------------------------------------------------------------
def payload_of(d):
    head = 35 + (8 + 9 * d["nd"] if d["nd"] else 0)
    return d["raw"][head:head + d["il"]]


def oracle_outputs(atz):
    """Each stream's deflate as the reference's reader runs it (doDeflate, main.cpp:976-1003)."""
    return [_libs.ora_deflate(payload_of(d), d["c"], d["w"], d["m"])[0] for d in atzfile.parse(atz)[2]]


def same_as_atzfile(atz, parsed):
    """The C++ reader's dump of an accepted file against tests/atzfile.py."""
    rc, ver, origlen, rows = parsed
    pv, po, descs, _ = atzfile.parse(atz)
    assert (rc, ver, origlen, len(rows)) == (0, pv, po, len(descs))
    at = 28
    for row, d in zip(rows, descs):
        ipos = at + 35 + (8 + 9 * d["nd"] if d["nd"] else 0)
        assert row == [d["off"], d["cl"], d["il"], d["c"], d["w"], d["m"], d["nd"], d["first_diff"] if d["nd"] else 0,
                       len(d["pieces"]) if d["pieces"] else 0, ipos]
        at += len(d["raw"])


def build_atz(version, origlen, streams, residue):
    """ATZ bytes: streams = [dict(off, cl, payload, c, w, m, fd, deltas, vals, pieces)], pieces
    the lengths of a stitched descriptor's list (c then carries bit 7) or None."""
    body = b""
    for s in streams:
        deltas = s.get("deltas", [])
        body += struct.pack("<QQQBBBQ", s["off"], s["cl"], len(s["payload"]), s["c"], s["w"], s["m"], len(deltas))
        if deltas:
            body += struct.pack("<Q", s["fd"]) + b"".join(struct.pack("<Q", d) for d in deltas) + bytes(s["vals"])
        body += s["payload"]
        if s.get("pieces") is not None:
            body += struct.pack("<I", len(s["pieces"])) + b"".join(struct.pack("<I", n) for n in s["pieces"])
    n = 28 + len(body) + len(residue)
    return b"ATZ" + bytes([version]) + struct.pack("<QQQ", n, origlen, len(streams)) + body + residue


def model_rebuild(origlen, streams, outputs, residue):
    """The original of build_atz's file: each stream's first cl output bytes, zero-extended, then its diffs (first_diff
    plus the deltas' sums, those below cl, in order: the last write wins); piece i goes to off + sum(len_j + 12, j < i)
    and every other byte, the framing between pieces included, comes from the residue in order."""
    out, taken = bytearray(origlen), bytearray(origlen)
    for s, o in zip(streams, outputs):
        b = bytearray((o[:s["cl"]] + bytes(s["cl"]))[:s["cl"]])
        at = s.get("fd", 0)
        for d, v in zip(s.get("deltas", []), s.get("vals", [])):
            at = (at + d) & (2 ** 64 - 1)
            if at < s["cl"]:
                b[at] = v
        sp, fp = 0, s["off"]
        for n in (s["pieces"] if s.get("pieces") is not None else [s["cl"]]):
            out[fp:fp + n] = b[sp:sp + n]
            taken[fp:fp + n] = b"\1" * n
            sp, fp = sp + n, fp + n + 12
    free = [k for k in range(origlen) if not taken[k]]
    assert len(free) == len(residue)
    for k, v in zip(free, residue):
        out[k] = v
    return bytes(out)


# ---- the oracle corpus -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus():
    """tests/test_gpu.py test_reconstruct_fuzzed_atz_rejected_or_equal_to_oracle's files and mutants."""
    r = random.Random(4242)
    files = []
    for i, data, cs, opts in G.fuzz_cases(400, 99):
        if len(files) == 30:
            break
        rc, want, st = _libs.ora_precompress(data, chunksize=cs, **G.opts_kwargs(opts))
        if rc == 0 and len(want) > 40 and st["streams"]:
            files.append((data, want, opts))
    assert len(files) >= 20
    mutants = []
    for data, good, opts in files:
        for _ in range(25):
            b = bytearray(good)
            if r.random() < 0.15:
                b = b[:r.randrange(28, len(b))]
                b[4:12] = struct.pack("<Q", len(b))   # keep the length field consistent
            else:
                hi = min(len(b), 28 + 43 * 3) if r.random() < 0.8 else len(b)
                at = r.randrange(12, hi)             # past the magic and the length field
                b[at] = r.randrange(256) if r.random() < 0.5 else b[at] ^ (1 << r.randrange(8))
            mutants.append(bytes(b))
    return files, mutants


def test_unmutated_files_rebuild_their_inputs(fc, corpus):
    files, _ = corpus
    goods = [good for _, good, _ in files]
    for good, parsed in zip(goods, fc.parse(goods)):
        same_as_atzfile(good, parsed)
    for (data, _, _), (rc, back, _) in zip(files, fc.rebuild([(g, oracle_outputs(g)) for g in goods])):
        assert rc == 0 and back == data


def test_mutants_refused_or_equal_to_oracle(fc, corpus):
    _, mutants = corpus
    parsed = fc.parse(mutants)
    ok = [b for b, p in zip(mutants, parsed) if p[0] == 0]
    for b, p in zip(mutants, parsed):
        if p[0] == 0:
            same_as_atzfile(b, p)
    refused = len(mutants) - len(ok)
    accepted = 0
    for b, (rc, back, specs) in zip(ok, fc.rebuild([(b, oracle_outputs(b)) for b in ok])):
        if rc != 0:   # the batch step's refusal: only the code is recorded
            assert rc == E_REF_ABORT
            refused += 1
            continue
        orc, want = _libs.ora_reconstruct(b)
        assert orc == 0 and back == want
        for d, s in zip(atzfile.parse(b)[2], specs):   # window 8 read as 9
            assert s[:7] == [d["c"], 9 if d["w"] == 8 else d["w"], d["m"], 0, 0, 0, 0]
        accepted += 1
    assert accepted > 0 and refused > 0


# ---- crafted size fields ---------------------------------------------------------------------------------
def test_crafted_size_fields_are_format_errors(fc):
    """The six files of test_gpu.py test_reconstruct_rejects_crafted_atz."""
    with open(os.path.join(GOLD, "zt", "input.bin"), "rb") as f:
        data = f.read()[:3000]
    s, _ = _libs.ora_deflate(_libs.text(random.Random(3), 5000), 6, 15, 8)
    data = data + s + b"tail"
    rc, good, st = _libs.ora_precompress(data)
    assert rc == 0 and struct.unpack_from("<Q", good, 20)[0] >= 1
    n = len(good)

    def put(at, v):
        b = bytearray(good)
        b[at:at + 8] = struct.pack("<Q", v)
        return bytes(b)
    cut = bytearray(good[:n // 2])
    cut[4:12] = struct.pack("<Q", len(cut))
    bad = [put(20, 1 << 62), put(28 + 16, (1 << 64) - 30), put(28 + 27, 1 << 61), put(28 + 8, 1 << 63),
           put(28, (1 << 64) - 1), bytes(cut)]
    res = fc.parse([good] + bad)
    assert res[0][0] == 0
    assert [p[0] for p in res[1:]] == [E_FORMAT] * 6


# ---- diff lists ------------------------------------------------------------------------------------------
def test_diff_cases_match_oracle(fc):
    """The cases of test_gpu.py test_reconstruct_diffs_match_oracle."""
    r = random.Random(11)
    text = _libs.text(r, 3000)
    real, _ = _libs.ora_deflate(text, 6, 15, 8)
    cl = len(real)
    cases = [
        (0, [0, 3, 0, 0, 7], [1, 2, 3, 4, 5]),                 # repeated positions: the last byte wins
        (5, [0, 1, 1, 1 << 40], [9, 8, 7, 6]),                  # a position far past comp_len
        (cl - 2, [0, 1, 5], [0xaa, 0xbb, 0xcc]),                # straddling the end of the stream
    ]
    jobs, want = [], []
    for fd, deltas, vals in cases:
        for extra in (0, 9):                                   # comp_len beyond the deflate output: zeros
            s = dict(off=2, cl=cl + extra, payload=text, c=6, w=15, m=8, fd=fd, deltas=deltas, vals=vals)
            a = build_atz(1, cl + extra + 6, [s], b"ab" + b"wxyz")
            rc, w = _libs.ora_reconstruct(a)
            assert rc == 0 and w == model_rebuild(cl + extra + 6, [s], [real], b"abwxyz")
            jobs.append((a, [real]))
            want.append(w)
    for (rc, back, _), w in zip(fc.rebuild(jobs), want):
        assert rc == 0 and back == w


# ---- stitched descriptors --------------------------------------------------------------------------------
def stitched_file(lens, out_extra, seed):
    """One stitched stream of pieces `lens` between 5 leading and 4 trailing bytes, a diff on the last byte of every
    piece that has one and on the first byte of the piece after it; its output is cl + out_extra arbitrary bytes."""
    r = random.Random(seed)
    cl = sum(lens)
    starts = [sum(lens[:i]) for i in range(len(lens))]
    pos = sorted({p for st, n in zip(starts, lens) if n for p in (st + n - 1, st + n) if p < cl})
    s = dict(off=5, cl=cl, payload=r.randbytes(11), c=0x86, w=15, m=8, pieces=list(lens), fd=pos[0],
             deltas=[0] + [b - a for a, b in zip(pos, pos[1:])], vals=list(r.randbytes(len(pos))))
    origlen = 5 + cl + 12 * (len(lens) - 1) + 4
    residue = r.randbytes(origlen - cl)
    return s, origlen, residue, r.randbytes(cl + out_extra), pos


@pytest.mark.parametrize("lens", [(1, 7, 1), (5, 0, 5)])
def test_stitched_streams_match_the_model(fc, lens):
    jobs, want, files = [], [], []
    for extra in (-3, 0, 4):
        s, origlen, residue, out, _ = stitched_file(lens, extra, 100 + extra)
        a = build_atz(4, origlen, [s], residue)
        jobs.append((a, [out]))
        want.append(model_rebuild(origlen, [s], [out], residue))
        files.append(a)
    for a, parsed in zip(files, fc.parse(files)):
        same_as_atzfile(a, parsed)
    for (rc, back, _), w in zip(fc.rebuild(jobs), want):
        assert rc == 0 and back == w


def test_stitched_refusals(fc):
    """The files of test_gpu_png.py test_atz4_reader_refuses_bad_piece_lists, with the code each rule gives."""
    from test_gpu_png import cases, expected_scan
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
    cut = o + zpng.hull(rec["pieces"])   # (the hull's last byte may be the original's last)
    res = zpng.residue(data[:cut], rec["pieces"])
    body = zpng.descriptor(rec, 6, 15, 8)
    files = [atz([rec]), b"ATZ\4" + struct.pack("<QQQ", 28 + len(body) + len(res), cut, 1) + body + res,
             atz([one]), atz([short]), atz([empty_first]), atz([empty_last]), atz([late]),
             atz([rec], origlen=o + n + 11), atz([rec, second]), atz([both_bits])]
    assert [p[0] for p in fc.parse(files)] == [0, 0] + [E_FORMAT] * 7 + [E_REF_ABORT]
    outs = [rec["stream"]]   # (what the stream's deflate gives when its parameters are the recorded ones)
    (rc0, back0, _), (rc1, back1, _) = fc.rebuild([(files[0], outs), (files[1], outs)])
    assert (rc0, back0) == (0, data) and (rc1, back1) == (0, data[:cut])


# ---- versions --------------------------------------------------------------------------------------------
NEWEST = {1: (0x06, 15, 8), 2: (0x16, 15, 8), 3: (0x46, 15, 8), 4: (0x86, 15, 8), 5: (0x46, 15, 0), 6: (0x46, 0x8f, 8)}


def test_versions(fc):
    """Version v's newest descriptor parses under its own magic and every later one, and is refused under an older."""
    r = random.Random(6)
    files, want, rebuilt = [], [], []
    for v, (c, w, m) in NEWEST.items():
        pieces = [4, 6] if c & 0x80 else None
        s = dict(off=2, cl=10, payload=r.randbytes(5), c=c, w=w, m=m, pieces=pieces)
        origlen = 2 + 10 + (12 if pieces else 0) + 3
        residue, out = r.randbytes(origlen - 10), r.randbytes(10)
        for magic in range(0, 8):
            files.append(build_atz(magic, origlen, [s], residue))
            want.append(E_FORMAT if magic in (0, 7) else E_REF_ABORT if magic < v else 0)
        rebuilt.append((build_atz(v, origlen, [s], residue), [out], model_rebuild(origlen, [s], [out], residue)))
    parsed = fc.parse(files)
    assert [p[0] for p in parsed] == want
    for a, p in zip(files, parsed):
        if p[0] == 0:
            same_as_atzfile(a, p)
    for (rc, back, _), (_, _, w) in zip(fc.rebuild([(a, o) for a, o, _ in rebuilt]), rebuilt):
        assert rc == 0 and back == w


# ---- the writer ------------------------------------------------------------------------------------------
def table_of(atz):
    """The writer's table of a file's recorded streams (the other records are residue either way)."""
    out = []
    for d in atzfile.parse(atz)[2]:
        at, pc = d["off"], []
        for n in d["pieces"] or []:
            pc.append((at, n))
            at += n + 12
        out.append(dict(off=d["off"], cl=d["cl"], il=d["il"], recomp=1, c=d["c"] & 0x7f, w=d["w"], m=d["m"],
                        first_diff=d["first_diff"], pos=d["pos"], val=d["val"], pieces=pc, payload=payload_of(d)))
    return out


def test_writer_reproduces_the_oracle_files(fc, corpus):
    files, _ = corpus
    for data, good, _ in files:
        assert fc.write(table_of(good), data) == (0, good)


@pytest.mark.parametrize("lens", [(1, 7, 1), (5, 0, 5)])
def test_writer_reproduces_the_stitched_file(fc, lens):
    s, origlen, residue, out, _ = stitched_file(lens, 0, 7)
    a = build_atz(4, origlen, [s], residue)
    assert fc.write(table_of(a), model_rebuild(origlen, [s], [out], residue)) == (0, a)


def test_writer_refuses_overlapping_records(fc):
    rec = dict(il=0, recomp=0, c=6, w=15, m=8, first_diff=-1, pos=[], val=b"", payload=b"")
    assert fc.write([dict(rec, off=10, cl=20), dict(rec, off=15, cl=20)], bytes(100)) == (E_REF_UB, None)
    assert fc.write([dict(rec, off=10, cl=20), dict(rec, off=30, cl=20)], bytes(100))[0] == 0
