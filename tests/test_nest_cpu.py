"""Nested files ("ATN" 1) on the CPU: the tests' model (tests/znest.py) and the product's reader,
reconstruct plans and writer (antiz_amd/csrc/atz_format.h).  tests/nest_check.cpp (stand-alone, includes only that
header) is built with -fsanitize=address,undefined and run directly as a child process; it executes both levels' plans
with memcpy at fake, far-apart base addresses after checking every range against its buffer, and exits with status 3 on
a violation."""
import os
import random
import struct
import subprocess

import pytest

import _libs
import atzfile
import znest
from test_format_cpu import build_atz, stitched_file, table_of, model_rebuild, CSRC, HERE

E_REF_ABORT, E_FORMAT = -5, -7   # include/atz_accel.h


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

    @staticmethod
    def _levels(lines, res):
        for t in lines:
            if t[0] == "N":
                res.append([int(t[1]), []])
            elif t[0] == "L":
                res[-1][1].append([int(x) for x in t[1:]] + [[]])
            elif t[0] == "D":
                res[-1][1][-1][-1].append([int(x) for x in t[1:]])

    def parse(self, files):
        """-> per file [rc, [per level, outermost first: pos len version origlen nstreams stripped [descriptor rows]]]"""
        out = []
        self._levels(self.run("parse", *[self.path(a) for a in files]), out)
        assert len(out) == len(files)
        return out

    def rebuild(self, jobs):
        """jobs: [(file, [each stream's deflate output, innermost level first])] -> per job (rc, rebuilt bytes or None)"""
        args = []
        for f, streams in jobs:
            blob = b"".join(struct.pack("<Q", len(s)) + s for s in streams)
            args += [self.path(f), self.path(blob), self.path()]
        rcs = [int(t[1]) for t in self.run("rebuild", *args) if t[0] == "R"]
        assert len(rcs) == len(jobs)
        out = []
        for k, rc in enumerate(rcs):
            back = None
            if rc == 0:
                with open(args[3 * k + 2], "rb") as f:
                    back = f.read()
            out.append((rc, back))
        return out

    def write(self, table, orig, inner):
        """table: test_format_cpu's -> (rc, the nested file, P)"""
        lines = [str(len(table))]
        for x in table:
            pc = x.get("pieces") or []
            lines.append(" ".join(str(v) for v in [x["off"], x["cl"], x["il"], int(x["recomp"]), x["c"], x["w"], x["m"],
                                                    x["first_diff"], len(x["pos"]), len(pc)] + list(x["pos"]) +
                                  [bytes(x["val"]).hex() or "-"] + [o for o, _ in pc] + [n for _, n in pc] +
                                  [x["payload"].hex() or "-"]))
        out = self.path()
        (t,) = self.run("write", self.path("\n".join(lines).encode()), self.path(orig), self.path(inner), out)
        assert t[0] == "W"
        if int(t[1]):
            return int(t[1]), None, None
        with open(out, "rb") as f:
            atn = f.read()
        with open(out + ".p", "rb") as f:
            P = f.read()
        assert len(atn) == int(t[2]) and len(P) == int(t[3])
        return 0, atn, P


@pytest.fixture(scope="module")
def nc(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("nest")
    exe = str(tmp / "nest_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(HERE, "nest_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    return Check(exe, str(tmp))


@pytest.fixture(scope="module")
def files():
    """[(data, depth, the model's file)]: one, two and three "ATN" headers, a diff list in an outer descriptor."""
    r = random.Random(77)
    out = []
    for deeper, depth in ((0, 1), (1, 2), (2, 4)):
        data = znest.sample(r, deeper=deeper)
        out.append((data, depth, znest.expected(data, depth)))
    data = znest.near_sample(r)   # one changed byte: the outer stream is recorded with a diff
    out.append((data, 1, znest.expected(data, 1)))
    return out


# ---- the model -----------------------------------------------------------------------------------------------
def test_model_round_trip(files):
    for (data, depth, f), heads in zip(files, (1, 2, 3, 1)):
        lv = znest.levels(f)
        assert f[:4] == b"ATN\1" and len(lv) == heads + 1 and all(x[:4] == b"ATZ\1" for x in lv)
        assert znest.reconstruct(f) == (0, data)
        outer, inner = znest.split(f)
        assert znest.join(outer, inner) == f
        rc, P = znest.reconstruct(inner)
        flat = znest.unstrip(outer, P)
        assert rc == 0 and znest.strip(flat) == (outer, P)
        assert flat == _libs.ora_precompress(data)[1] and znest.origlen(f) == len(data)
    diffs = znest.parse_stripped(znest.split(files[3][2])[0])[2]
    assert [d["nd"] for d in diffs] == [1]
    # no stream inside the streams, no stream at all, depth 0: the flat file
    r = random.Random(5)
    plain = _libs.text(r, 500) + znest.z(_libs.text(r, 3000), 6) + _libs.text(r, 100)
    for data in (plain, _libs.text(r, 2000)):
        assert znest.expected(data, 2) == _libs.ora_precompress(data)[1]
    assert znest.expected(files[0][0], 0) == _libs.ora_precompress(files[0][0])[1]


# ---- the reader ----------------------------------------------------------------------------------------------
def model_levels(f):
    """nest_check's parse lines from the model."""
    out, pos = [], 0
    lv = znest.levels(f)
    for k, x in enumerate(lv):
        stripped = k + 1 < len(lv)
        pos += znest.HEADER if stripped else 0
        rows, at = [], 28
        if stripped:
            ver, origlen, descs, _ = znest.parse_stripped(x)
        else:
            ver, origlen, descs, _ = atzfile.parse(x)
        for d in descs:
            ipos = d["ipos"] if stripped else at + 35 + (8 + 9 * d["nd"] if d["nd"] else 0)
            rows.append([d["off"], d["cl"], d["il"], d["c"], d["w"], d["m"], d["nd"], d["first_diff"] if d["nd"] else 0,
                         len(d["pieces"]) if d["pieces"] else 0, ipos])
            at += len(d["raw"])
        out.append([pos, len(x), ver, origlen, len(descs), int(stripped), rows])
        pos += len(x)
    return out


def level_outputs(f):
    """Each stream's deflate as the reference's reader runs it, innermost level first."""
    lv = znest.levels(f)
    outs, P = [], None
    for k in range(len(lv) - 1, -1, -1):
        flat = lv[k] if P is None else znest.unstrip(lv[k], P)
        for d, pay in zip(atzfile.parse(flat)[2], znest.payloads(flat)):
            outs.append(_libs.ora_deflate(pay, d["c"], d["w"], d["m"])[0])
        rc, P = _libs.ora_reconstruct(flat)
        assert rc == 0
    return outs


def test_accepted_files_agree_with_the_model_and_rebuild(nc, files):
    fs = [f for _, _, f in files]
    for f, (rc, lv) in zip(fs, nc.parse(fs)):
        assert rc == 0 and lv == model_levels(f)
    for (data, _, _), (rc, back) in zip(files, nc.rebuild([(f, level_outputs(f)) for f in fs])):
        assert rc == 0 and back == data
    # a flat file is one level
    flat = _libs.ora_precompress(files[0][0])[1]
    (rc, lv), = nc.parse([flat])
    assert rc == 0 and lv == model_levels(flat)
    assert nc.rebuild([(flat, level_outputs(flat))]) == [(0, files[0][0])]


def test_stripped_stitched_outer_rebuilds(nc):
    """An ATZ4 outer whose one descriptor is stitched and carries diffs: its piece list directly follows its diff list."""
    s, origlen, residue, out, _ = stitched_file((5, 0, 5), 0, 21)
    flat = build_atz(4, origlen, [s], residue)
    outer, P = znest.strip(flat)
    assert P == s["payload"]
    inner = b"ATZ\1" + struct.pack("<QQQ", 28 + len(P), len(P), 0) + P   # P's file: no stream inside
    f = znest.join(outer, inner)
    (rc, lv), = nc.parse([f])
    assert rc == 0 and lv == model_levels(f) and lv[0][6][0][8] == 3
    assert nc.rebuild([(f, [out])]) == [(0, model_rebuild(origlen, [s], [out], residue))]


def test_empty_payload_beside_others(nc):
    """A stripped descriptor of infl_len 0 between two others: it takes no byte of P and the next one starts where it does."""
    r = random.Random(31)
    pay = [r.randbytes(40), b"", r.randbytes(25)]
    streams = [dict(off=2 + 20 * k, cl=10, payload=p, c=6, w=15, m=8) for k, p in enumerate(pay)]
    flat = build_atz(1, 70, streams, r.randbytes(40))
    outer, P = znest.strip(flat)
    inner = b"ATZ\1" + struct.pack("<QQQ", 28 + len(P), len(P), 0) + P
    f = znest.join(outer, inner)
    (rc, lv), = nc.parse([f])
    assert rc == 0 and lv == model_levels(f) and [d[9] for d in lv[0][6]] == [0, 40, 40]
    outs = [r.randbytes(10) for _ in pay]
    orig = model_rebuild(70, streams, outs, flat[-40:])
    assert nc.rebuild([(f, outs)]) == [(0, orig)]
    rc, atn, P2 = nc.write(table_of(flat), orig, inner)
    assert rc == 0 and P2 == P and znest.split(atn)[0] == outer


# ---- the writer ----------------------------------------------------------------------------------------------
def test_stripped_writer_then_unstrip_is_the_flat_file(nc, files):
    for data, depth, f in files:
        flat = _libs.ora_precompress(data)[1]
        outer, inner = znest.split(f)
        rc, atn, P = nc.write(table_of(flat), data, inner)
        assert rc == 0 and atn == f
        assert P == znest.strip(flat)[1]
        assert znest.unstrip(znest.split(atn)[0], P) == flat
    s, origlen, residue, out, _ = stitched_file((1, 7, 1), 0, 7)
    flat = build_atz(4, origlen, [s], residue)
    inner = random.Random(8).randbytes(100)   # (the writer does not look at the inner file)
    rc, atn, P = nc.write(table_of(flat), model_rebuild(origlen, [s], [out], residue), inner)
    assert rc == 0 and atn == znest.join(znest.strip(flat)[0], inner) and P == s["payload"]


def test_writer_cuts_long_copies(nc):
    """An inner file and a payload longer than the split size go out as several segments (nest_check requires it)."""
    r = random.Random(3)
    pay = r.randbytes(300) * 4000   # 1.2 MB
    s = dict(off=3, cl=50, payload=pay, c=6, w=15, m=8)
    flat = build_atz(1, 60, [s], r.randbytes(10))
    inner = r.randbytes(500) * 5000   # 2.5 MB
    rc, atn, P = nc.write(table_of(flat), bytes(60), inner)
    assert rc == 0 and P == pay and znest.split(atn)[1] == inner


# ---- refusals ------------------------------------------------------------------------------------------------
def put8(b, at, v):
    b = bytearray(b)
    b[at:at + 8] = struct.pack("<Q", v & (2 ** 64 - 1))
    return bytes(b)


def wrap(inner, il=None):
    """One more level around `inner`: a stripped outer with one descriptor whose payload is the whole of inner's original."""
    il = znest.origlen(inner) if il is None else il
    outer = b"ATZ\1" + struct.pack("<QQQ", 28 + 35, 10, 1) + struct.pack("<QQQBBBQ", 0, 10, il, 6, 15, 8, 0)
    return znest.join(outer, inner)


def refusals(f):
    """{name: a file every reader must refuse}, made from the accepted nested file f (one "ATN" header)."""
    total, outer_len = struct.unpack_from("<QQ", f, 4)
    outer, inner = znest.split(f)
    at_inner = znest.HEADER + outer_len
    bad = {}
    # truncation at every structural boundary, with the length field left and with it set to the new size
    first = znest.parse_stripped(outer)[2][0]
    cuts = {"magic": 4, "length": 12, "header": 20, "outer_header": 20 + 28, "outer_desc": 20 + 28 + 35,
            "outer_desc_end": 20 + 28 + len(first["raw"]), "outer_end": at_inner, "inner_magic": at_inner + 4,
            "inner_header": at_inner + 28, "inner_desc": at_inner + 28 + 35, "last_byte": total - 1}
    for name, n in cuts.items():
        bad["cut_" + name] = f[:n]
        if n >= 12:
            bad["cut_fixed_" + name] = put8(f[:n], 4, n)
    # lengths off by one
    for name, at, v in (("whole", 4, total), ("outer_len", 12, outer_len), ("outer_own", 20 + 4, outer_len),
                        ("inner_own", at_inner + 4, len(inner))):
        bad[name + "_plus"] = put8(f, at, v + 1)
        bad[name + "_minus"] = put8(f, at, v - 1)
    bad["whole_plus_byte"] = put8(f + b"\0", 4, total + 1)   # (consistent: the inner's own length then disagrees)
    # the inner's original one byte longer than the payloads: a valid inner file, one more residue byte
    longer = put8(put8(inner, 4, len(inner) + 1), 12, znest.origlen(inner) + 1) + b"x"
    bad["inner_origlen"] = znest.join(outer, longer)
    assert znest.reconstruct(longer)[0] == 0
    # an outer without a descriptor (its payloads, none, are the empty file's original)
    empty = b"ATZ\1" + struct.pack("<QQQ", 28, 0, 0)
    bad["outer_no_descriptor"] = znest.join(b"ATZ\1" + struct.pack("<QQQ", 28 + 5, 5, 0) + b"hello", empty)
    bad["version_0"] = b"ATN\0" + f[4:]
    bad["version_2"] = b"ATN\2" + f[4:]
    # a stripped descriptor whose diff list or piece list runs past the outer
    one = struct.pack("<QQQBBBQ", 0, 10, znest.origlen(inner), 6, 15, 8, 3) + struct.pack("<Q", 0) + bytes(8 * 3 + 2)
    bad["diffs_past_outer"] = znest.join(b"ATZ\1" + struct.pack("<QQQ", 28 + len(one), 10, 1) + one, inner)
    one = struct.pack("<QQQBBBQ", 0, 10, znest.origlen(inner), 0x86, 15, 8, 0) + struct.pack("<III", 3, 5, 4)
    bad["pieces_past_outer"] = znest.join(b"ATZ\4" + struct.pack("<QQQ", 28 + len(one), 22 + 12, 1) + one, inner)
    # a payload past P
    bad["payload_past_p"] = wrap(inner, znest.origlen(inner) + 1)
    return bad


def deep(f, heads):
    while len(znest.levels(f)) - 1 < heads:
        f = wrap(f)
    return f


def test_refusals(nc, files):
    f = files[0][2]
    bad = refusals(f)
    names = sorted(bad)
    res = nc.parse([bad[k] for k in names])
    assert {k: rc for k, (rc, _) in zip(names, res) if rc != E_FORMAT} == {}
    # the same shapes, valid: the fabricated wrapper itself and eight headers are read, nine are not
    ok = [wrap(f), deep(f, 8), deep(f, 9)]
    res = nc.parse(ok)
    assert [rc for rc, _ in res] == [0, 0, E_FORMAT]
    assert res[0][1] == model_levels(ok[0]) and len(res[1][1]) == 9
    # a descriptor byte no version knows, in the outer and in the inner: the reference's abort
    at = znest.HEADER + 28 + 24
    res = nc.parse([f[:at] + b"\x0a" + f[at + 1:]])
    assert res[0][0] == E_REF_ABORT


def test_mutants_refused_or_parsed_as_the_model_parses_them(nc, files):
    r = random.Random(909)
    mutants = []
    for _, _, good in files:
        outer_len = struct.unpack_from("<Q", good, 12)[0]
        for _ in range(60):
            b = bytearray(good)
            if r.random() < 0.15:
                b = b[:r.randrange(20, len(b))]
                b[4:12] = struct.pack("<Q", len(b))   # keep the whole length consistent
            else:
                # past the magic; mostly in the headers and first descriptors of the two files
                where = r.random()
                lo, hi = (4, 20 + 28 + 43 * 2) if where < 0.5 else (20 + outer_len, 20 + outer_len + 28 + 43 * 2) \
                    if where < 0.85 else (4, len(b))
                at = r.randrange(lo, min(hi, len(b)))
                b[at] = r.randrange(256) if r.random() < 0.5 else b[at] ^ (1 << r.randrange(8))
            mutants.append(bytes(b))
    parsed = nc.parse(mutants)   # (never a sanitizer report: Check.run requires a clean exit)
    ok = [(b, lv) for b, (rc, lv) in zip(mutants, parsed) if rc == 0]
    for b, lv in ok:
        assert lv == model_levels(b)
    assert 0 < len(ok) < len(mutants)
    # every accepted one runs through both levels' plans with arbitrary outputs: refused there or rebuilt in bounds
    jobs = [(b, [r.randbytes(d[1] + r.randrange(-2, 3) if d[1] > 2 else d[1]) for L in reversed(lv) for d in L[6]])
            for b, lv in ok]
    for rc, back in nc.rebuild(jobs):
        assert rc in (0, E_REF_ABORT, E_FORMAT)


# ---- the switch ----------------------------------------------------------------------------------------------
def test_depth_parser():
    import antiz_amd
    assert [antiz_amd.nest_depth(t) for t in ("", "0", "1", "4", "04", 0, 3)] == [0, 0, 1, 4, 4, 0, 3]
    for t in ("5", "-1", "x", "1.0", " 1", "1 ", "+1", "0x1", "١", 5, -1, True, "99999999999999999999"):
        with pytest.raises(ValueError):
            antiz_amd.nest_depth(t)
