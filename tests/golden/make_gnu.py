#!/usr/bin/env python3
"""Writes tests/golden/gnu.json and gnu.bin: raw deflate bodies written by the local `gzip` and `zip` binaries (GNU's
deflater: DESIGN.md s7.5) on seeded inputs.  Run by hand where both are installed; no test runs it.

Each entry of gnu.json stores its class, level, block symbol counts and where its body lies in gnu.bin (at, len);
the input is the body's inflation.  Classes:
  a  under 4 096 symbols: byte-identical to zlib's raw deflate at memLevel 8
  b  the block heuristic is evaluated at 4 096 symbols and passes / fails by a small margin ("pass" / "fail")
  c  it fires at one multiple of 4 096 and not at the next one evaluated
  d  levels 1 and 2 (never evaluated) and a level-6 input on which it never fires: the 32 767-symbol flush
  e  a stored block among dynamic ones
  g  "tail": the last match differs from zlib's (GNU compares past the end of input; not modelled)
and, beside the entries, one archive made by `zip` with three members at three levels (class f).
The script asserts that every a-f body has zlib's token stream and the model's blocks, and that g's have not.

usage: python tests/golden/make_gnu.py   (needs oracle/_ref/libz128.so: __graft_entry__.build())"""
import json
import os
import random
import struct
import subprocess
import sys
import tempfile
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zgnu  # noqa: E402
import zraw  # noqa: E402


def gzip_body(data, level):
    """the raw deflate body of `gzip -level -n` on data"""
    r = subprocess.run(["gzip", "-%d" % level, "-n", "-c"], input=data, stdout=subprocess.PIPE, check=True)
    g = r.stdout
    assert g[:3] == b"\x1f\x8b\x08" and g[3] == 0
    return g[10:-8]


def zlib_tokens(data, level):
    blocks, out, _ = zgnu.tokenize(zraw.raw_deflate(data, level, 8))
    assert out == data
    return blocks


def tokens_of(body, data):
    blocks, out, used = zgnu.tokenize(body)
    assert out == data and used == len(body)
    return blocks


# ---- inputs --------------------------------------------------------------------------------------------
def words(r, n, vocab=400):
    v = [bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(r.randint(2, 9))) for _ in range(vocab)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(v) + (b" " if r.random() < 0.9 else b".\n")
    return bytes(out[:n])


def lits_and_copies(r, nlit, ncopy, lo, hi, alphabet=256, bump=0):
    """random bytes (literals) with ncopy copies of lo..hi earlier bytes spread among them; the first |bump|
    copies are one byte longer (bump > 0) or shorter"""
    out = bytearray(r.randrange(alphabet) for _ in range(64))
    per = max(1, nlit // max(ncopy, 1))
    for i in range(ncopy):
        out += bytes(r.randrange(alphabet) for _ in range(r.randint(per - 1, per + 1)))
        ln = r.randint(lo, hi) + (0 if i >= abs(bump) else 1 if bump > 0 else -1)
        at = r.randrange(0, len(out) - ln)
        out += out[at:at + ln]
    return bytes(out)


def unique_trigrams(r, n, before):
    """before + n random bytes none of which ends a trigram seen earlier: each of them parses to a literal"""
    out = bytearray(before)
    seen = {bytes(out[i:i + 3]) for i in range(len(out) - 2)}
    while len(out) < len(before) + n:
        t = bytes(out[-2:]) + bytes([r.randrange(256)])
        if t in seen:
            continue
        seen.add(t)
        out.append(t[2])
    return bytes(out)


def level_gadgets(r):
    """A few hundred bytes on which neighbouring levels part ways, so that a body names its level: a match of 17
    at p with one of 30 at p + 1 (max_lazy 16 at level 6, more from 7 on), a match of 5 with one of 12 behind it
    (max_lazy 4 at level 4), and a recent match of 9 before an older one of 20 (nice_length 8 at level 1, 16 at 2)."""
    rb = lambda n: bytes(r.randrange(256) for _ in range(n))
    out = bytearray()
    for short, long_ in ((16, 30), (4, 12)):
        w, c = rb(long_), rb(1)
        out += rb(9) + c + w[:short] + bytes([w[short] ^ 1]) + rb(9) + bytes([c[0] ^ 1]) + w + rb(9) + c + w + rb(5)
    for short, long_ in ((9, 20), (17, 26)):   # (nice_length 16 at level 2, 32 at level 3)
        w = rb(long_)
        out += rb(9) + w + rb(9) + w[:short] + bytes([w[short] ^ 1]) + rb(9) + w + rb(5)
    return bytes(out)


def hash_gadget(r, chain):
    """A match of 12 whose trigram has `chain` younger neighbours in the 15-bit hash of memLevel 8, (c1 << 10 ^ c2
    << 5 ^ c3) & 0x7fff, that the 16-bit hash of memLevel 9 (shifts of 6) keeps apart: with a budget of `chain`
    nodes only memLevel 9's walk reaches it."""
    rb = lambda n: bytes(r.randrange(1, 256) for _ in range(n))
    w = rb(12)
    near = bytes([w[0], w[1] ^ 1, w[2] ^ 32])
    return rb(7) + w + rb(7) + b"".join(near + rb(3) for _ in range(chain)) + rb(7) + w + rb(7)


def ab_runs(r, nruns, k):
    """nruns runs (a b) * k, no pair of bytes used twice in either order: two literals and one match of distance 2
    each, whatever the level"""
    pairs = [(a, b) for a in range(256) for b in range(a + 1, 256)]
    r.shuffle(pairs)
    return b"".join(bytes(pairs[i]) * k for i in range(nruns))


def names_its_level(data, level, body, hint=0):
    """no level tried before `level` in the hint's order gives the same body"""
    order = [lv for lv in zgnu.LEVELS[hint] if lv]
    return all(gzip_body(data, lv) != body for lv in order[:order.index(level)])


# ---- checks shared by every a-f entry -----------------------------------------------------------------------
def check_entry(data, level, body):
    """zlib's tokens, the model's blocks; -> (symbol counts, trace of the heuristic)"""
    blocks = tokens_of(body, data)
    toks = zgnu.flat_tokens(blocks, data)
    assert toks == zgnu.flat_tokens(zlib_tokens(data, level), data), "not zlib's token stream"
    trace = []
    counts = zgnu.gnu_blocks(toks, level, trace)
    assert counts == zgnu.symbol_counts(blocks), (counts, zgnu.symbol_counts(blocks))
    return counts, trace


BLOB = bytearray()   # gnu.bin: the bodies and the archive, one after the other


def stored(b):
    BLOB.extend(b)
    return {"at": len(BLOB) - len(b), "len": len(b)}


def entry(cls, level, body, note, counts):
    return dict({"class": cls, "level": level, "note": note, "blocks": counts}, **stored(body))


def margin(t):   # of one evaluation (last_lit, last_dist, out, in): > 0 passes by that much, <= 0 fails
    return t[3] // 2 - t[2]


def main():
    entries = []
    ver = {"gzip": subprocess.run(["gzip", "--version"], stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()[0],
           "zip": [l for l in subprocess.run(["zip", "-v"], stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
                   if l.startswith("This is Zip")][0]}
    # a
    for level in (1, 6, 9):
        data = words(random.Random(100 + level), 3000)
        body = gzip_body(data, level)
        counts, _ = check_entry(data, level, body)
        assert sum(counts) < 4096 and body == zraw.raw_deflate(data, level, 8)
        entries.append(entry("a", level, body, "small", counts))
    # b: one evaluation at 4 096 symbols with few matches.  The margin in / 2 - out moves by about half a byte per
    # copy made one byte longer, so each seed is steered to a margin of 1 (passes) and of 0 or -1 (fails)
    for level in (3, 4, 6, 9):
        found = {}
        for kind, want in (("pass", 1), ("fail", 0)):
            for seed in range(40):
                bump = 0
                for _ in range(12):
                    r = random.Random(seed * 10 + level)
                    data = lits_and_copies(r, 3150, 1000, 6 if level < 4 else 5, 14 if level < 4 else 13, bump=bump) + \
                        bytes(r.randrange(256) for _ in range(300))
                    if kind == "fail":   # ... and fires at 8 192, or the one block would be zlib's at memLevel 8 too
                        data += ab_runs(r, 1500, 20)   # (three symbols to 40 bytes, cheap ones)
                    data += level_gadgets(r)
                    body = gzip_body(data, level)
                    trace = []
                    try:
                        zgnu.gnu_blocks(zgnu.flat_tokens(tokens_of(body, data), data), level, trace)
                    except AssertionError:   # a stored final block with a repeated trigram: another seed
                        break
                    assert len(trace) == (1 if kind == "pass" else 2) and trace[0][1] < trace[0][0] // 2
                    mg = margin(trace[0])
                    if (0 < mg <= 2) if kind == "pass" else (-2 <= mg <= 0):
                        counts, _ = check_entry(data, level, body)
                        assert counts[0] == (4096 if kind == "pass" else 8192)
                        assert all(body != zraw.raw_deflate(data, level, m) for m in (8, 9))
                        assert names_its_level(data, level, body)
                        found[kind] = entry("b", level, body, "%s: out %d, in/2 %d" % (kind, trace[0][2], trace[0][3] // 2), counts)
                        break
                    bump = max(-1000, min(1000, bump + 2 * (want - mg)))
                if kind in found:
                    break
        assert len(found) == 2, (level, list(found))
        entries += [found["pass"], found["fail"]]
    # c: fires at 4 096, then a block evaluated at 4 096 and 8 192 without firing, and the converse inside one block
    r = random.Random(7)
    data = lits_and_copies(r, 3100, 1100, 40, 60) + lits_and_copies(r, 8600, 300, 3, 4)
    body = gzip_body(data, 6)
    counts, trace = check_entry(data, 6, body)
    fired = [margin(t) > 0 and t[1] < t[0] // 2 for t in trace]
    assert fired[:3] == [True, False, False] and counts[0] == 4096, (fired, counts)
    assert names_its_level(data, 6, body)
    entries.append(entry("c", 6, body, "fires at the first multiple, not at the next two", counts))
    data = lits_and_copies(r, 4000, 200, 3, 4) + lits_and_copies(r, 3300, 1300, 40, 60)
    body = gzip_body(data, 6)
    counts, trace = check_entry(data, 6, body)
    fired = [margin(t) > 0 and t[1] < t[0] // 2 for t in trace]
    assert fired[:2] == [False, True] and counts[0] == 8192, (fired, counts)
    entries.append(entry("c", 6, body, "not at 4 096, fires at 8 192", counts))
    # d: the 32 767-symbol flush
    for level in (1, 2, 6):
        # runs of 6 bytes are 3 symbols: matches are a third of them, but out stays above in / 2 = the symbol count.
        # The gadgets in front make the body this level's and memLevel 8's alone (else zlib at memLevel 9 writes it too)
        r = random.Random(300 + level)
        data = level_gadgets(r) + hash_gadget(r, {1: 4, 2: 8, 6: 128}[level]) + ab_runs(r, 11300, 3)
        body = gzip_body(data, level)
        counts, trace = check_entry(data, level, body)
        assert counts[0] == 32767 and (level == 6) == bool(trace)
        assert all(body != zraw.raw_deflate(data, level, m) for m in (8, 9))   # (memLevel 9 has these blocks, not this parse)
        assert names_its_level(data, level, body)
        assert not any(margin(t) > 0 and t[1] < t[0] // 2 for t in trace)
        entries.append(entry("d", level, body, "full buffer", counts))
    # e: a stored block between dynamic ones (its bytes hold no repeated trigram: literals alone)
    # (the first part's length is searched so that the heuristic's flush falls at its end: what is left of it
    # would make the next block worth Huffman codes)
    for nlit in range(2900, 3200, 10):
        r = random.Random(11)
        data = unique_trigrams(r, 36000, lits_and_copies(r, nlit, 1000, 40, 60, alphabet=100)) + words(r, 6000)
        body = gzip_body(data, 6)
        blocks = tokens_of(body, data)
        types = [b["btype"] for b in blocks]
        if 0 in types[1:-1] and types[0] == 2 and types[-1] == 2:
            break
    else:
        raise AssertionError("no stored block between dynamic ones")
    counts, _ = check_entry(data, 6, body)
    entries.append(entry("e", 6, body, "block types %s" % types, counts))
    # f: one archive, three members at three levels, made by zip
    members = []
    with tempfile.TemporaryDirectory() as td:
        for k, level in enumerate((3, 6, 9)):
            r = random.Random(500 + level)
            data = lits_and_copies(r, 3100, 1000, 30, 50) + bytes(r.randrange(256) for _ in range(700)) + level_gadgets(r)
            name = "m%d.bin" % k
            with open(os.path.join(td, name), "wb") as f:
                f.write(data)
            os.utime(os.path.join(td, name), (946684800, 946684800))
            subprocess.run(["zip", "-q", "-X", "-%d" % level, "a.zip", name], cwd=td, check=True,
                           env=dict(os.environ, TZ="UTC"))
            members.append((name, level, data))
        with open(os.path.join(td, "a.zip"), "rb") as f:
            zbytes = f.read()
    zmem = []
    for name, level, data in members:
        at = zbytes.find(b"PK\3\4" + b"\x14\0", 0)
        while at >= 0:
            nlen, xlen = struct.unpack_from("<HH", zbytes, at + 26)
            if zbytes[at + 30:at + 30 + nlen] == name.encode():
                break
            at = zbytes.find(b"PK\3\4", at + 1)
        assert at >= 0
        method, = struct.unpack_from("<H", zbytes, at + 8)
        csize, usize = struct.unpack_from("<II", zbytes, at + 18)
        d = at + 30 + nlen + xlen
        assert method == 8 and usize == len(data)
        body = zbytes[d:d + csize]
        assert body == gzip_body(data, level), "zip's deflater is not gzip's"
        counts, _ = check_entry(data, level, body)
        assert counts[0] == 4096 and body != zraw.raw_deflate(data, level, 8)
        lv = (struct.unpack_from("<H", zbytes, at + 6)[0] >> 1) & 3   # the hint zip states: 1 max, 2 or 3 fast
        assert names_its_level(data, level, body, 2 if lv == 1 else 1 if lv else 0)
        zmem.append({"name": name, "level": level, "offset": d, "csize": csize, "blocks": counts})
    # g: the last match differs from zlib's
    tails = []
    for seed in range(4000):
        if len(tails) == 2:
            break
        r = random.Random(9000 + seed)
        key = bytes(r.randrange(97, 123) for _ in range(2))
        k = r.randint(3, 6)
        data = words(r, 1500) + key + b"\0" * (k + r.randint(3, 9)) + words(r, 800) + key + b"\0" * k + b"x" + \
            words(r, 700) + key + b"\0" * k
        body = gzip_body(data, 6)
        bt, zt = zgnu.flat_tokens(tokens_of(body, data), data), zgnu.flat_tokens(zlib_tokens(data, 6), data)
        if bt == zt:
            continue
        same = 0
        while bt[same] == zt[same]:
            same += 1
        assert bt[same][0] >= len(data) - 258
        tails.append(entry("g", 6, body, "tail: tokens differ from position %d of %d" % (bt[same][0], len(data)),
                           zgnu.symbol_counts(tokens_of(body, data))))
    assert len(tails) == 2
    entries += tails
    out = {"what": "raw deflate bodies written by the gzip and zip binaries named in `versions` (tests/golden/make_gnu.py)",
           "versions": ver, "entries": entries,
           "zip": dict({"members": zmem}, **stored(zbytes))}
    path = os.path.join(HERE, "gnu.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    with open(os.path.join(HERE, "gnu.bin"), "wb") as f:
        f.write(BLOB)
    print("wrote", path, os.path.getsize(path), "bytes and gnu.bin,", len(BLOB), "bytes;", len(entries), "entries")
    for e in entries:
        print(e["class"], e["level"], e["len"], e["note"], e["blocks"][:6])


if __name__ == "__main__":
    main()
