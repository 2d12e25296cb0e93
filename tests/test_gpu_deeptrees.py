"""Trees deeper than zlib's length limit (tests/deeptrees.py) on the MI355X: k_deflate's build_tree through
its length-limit fix-up (Z/trees.c:531-564) on all three trees, from the register heap and from the LDS heap,
byte for byte against zlib 1.2.8; k_inflate on the 15-bit and 7-bit codes such streams carry; and the same
streams through precompress / reconstruct, with the default caps and with caps that defer and retry.

tests/golden/deeptrees.json (make_deeptrees.py) holds the real zlib 1.2.8's stream hash and inflate results of
every item; tests/test_oracle.py shows on the CPU that the items reach the paths they are named for.  The
Z_RLE and Z_HUFFMAN_ONLY streams come from oracle/_ref/libz128.so (tests/zstrat.py); without it these tests
fail, they do not skip.
"""
import hashlib
import os
import random
import subprocess
import sys

import pytest

import _libs
import deeptrees as DT
import zstrat

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (1 << zstrat.Z_HUFFMAN_ONLY) | (1 << zstrat.Z_RLE)


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
    with atz.Context(device=0) as c:
        yield c


@pytest.fixture(scope="module")
def streams():
    """zlib 1.2.8's stream of every item (the oracle's, or zstrat's), checked against the fixture."""
    fx = DT.fixture()["items"]
    out = {}
    for it in DT.items():
        s = DT.reference_stream(it)
        assert [len(s), sha(s)] == fx[it.name]["deflate"], it.name
        out[it.name] = s
    return out


def first_diff(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


# ---- 1. exact deflate -------------------------------------------------------------------------------
def test_exact_deflate(ctx, streams):
    """One batch over every item, one wavefront a trial: each output is zlib 1.2.8's (the fixture's hash), and
    the default-strategy ones are the oracle's byte for byte."""
    fx = DT.fixture()["items"]
    buf, batch = bytearray(), []
    for it in DT.items():
        batch.append((len(buf), len(it.data), it.level, it.window, it.memlevel, it.strategy))
        buf += it.data
        buf += b"\0" * (-len(buf) % 16)
    got = ctx.deflate_batch(bytes(buf), batch)
    bad = []
    for it, g in zip(DT.items(), got):
        want = streams[it.name]
        if [len(g), sha(g)] != fx[it.name]["deflate"] or (it.strategy == DT.Z_DEFAULT and g != want):
            bad.append((it.name, "first difference at byte %d" % first_diff(g, want), len(g), len(want)))
    print("deep trees: %d items, %d differ" % (len(batch), len(bad)))
    assert not bad, bad[:20]


# ---- 2. inflate -------------------------------------------------------------------------------------
def test_inflate_long_codes(ctx, streams):
    """k_inflate past its 6-bit root table (15-bit literal/length and distance codes, 7-bit code-length codes),
    on whole streams and on streams cut 1, 2, 5 and 9 bytes short, from unaligned starts: zlib 1.2.8's
    (status, consumed, produced)."""
    fx = DT.fixture()["items"]
    buf, ranges, want = bytearray(), [], []
    for k, it in enumerate(DT.items()):
        s = streams[it.name]
        assert len(fx[it.name]["inflate"]) == len(DT.cuts_of(s))
        for (cut, part), triple in zip(DT.cuts_of(s), fx[it.name]["inflate"]):
            buf += bytes((k + cut) % 3)   # unaligned starts
            ranges.append((len(buf), len(part)))
            buf += part
            want.append((it.name, cut, tuple(triple)))
    got = ctx.inflate_batch(bytes(buf), ranges)
    bad = [(name, cut, tuple(g), w) for g, (name, cut, w) in zip(got, want) if tuple(g) != w]
    assert not bad, bad[:10]
    assert sum(w[0] == 0 for _, _, w in want) == len(DT.items())   # every whole stream ends; no cut one does


# ---- 3. end to end ----------------------------------------------------------------------------------
def build_file(names, streams, seed):
    """-> (file bytes, [(offset, item name)]): the named items' streams with 20-400 bytes of text between them."""
    r = random.Random(seed)
    parts, recs, pos = [], [], 0
    for name in names:
        fill = _libs.text(random.Random(r.randrange(1 << 30)), r.randrange(20, 400))
        parts.append(fill)
        pos += len(fill)
        recs.append((pos, name))
        parts.append(streams[name])
        pos += len(streams[name])
    parts.append(_libs.text(random.Random(9), 333))
    return b"".join(parts), recs


def e2e_names():
    """About 30 default-strategy items the reference's scanner sees (windowBits 10 and up, more than 16 bytes):
    each tree's fix-up, from both heaps, and the ties."""
    by = {it.name: it for it in DT.default_items()}
    pick = [n for n in by if n.startswith(("l_deep", "d_chain", "edge_tie"))]
    pick += [n for n in by if n.startswith("bl_deep") and by[n].window >= 12 and len(by[n].data) <= 20000][:6]
    assert 28 <= len(pick) <= 36 and all(by[n].window >= 10 for n in pick), len(pick)
    return pick


@pytest.fixture(scope="module")
def e2e(streams):
    data, recs = build_file(e2e_names(), streams, seed=5)
    assert len(data) < 524288   # one chunk of the scan: no stream lies across a chunk's end
    rc, ref, stats = _libs.ora_precompress(data)
    assert rc == 0 and ref[:4] == b"ATZ\1"
    return dict(data=data, recs=recs, ref=ref, ora=stats)


def test_end_to_end(atz, e2e):
    """precompress with default options writes the oracle's ATZ1; every stream is recorded with no diffs (its
    parameters are in the reference's lists: every level and memLevel at the header's window); reconstruct
    returns the file."""
    import nearmiss
    by = {s["offset"]: s for s in e2e["ora"]["streams"]}
    for pos, name in e2e["recs"]:
        assert by[pos]["recomp"] == 1 and by[pos]["n_diff"] == 0, name
    with atz.Context(device=0) as c:
        got, st = c.precompress(e2e["data"])
        first = first_diff(got, e2e["ref"])
        assert got == e2e["ref"], "ATZ1 differs from the oracle's at byte %d" % first
        table = {e["offset"]: e for e in nearmiss.parse_atz1(got)}
        for pos, name in e2e["recs"]:
            assert table[pos]["n_diff"] == 0 and table[pos]["comp_len"] == by[pos]["comp_len"], name
        assert c.reconstruct(got) == e2e["data"]


CAPS = r"""
import hashlib, sys
sys.path.insert(0, %r)
import antiz_amd
data = open(sys.argv[1], "rb").read()
with antiz_amd.Context(device=0) as c:
    out, st = c.precompress(data)
    back = c.reconstruct(out)
print(int(back == data))
print(hashlib.sha256(out).hexdigest())
""" % ROOT


def test_end_to_end_small_caps(e2e, tmp_path):
    """ATZ_CAP_DIV=4096 (read once per process, so a process of its own): the deferred and retry paths build
    the same trees, so the same ATZ1."""
    path = str(tmp_path / "f.bin")
    with open(path, "wb") as f:
        f.write(e2e["data"])
    r = subprocess.run([sys.executable, "-c", CAPS, path], env=dict(os.environ, ATZ_CAP_DIV="4096"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2] == "1"
    assert lines[-1] == sha(e2e["ref"])


# ---- 4. strategies end to end -------------------------------------------------------------------------
def test_strategy_streams_end_to_end(atz, streams):
    """The huff_fib and rle_fib streams in one file: with strategies off the ATZ1 is the oracle's; under
    strategies ("huffman", "rle") every stream the reference walk leaves alone is recorded exactly in the ATZ2,
    with the parameters of the Python model of the rule (zstrat.rule); the file round-trips."""
    from test_gpu_strategy import parse_atz
    by_name = {it.name: it for it in DT.items()}
    data, recs = build_file([it.name for it in DT.items() if it.strategy], streams, seed=6)
    rc, ref, stats = _libs.ora_precompress(data)
    assert rc == 0
    ora = {s["offset"]: s for s in stats["streams"]}
    with atz.Context(device=0) as c:
        off, _ = c.precompress(data)
    assert off[:4] == b"ATZ\1" and off == ref, "ATZ1 differs from the oracle's at byte %d" % first_diff(off, ref)
    with atz.Context(device=0, strategies=("huffman", "rle")) as c:
        on, _ = c.precompress(data)
        assert c.reconstruct(on) == data
    ver, origlen, entries = parse_atz(on)
    assert on[:4] == b"ATZ\2" and ver == 2 and origlen == len(data)
    on_by = {d["off"]: d for d in entries}
    off_by = {d["off"]: d for d in parse_atz(off)[2]}
    n_ext = 0
    for pos, name in recs:
        it, stream = by_name[name], streams[name]
        if ora[pos]["recomp"]:    # the reference walk's own (a default trial within recomp_tresh): untouched
            assert on_by[pos]["raw"] == off_by[pos]["raw"], name
            continue
        d = on_by[pos]
        assert d["nd"] == 0 and d["cl"] == len(stream) and d["il"] == len(it.data), name
        want = zstrat.rule(stream, it.data, MASK)
        assert want["diff_pos"] == [], name
        assert (d["c"] >> 4, d["c"] & 15, d["w"], d["m"]) == (want["strategy"], want["level"], want["window"], want["memlevel"]), name
        n_ext += 1
    print("recorded by the extension: %d of %d" % (n_ext, len(recs)))
    assert n_ext >= 20 and len(entries) == len(off_by) + n_ext
