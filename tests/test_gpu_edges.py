"""The size-class and window edges (tests/edges.py) on the MI355X: lengths one below, at and one above every
threshold that selects a kernel, an LDS class or a code path -- the k_buckets_sort and k_match_lds classes, the
16-bit bucket kernels, the no-slide and replay limits around MAX_DIST, blocks of lit_bufsize - 1 symbols,
deflate_stored's cuts, k_inflate's far-copy distance, flush size and arena slot -- byte for byte against the real
zlib 1.2.8 and the real reference (tests/golden/edges.json, made by make_edges.py).  tests/test_edges_cpu.py
shows on the CPU that the oracle gives the same and that the inputs reach the edges they are named for.

The Z_FILTERED / Z_RLE / Z_HUFFMAN_ONLY streams come from oracle/_ref/libz128.so (tests/zstrat.py); without it
that test fails, it does not skip.
"""
import functools
import hashlib
import os
import subprocess
import sys

import pytest

import _libs
import edges as E
import zstrat

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def reference(it):
    """zlib 1.2.8's stream of an item, for the report of a failure (the fixture holds its length and hash)."""
    if it.strategy:
        return zstrat.deflate(it.data, it.level, it.window, it.memlevel, it.strategy)
    return _libs.ora_deflate(it.data, it.level, it.window, it.memlevel)[0]


def deflate_items(c, its):
    """One deflate_batch over `its` in this order (a payload that several items share is in the buffer once)."""
    buf, at, batch = bytearray(), {}, []
    for it in its:
        if id(it.data) not in at:
            at[id(it.data)] = len(buf)
            buf += it.data
            buf += bytes(-len(buf) % 16)
        batch.append((at[id(it.data)], len(it.data), it.level, it.window, it.memlevel, it.strategy))
    return c.deflate_batch(bytes(buf), batch)


def check(its, outs, want):
    """want: the fixture's [length, hash] per item.  A failing item is reported with its family, content, length,
    level, window, memLevel, strategy, first differing byte and the two lengths."""
    assert len(its) == len(outs) == len(want)
    bad = [E.describe(it, o, reference(it)) for it, o, w in zip(its, outs, want) if [len(o), E.sha16(o)] != w]
    print("%s: %d items, %d differ" % (its[0].family, len(its), len(bad)))
    assert not bad, "%d differ:\n%s" % (len(bad), "\n".join(bad[:10]))


def family(name, count):
    pos, its = zip(*E.family(name))
    assert len(its) == count
    fx = E.fixture()["deflate"]
    return list(its), [fx[k] for k in pos]


# ---- deflate ----------------------------------------------------------------------------------------
def test_class_edges(atz):
    """D1 under ATZ_BUCKETS_VERIFY=1 (read per call): every k_buckets_sort job is also built by the in-order
    kernels and compared array for array, with its deepest-bucket report -- on streams that are one bucket (zeros)
    at every class edge -- and every output is zlib's."""
    its, want = family("D1", 1620)
    os.environ["ATZ_BUCKETS_VERIFY"] = "1"
    try:
        with atz.Context(device=0) as c:
            outs = deflate_items(c, its)
    finally:
        del os.environ["ATZ_BUCKETS_VERIFY"]
    check(its, outs, want)


def test_window_edges(ctx):
    """D2: lengths around MAX_DIST, wsize + MAX_DIST and two windows at every windowBits, on data whose only
    copy lies at distance MAX_DIST - 1, MAX_DIST and MAX_DIST + 1."""
    its, want = family("D2", E.N_D2)
    check(its, deflate_items(ctx, its), want)


def test_block_ends(ctx):
    """D3: streams of exactly lit_bufsize - 1 literals and their neighbours at every memLevel; level 0 around
    deflate_stored's block size."""
    its, want = family("D3", E.N_D3)
    check(its, deflate_items(ctx, its), want)


def test_neighbours(ctx):
    """D4: A's last match ends at A's last byte, at a multiple of 256, and the next stream of the batch goes on
    with the bytes that match's source goes on with: a match that reads past the stream's end gets longer.  In
    the order A, B and in the order B, A (what follows A then is another pair's B): the same bytes, zlib's."""
    its, want = family("D4", E.N_D4)
    assert all(a.tag.endswith("A") and b.tag.endswith("B") for a, b in zip(its[0::2], its[1::2]))
    fwd = deflate_items(ctx, its)
    swap = [k ^ 1 for k in range(len(its))]
    rev = deflate_items(ctx, [its[k] for k in swap])
    check(its, fwd, want)
    check(its, [rev[k] for k in swap], want)


def test_strategy_edges(ctx):
    """D5: the block-end and window-edge inputs under Z_FILTERED, Z_HUFFMAN_ONLY and Z_RLE at windowBits 9, 12
    and 15, against the reference's zlib run here and against the fixture."""
    its = list(E.strategy_items())
    assert len(its) == E.N_D5
    outs = deflate_items(ctx, its)
    live = [zstrat.deflate(it.data, it.level, it.window, it.memlevel, it.strategy) for it in its]
    check(its, live, E.fixture()["strategy"])
    check(its, outs, E.fixture()["strategy"])
    assert outs == live


# ---- inflate ----------------------------------------------------------------------------------------
def test_inflate_distance_edges(ctx):
    """I1: a copy at distance exactly P for every P in 4020..4110 (k_inflate<4096> serves a copy from HBM exactly
    when the distance is above 4032) and at the ring's, the flush's and the window's sizes; the whole stream,
    the stream and seven more bytes, and three cuts, from unaligned starts: zlib 1.2.8's (status, consumed,
    produced)."""
    fx = E.fixture()["inflate"]
    buf, ranges, want = bytearray(), [], []
    for i, (P, d, (lv, w, m)) in enumerate(E.inflate_payloads()):
        s = _libs.ora_deflate(d, lv, w, m)[0]
        assert [len(s), E.sha16(s)] == fx[i]["stream"], P
        for k, ((tag, part), triple) in enumerate(zip(E.inflate_cases(s, i), fx[i]["cases"])):
            buf += bytes((i + k) % 3)   # unaligned starts
            ranges.append((len(buf), len(part)))
            buf += part
            want.append((P, tag, tuple(triple)))
    assert len(ranges) == 5 * len(E.DIST_PS) == 510
    got = ctx.inflate_batch(bytes(buf), ranges)
    bad = [(P, tag, tuple(g), w) for g, (P, tag, w) in zip(got, want) if tuple(g) != w]
    assert not bad, (len(bad), bad[:10])
    assert sum(w[0] == 0 for _, _, w in want) == 2 * len(E.DIST_PS)


# ---- end to end -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e2e():
    data, recs = E.e2e_file()
    fx = E.fixture()["e2e"]
    assert sha(data) == fx["input_sha256"] and len(recs) == fx["n_streams"]
    out = {"data": data, "recs": recs}
    for name, brute in (("default", 0), ("brute", 1)):
        rc, ref, stats = _libs.ora_precompress(data, brute=brute)
        assert rc == 0 and sha(ref) == fx["atz_sha256"][name]
        out[name] = stats["streams"]
    return out


@pytest.mark.parametrize("name", ["default", "brute"])
def test_end_to_end(atz, name):
    """The I1 streams, streams of every inflated length around the flush, ring, arena-slot and class sizes and
    the neighbour pairs in one file: the scan table, each stream's parameters, ident and decision are the
    oracle's, the ATZ1 is the real reference's, reconstruct restores the file, and the streams past 64 KiB lost
    their arena slot and were inflated again."""
    ora, data = e2e()[name], e2e()["data"]
    with atz.Context(device=0, brute_window=name == "brute") as c:
        recs = c.scan(data)
        assert [r[:4] for r in recs] == [(s["offset"], s["type"], s["comp_len"], s["infl_len"]) for s in ora]
        res, _ = c.sweep()
        got = [(r["clevel"], r["window"], r["memlevel"], r["ident"], r["recomp"]) for r in res]
        exp = [(s["clevel"], s["window"], s["memlevel"], s["ident"], s["recomp"]) for s in ora]
        bad = [(s["offset"], g, e) for s, g, e in zip(ora, got, exp) if g != e]
        assert not bad and len(got) == len(exp), bad[:10]
        out, st = c.precompress(data)
        assert sha(out) == E.fixture()["e2e"]["atz_sha256"][name], st
        assert st["n_inflate_retries"] >= 1, st
        assert c.reconstruct(out) == data


CAPS = r"""
import hashlib, sys
sys.path.insert(0, %r)
import antiz_amd
data = open(sys.argv[1], "rb").read()
for brute in (False, True):
    with antiz_amd.Context(device=0, brute_window=brute) as c:
        out, st = c.precompress(data)
        back = c.reconstruct(out)
    print(int(back == data), hashlib.sha256(out).hexdigest())
""" % ROOT


def test_end_to_end_small_caps(tmp_path):
    """ATZ_CAP_DIV=4096 (read once per process, so a process of its own): deferred rounds, per-round tables and
    unsaved replays on the same file give the same bytes, for both settings."""
    path = str(tmp_path / "edges.bin")
    with open(path, "wb") as f:
        f.write(e2e()["data"])
    r = subprocess.run([sys.executable, "-c", CAPS, path], env=dict(os.environ, ATZ_CAP_DIV="4096"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    fx = E.fixture()["e2e"]["atz_sha256"]
    assert r.stdout.strip().splitlines()[-2:] == ["1 " + fx["default"], "1 " + fx["brute"]]
