"""Opt-in nesting (atz_set_nesting, Context(nest=...), ATZ_NEST) on the GPU: the streams inside the
recorded streams' payloads, precompressed in the same call into a nested file ("ATN" 1).

With no mask on every level is an ATZ1, so the device's nested file is pinned byte for byte to tests/znest.py's, which
is the oracle run level by level, and the oracle rebuilds the original from the device's file on the CPU.  With masks
the levels are compared with what contexts without a depth write for the same bytes."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import sys

import pytest

import _libs
import atzfile
import znest
import zpng
import zraw
import zstrat
from test_gpu_strategy import dev_copy, gradient, hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1


def ctx(**kw):
    import antiz_amd
    return antiz_amd.Context(device=0, **kw)


@pytest.fixture(scope="module")
def case1():
    """One level-6 stream whose payload is text, a level-1 stream, text, a level-9 stream."""
    data = znest.sample(random.Random(101))
    return data, znest.expected(data, 1)


def check(data, depth, want=None, **opts):
    """precompress at `depth` equals the model's file (or `want`); both readers give the data back.  -> the file"""
    want = znest.expected(data, depth, **({"chunksize": opts["chunksize"]} if "chunksize" in opts else {})) \
        if want is None else want
    with ctx(nest=depth, **opts) as c:
        out, st = c.precompress(data)
        assert out == want
        assert st["atz_bytes"] == len(out)
        assert c.reconstruct(out) == data
    assert znest.reconstruct(out) == (0, data)
    return out


# ---- 1 ---------------------------------------------------------------------------------------------------
def test_one_level(case1):
    data, want = case1
    assert want[:4] == b"ATN\1"
    with ctx(nest=1) as c:
        out, st = c.precompress(data)
        assert out == want
        inner = c.nest_stats(1)
        assert inner["n_recomp"] == 2 and inner["file_bytes"] == znest.origlen(znest.split(out)[1])
        assert c.nest_stats(0)["n_recomp"] == st["n_recomp"] == 1
        assert st["atz_bytes"] == len(out) and st["file_bytes"] == len(data)
        assert inner["atz_bytes"] == len(znest.split(out)[1])
        import antiz_amd
        with pytest.raises(antiz_amd.AtzError) as e:
            c.nest_stats(2)
        assert e.value.code == E_ARG
        assert c.reconstruct(out) == data
    assert znest.reconstruct(out) == (0, data)


# ---- 2 ---------------------------------------------------------------------------------------------------
def test_inner_stream_over_two_payloads():
    """Descriptor order, no padding: the halves of an inner stream end one payload and begin the next, with residue
    between the two outer streams in the file; in P they are one stream."""
    r = random.Random(202)
    s = znest.z(_libs.text(r, 4000), 5)
    h = len(s) // 2
    ta, tb = _libs.text(r, 1111), _libs.text(r, 777)
    data = _libs.text(r, 333) + znest.z(ta + s[:h], 6) + b"residue between the two" + znest.z(s[h:] + tb, 6) + _libs.text(r, 99)
    out = check(data, 1)
    outer, inner = znest.split(out)
    assert [d["il"] for d in znest.parse_stripped(outer)[2]] == [len(ta) + h, len(s) - h + len(tb)]
    assert [(d["off"], d["cl"]) for d in atzfile.parse(inner)[2]] == [(len(ta), len(s))]


# ---- 3 ---------------------------------------------------------------------------------------------------
def test_nothing_inside_is_the_flat_file():
    r = random.Random(303)
    plain = _libs.text(r, 500) + znest.z(_libs.text(r, 3000), 6) + _libs.text(r, 100) + znest.z(_libs.text(r, 900), 9)
    for data, streams in ((plain, 2), (_libs.text(r, 5000), 0)):
        with ctx() as c:
            off, _ = c.precompress(data)
        with ctx(nest=2) as c:
            on, st = c.precompress(data)
            assert st["n_recomp"] == streams
        assert on == off and on[:4] == b"ATZ\1" and on == _libs.ora_precompress(data)[1]


# ---- 4 ---------------------------------------------------------------------------------------------------
def test_three_levels_deep():
    data = znest.sample(random.Random(404), deeper=1)
    one, two, four = (check(data, d) for d in (1, 2, 4))
    assert [len(znest.levels(f)) for f in (one, two, four)] == [2, 3, 3]
    assert znest.split(two)[1][:4] == b"ATN\1" and four == two
    with ctx(nest=4) as c:
        c.precompress(data)
        assert [c.nest_stats(k)["n_recomp"] for k in range(4)] == [1, 2, 2, 0]
        import antiz_amd
        with pytest.raises(antiz_amd.AtzError):
            c.nest_stats(4)   # level 3 recorded nothing: no level 4


# ---- 5 ---------------------------------------------------------------------------------------------------
def test_outer_stream_variants():
    r = random.Random(505)
    near = znest.near_sample(r)                       # recorded with one diff, two streams inside
    inside = _libs.text(r, 600) + znest.z(_libs.text(r, 2500), 3) + _libs.text(r, 200)
    rle = zstrat.deflate(inside * 2, 6, 15, 8, zstrat.Z_RLE)   # found, not recorded: contributes nothing
    # (an empty-payload stream, 78 9C 03 00 00 00 00 01: the reference's scan does not list it, so no descriptor of a
    # written file has infl_len 0; the readers' side of that is tests/test_nest_cpu.py's)
    data = near + znest.z(b"", 6) + _libs.text(r, 50) + rle + _libs.text(r, 70) + znest.z(inside, 9) + b"end"
    rc, flat, st = _libs.ora_precompress(data)
    recs = atzfile.parse(flat)[2]
    assert rc == 0 and len(st["streams"]) == 3           # the Z_RLE stream is among the found ones only
    assert [(d["nd"], d["il"]) for d in recs] == [(1, recs[0]["il"]), (0, len(inside))]
    out = check(data, 1)
    outer, inner = znest.split(out)
    descs = znest.parse_stripped(outer)[2]
    assert [(d["nd"], d["il"], d["ipos"]) for d in descs] == [(1, recs[0]["il"], 0), (0, len(inside), recs[0]["il"])]
    assert descs[0]["raw"] == recs[0]["raw"][:35 + 8 + 9]     # the stripped descriptor keeps its diffs
    assert znest.origlen(inner) == recs[0]["il"] + len(inside) and len(atzfile.parse(inner)[2]) == 3


# ---- 6 ---------------------------------------------------------------------------------------------------
def test_small_chunks_with_inner_streams_on_the_seams():
    """chunksize 4096 and P five chunks long.  The reference's scan keeps a stream that crosses a chunk seam only where
    its header's first byte is the chunk's last (its refill repeats that byte, main.cpp:207-216): such streams lie at
    4095 and 8191 of P, one that crosses a seam elsewhere (12100) is lost, as in any file."""
    r = random.Random(606)
    fill = _libs.text(r, 190)
    P = bytearray((fill * 200)[:5 * 4096 + 321])
    placed = []
    for at, lv in ((700, 3), (4095, 6), (8191, 9), (12100, 1), (3 * 4096 + 2000, 5)):
        s = znest.z(_libs.text(r, 700), lv)
        P[at:at + len(s)] = s
        placed.append((at, len(s)))
    outer = znest.z(bytes(P), 6)
    assert 100 + len(outer) < 4096                       # the outer stream lies in the file's first chunk
    data = _libs.text(r, 100) + outer + _libs.text(r, 9000)
    out = check(data, 1, chunksize=4096)
    inner = atzfile.parse(znest.split(out)[1])[2]
    assert [(d["off"], d["cl"]) for d in inner] == placed[:3] + placed[4:]
    with ctx(nest=1, chunksize=4096) as c:
        c.precompress(data)
        assert c.nest_stats(1)["file_bytes"] == len(P) and c.nest_stats(1)["n_recomp"] == 4


# ---- 7 ---------------------------------------------------------------------------------------------------
def by_levels(data, out, **masks):
    """A nested file written under masks, level by level against contexts without a depth: the unstripped outer is the
    flat file of the data, the inner file the flat file of P.  -> (the unstripped outer, P, the inner file)"""
    outer, inner = znest.split(out)
    with ctx(**masks) as c:
        flat, _ = c.precompress(data)
        P = c.reconstruct(inner)
        assert znest.unstrip(outer, P) == flat
        assert c.precompress(P)[0] == inner
        assert c.reconstruct(out) == data
    return flat, P, inner


def test_masks_pass_down_containers():
    r = random.Random(707)
    t = _libs.text(r, 2000)
    entry = zraw.zip_entry(zraw.raw_deflate(t, 6, 8), len(t), name=b"a.txt")
    payload = _libs.text(r, 500) + znest.z(_libs.text(r, 1800), 6) + _libs.text(r, 100) + entry + _libs.text(r, 60)
    data = _libs.text(r, 400) + zraw.gzip_member(zraw.raw_deflate(payload, 6, 8), payload, name=b"p.tar") + _libs.text(r, 90)
    with ctx(nest=1, containers=("zip", "gzip")) as c:
        out, _ = c.precompress(data)
        assert c.nest_stats(1)["n_recomp"] == 2
    assert out[:4] == b"ATN\1"
    flat, P, inner = by_levels(data, out, containers=("zip", "gzip"))
    assert P == payload and flat[:4] == b"ATZ\3" and inner[:4] == b"ATZ\3"
    assert sorted(d["c"] for d in atzfile.parse(inner)[2]) == [0x06, 0x46]
    # the child gets the masks of its parent, no more: with "gzip" alone nothing announces the ZIP entry's body
    with ctx(nest=1, containers="gzip") as c:
        out, _ = c.precompress(data)
    flat, P, inner = by_levels(data, out, containers="gzip")
    assert P == payload and inner[:4] == b"ATZ\1" and [d["c"] for d in atzfile.parse(inner)[2]] == [0x06]


def test_masks_pass_down_stitched_outer():
    r = random.Random(708)
    payload = gradient(31, 5000) + znest.z(_libs.text(r, 2200), 6) + gradient(32, 3000)
    s = zstrat.deflate(payload, 6, 15, 8, zstrat.Z_FILTERED)
    data = _libs.text(r, 300) + zpng.png(s, zpng.split(len(s), 2048))[0] + _libs.text(r, 80)
    masks = dict(stitch="png", strategies="filtered")
    with ctx(nest=1, **masks) as c:
        out, _ = c.precompress(data)
    assert out[:4] == b"ATN\1"
    outer, inner = znest.split(out)
    ver, _, (d,), _ = znest.parse_stripped(outer)
    assert ver == 4 and d["c"] == 0x80 | 0x10 | 6 and d["pieces"] == zpng.split(len(s), 2048) and d["il"] == len(payload)
    assert len(d["raw"]) == 35 + 4 + 4 * len(d["pieces"])    # the piece list directly follows the fixed fields
    flat, P, inner = by_levels(data, out, **masks)
    assert P == payload and inner[:4] == b"ATZ\1" and atzfile.parse(flat)[2][0]["pieces"] == d["pieces"]


# ---- 8 ---------------------------------------------------------------------------------------------------
def test_reader_refuses_what_the_cpu_reader_refuses(case1):
    import antiz_amd
    from test_nest_cpu import refusals, deep, wrap
    data, good = case1
    bad = refusals(good)
    bad["nine_levels"] = deep(good, 9)
    with ctx() as c:   # (a context without a depth reads a nested file)
        assert c.reconstruct(good) == data
        for name in sorted(bad):
            with pytest.raises(antiz_amd.AtzError):
                c.reconstruct(bad[name])
        assert c.reconstruct(good) == data


# ---- 9 ---------------------------------------------------------------------------------------------------
def test_interfaces(case1):
    import antiz_amd
    data, want = case1
    L = antiz_amd.lib()
    with ctx() as c:
        assert L.atz_set_nesting(c.h, 5) == E_ARG and L.atz_set_nesting(c.h, -1) == E_ARG
        assert c.precompress(data)[0] == _libs.ora_precompress(data)[1]   # the refused settings left depth 0
        scanned = c.scan(data)
        swept = c.sweep()
        assert L.atz_set_nesting(c.h, 4) == 0 and L.atz_set_nesting(c.h, 1) == 0
        assert c.scan(data) == scanned and c.sweep() == swept
        # the shard calls refuse a context with a depth
        with dev_copy(data) as d:
            for call in (lambda: c.shard_scan(d, data, 0, 1), lambda: c.shard_sweep(d, data, []),
                         lambda: c.shard_piece(d), lambda: c.shard_assemble(d, len(data), b"", 0, 0, d, len(data))):
                with pytest.raises(antiz_amd.AtzError) as e:
                    call()
                assert e.value.code == E_ARG
            # device entry points
            p, n, st = c.precompress_device(d, data)
            got = C.create_string_buffer(n)
            assert hip().hipMemcpy(got, p, n, 2) == 0   # device to host
            assert got.raw == want and st["atz_bytes"] == n
        with dev_copy(want) as d:
            p, n = c.reconstruct_device(d, want)
            got = C.create_string_buffer(n)
            assert hip().hipMemcpy(got, p, n, 2) == 0
            assert got.raw == data
        # two calls in a row: the second file has no stream inside its stream, the third is the first again
        r = random.Random(909)
        plain = _libs.text(r, 500) + znest.z(_libs.text(r, 3000), 6) + _libs.text(r, 100)
        assert c.precompress(data)[0] == want and c.nest_stats(1)["n_recomp"] == 2
        assert c.precompress(plain)[0] == _libs.ora_precompress(plain)[1] and c.nest_stats(1)["n_recomp"] == 0
        nostream = _libs.text(r, 800)
        assert c.precompress(nostream)[0] == _libs.ora_precompress(nostream)[1]
        with pytest.raises(antiz_amd.AtzError):
            c.nest_stats(1)   # no recorded stream: level 1 did not run
        assert c.precompress(data)[0] == want
    with pytest.raises(ValueError):
        ctx(nest="two")
    with pytest.raises(ValueError):
        ctx(nest=5)


def test_context_reads_the_environment(case1, monkeypatch):
    data, want = case1
    monkeypatch.setenv("ATZ_NEST", "1")
    with ctx() as c:
        assert c.precompress(data)[0] == want
    monkeypatch.setenv("ATZ_NEST", "1x")
    with pytest.raises(ValueError):
        ctx()


# ---- 10 --------------------------------------------------------------------------------------------------
def test_cli(case1, tmp_path):
    import antiz_amd
    data, want = case1
    f = str(tmp_path / "f.bin")
    with open(f, "wb") as fh:
        fh.write(data)
    env = dict(os.environ, ATZ_NEST="1", ATZ_DEVICE="0")
    r = subprocess.run([antiz_amd.CLI_PATH, "-i", f], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    assert "OK! Restoration is bit by bit identical" in r.stdout
    with open(f + ".atz", "rb") as fh:
        assert fh.read() == want
    env.pop("ATZ_NEST")   # any context reads a nested file
    r = subprocess.run([antiz_amd.CLI_PATH, "-r", "-i", f + ".atz", "-o", f + ".back"], env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    with open(f + ".back", "rb") as fh:
        assert fh.read() == data
    r = subprocess.run([antiz_amd.CLI_PATH, "-i", f], env=dict(env, ATZ_NEST="7"), capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 1 and "ATZ_NEST" in r.stderr


# ---- 11 --------------------------------------------------------------------------------------------------
CAPS = r"""
import hashlib, sys
sys.path.insert(0, %r)
import antiz_amd
data = open(sys.argv[1], "rb").read()
with antiz_amd.Context(device=0, nest=1) as c:
    out, st = c.precompress(data)
    back = c.reconstruct(out)
    inner = c.nest_stats(1)["n_recomp"]
print(int(back == data), inner)
print(hashlib.sha256(out).hexdigest())
""" % ROOT


def test_memory_caps_divided_down(case1, tmp_path):
    """Every device-memory cap at 1/4096 (tests/test_gpu_knobs.py): both levels go through the paths past the caps."""
    data, want = case1
    f = str(tmp_path / "f.bin")
    with open(f, "wb") as fh:
        fh.write(data)
    r = subprocess.run([sys.executable, "-c", CAPS, f], env=dict(os.environ, ATZ_CAP_DIV="4096"), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2].split() == ["1", "2"] and lines[-1] == hashlib.sha256(want).hexdigest()
