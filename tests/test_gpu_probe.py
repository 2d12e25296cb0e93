"""The probe extension on the GPU: k_probe_ordered's list against the Python model, position
for position; an anchorless raw body end to end; the walk's parameters and near-miss diffs against the model;
precedence of every record made before; the acceptance limits; the slot-loss path, a cap knob and the errors.

Every expected deflate byte comes from oracle/_ref/libz128.so (zstrat / zraw); the model is tests/zprobe.py.
"""
import hashlib
import os
import random
import subprocess
import sys
import zlib

import pytest

import _libs
import zpng
import zprobe
import zraw
import zstrat
from test_gpu_strategy import dev_copy, padded, parse_atz, rnd, txt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = ("deflate",)


@pytest.fixture(scope="module")
def ctx():
    import antiz_amd
    with antiz_amd.Context(device=0, probe=PROBE) as c:
        yield c


# ---- 1. positions ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noise():
    return rnd(4242, 200000 + 77)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 9, 10, 11, 4095, 4096, 4097, 65535, 65536, 65537, 200077])
def test_positions_in_random_bytes(ctx, noise, n):
    data = noise[-n:] if n else b""
    got = ctx.probe_positions(data)
    assert got == zprobe.positions(data)
    assert got == sorted(set(got))
    if n >= 65535:
        assert len(got) > 20


def test_positions_in_deflate_data(ctx):
    data = zstrat.deflate(txt(11, 800000), 6, -15, 8, 0)[:256 << 10]
    assert len(data) == 256 << 10
    want = zprobe.positions(data)
    assert ctx.probe_positions(data) == want and len(want) > 100


N_PLANT, SEG = 65536 + 77, 36864   # two blocks: the second one's segment starts at SEG


def planted_file(shift, swap):
    """Random bytes with hand-built headers of nc = 4 and nc = 19 whose first byte lies `shift` - 10 bytes from
    a lane's 16-byte load + 16, a wave's 1 KiB, a 4 KiB step and the segment seam between the two blocks."""
    r = random.Random(100 * shift + swap)
    b = bytearray(r.randbytes(N_PLANT))
    spots = []
    for k, seam in enumerate((16 * 51, 16 * 91, 1024 * 5, 1024 * 7, 4096 * 3, 4096 * 5, SEG, 4096 * 12 + 16 * 7)):
        nc = 19 if (k + swap) & 1 else 4
        p = seam - 10 + shift
        b[p:p + zprobe.header_bytes(nc)] = zprobe.header(nc, r, bfinal=k & 1)
        spots.append(p)
    return bytes(b), spots


@pytest.mark.parametrize("swap", [0, 1])
def test_positions_at_the_seams(ctx, swap):
    """shift 0..10: p mod 16 = 6..15 and 0 (a header of 10 bytes ends in the next lane's load), p = 4086..4096 of
    a step, the last bytes of block 0's segment and the first of block 1's."""
    for shift in range(11):
        data, spots = planted_file(shift, swap)
        want = zprobe.positions(data)
        assert set(spots) <= set(want), shift
        assert ctx.probe_positions(data) == want, shift


@pytest.mark.parametrize("nc", [4, 19])
def test_positions_at_the_end_of_the_file(ctx, nc):
    """A header at every p of the file's last 12 bytes: complete ones survive, truncated ones do not."""
    r = random.Random(nc)
    for lead in (300, 4096 - 5, 65536 + 4096 - 7):
        for tail in range(1, 13):
            h = zprobe.header(nc, r)
            data = r.randbytes(lead) + h[:tail] + r.randbytes(max(0, tail - len(h)))
            assert len(data) == lead + tail
            want = zprobe.positions(data)
            assert (lead in want) == (len(h) <= tail)
            assert ctx.probe_positions(data) == want, (lead, tail)


# ---- 2. end to end -----------------------------------------------------------------------------------
def ref_records(data):
    rc, _, stats = _libs.ora_precompress(data)
    assert rc == 0
    return [(s["offset"], s["comp_len"], s["infl_len"], s["type"]) for s in stats["streams"]]


def scan_of(c, data, sweep=False):
    got = [(o, cl, il, ty) for o, ty, cl, il, _ in c.scan(data)]
    res, diffs = c.sweep()
    return (got, res, diffs) if sweep else got


def expected(data):
    """The reference's records and the probe's, as the model merges them."""
    ref = ref_records(data)
    return sorted(ref + zprobe.probe_records(data, [(o, cl) for o, cl, _, _ in ref])), ref


@pytest.fixture(scope="module")
def e2e():
    payload = txt(77, 2000)
    body = zraw.raw_deflate(payload, 6, 8)
    assert (body[0] >> 1) & 3 == 2
    data = rnd(1, 3001) + body + rnd(2, 2222)
    return dict(data=data, at=3001, body=body, payload=payload)


def test_end_to_end_mask_off(e2e, monkeypatch):
    import antiz_amd
    monkeypatch.delenv("ATZ_PROBE", raising=False)
    data = e2e["data"]
    with antiz_amd.Context(device=0) as c:
        plain, _ = c.precompress(data)
    with antiz_amd.Context(device=0, probe=()) as c:
        off, _ = c.precompress(data)
        recs = scan_of(c, data)
    rc, ref, _ = _libs.ora_precompress(data)
    assert rc == 0 and off == plain == ref and off[:4] == b"ATZ\1"
    lo, hi = e2e["at"], e2e["at"] + len(e2e["body"])
    assert not any(o < hi and lo < o + cl for o, cl, _, _ in recs)
    monkeypatch.setenv("ATZ_PROBE", "")
    with antiz_amd.Context(device=0) as c:
        assert c.precompress(data)[0] == plain


def test_end_to_end_mask_on(ctx, e2e, tmp_path, monkeypatch):
    import antiz_amd
    data, at, body, payload = e2e["data"], e2e["at"], e2e["body"], e2e["payload"]
    want, ref = expected(data)
    got, res, diffs = scan_of(ctx, data, sweep=True)
    assert got == want
    mine = [k for k, r in enumerate(got) if r[3] == 24]
    assert [got[k] for k in mine] == [(at, len(body), len(payload), 24)]
    x = res[mine[0]]
    assert (x["recomp"], x["clevel"], x["window"], x["memlevel"], x["ident"], x["n_diff"]) == \
           (1, 0x40 | 6, 15, 8, len(body), 0)
    atz, st = ctx.precompress(data)
    ver, origlen, descs = parse_atz(atz)
    assert atz[:4] == b"ATZ\3" and ver == 3 and origlen == len(data)
    d = {d["off"]: d for d in descs}[at]
    assert (d["c"], d["w"], d["m"], d["cl"], d["il"], d["nd"]) == (antiz_amd.pack_clevel(0, 6, raw=True), 15, 8,
                                                                  len(body), len(payload), 0)
    with antiz_amd.Context(device=0) as c:   # a context without the mask reads the file
        assert c.reconstruct(atz) == data
    assert ctx.reconstruct(atz) == data
    # None reads ATZ_PROBE
    monkeypatch.setenv("ATZ_PROBE", "deflate")
    with antiz_amd.Context(device=0) as c:
        assert c.precompress(data)[0] == atz
    monkeypatch.setenv("ATZ_PROBE", "deflate,brute")
    with pytest.raises(ValueError):
        antiz_amd.Context(device=0)
    monkeypatch.delenv("ATZ_PROBE")
    # the CLI
    f = str(tmp_path / "f")
    with open(f, "wb") as fh:
        fh.write(data)
    env = dict(os.environ, ATZ_PROBE="deflate", ATZ_DEVICE="0")
    r = subprocess.run([antiz_amd.CLI_PATH, "-i", f], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    assert "OK! Restoration is bit by bit identical" in r.stdout
    assert open(f + ".atz", "rb").read() == atz


# ---- 3. levels, near-misses ----------------------------------------------------------------------------
def joined(items, seed=9):
    """-> (file, [offset of each item]) with random filler of 100-400 bytes around the items."""
    r = random.Random(seed)
    parts, at, pos = [], [], 0
    for blob in items:
        fill = r.randbytes(r.randrange(100, 400))
        parts += [fill, blob]
        at.append(pos + len(fill))
        pos += len(fill) + len(blob)
    parts.append(r.randbytes(150))
    return b"".join(parts), at


def test_levels_and_memlevels(ctx):
    params = [(1, 8), (9, 8), (6, 9), (6, 1), (9, 9), (3, 1)]
    payloads = [txt(600 + k, 3000 + 500 * k) for k in range(len(params))]
    bodies = [zraw.raw_deflate(p, lv, m) for p, (lv, m) in zip(payloads, params)]
    data, at = joined(bodies)
    want, _ = expected(data)
    got, res, _ = scan_of(ctx, data, sweep=True)
    assert got == want
    by = {r[0]: k for k, r in enumerate(got)}
    for o, body, payload in zip(at, bodies, payloads):
        assert got[by[o]] == (o, len(body), len(payload), 24)
        w = zprobe.rule(body, payload)
        assert w is not None and w["diff_pos"] == []
        x = res[by[o]]
        assert (x["recomp"], x["clevel"], x["window"], x["memlevel"], x["ident"], x["n_diff"]) == \
               (1, 0x40 | w["level"], 15, w["memlevel"], len(body), 0), o


def test_near_miss_bodies(ctx):
    """Bodies with 1 and with 40 bytes altered past the first block (padding bits inflate ignores)."""
    payload = txt(501, 5000) + rnd(1, 20000) + txt(502, 4000)
    good = zstrat.deflate(payload, 6, 15, 1, 0)
    bodies = [padded(good, alt)[2:-4] for alt in (1, 40)]
    assert all((b[0] >> 1) & 3 == 2 and b[:600] == good[2:602] for b in bodies)
    data, at = joined(bodies, seed=10)
    got, res, diffs = scan_of(ctx, data, sweep=True)
    assert got == expected(data)[0]
    lists = _libs.diff_lists(res, diffs)
    by = {r[0]: k for k, r in enumerate(got)}
    for o, body, alt in zip(at, bodies, (1, 40)):
        k = by[o]
        assert got[k] == (o, len(body), len(payload), 24)
        w = zprobe.rule(body, payload)
        assert w is not None and len(w["diff_pos"]) == alt
        assert (res[k]["recomp"], res[k]["clevel"], res[k]["memlevel"], res[k]["ident"]) == \
               (1, 0x40 | w["level"], w["memlevel"], w["ident"]), o
        assert lists[k][0] == w["diff_pos"] and bytes(lists[k][1]) == w["diff_val"], o


# ---- 4. precedence ---------------------------------------------------------------------------------------
def flushed(wbits, seed=0):
    """A stream with two Z_FULL_FLUSH points: byte-aligned, self-contained dynamic blocks follow them.
    -> (stream, [offset of the block behind each flush point])"""
    z = zlib.compressobj(6, zlib.DEFLATED, wbits)
    out, marks = b"", []
    for k in range(3):
        out += z.compress(zprobe.skewed(seed + k, 1500))
        if k < 2:
            out += z.flush(zlib.Z_FULL_FLUSH)
            marks.append(len(out))
    return out + z.flush(), marks


def test_no_probe_record_inside_a_reference_record(ctx):
    stream, marks = flushed(15)
    data, (at,) = joined([stream], seed=11)
    for m in marks:   # each would be a record of its own
        assert zprobe.probe_ok(data, at + m) and zprobe.accept(data, at + m) is not None
    want, ref = expected(data)
    assert want == ref and (at, len(stream), 4500) in [r[:3] for r in ref]
    assert scan_of(ctx, data) == ref


def test_one_record_for_an_anchorless_flushed_stream(ctx):
    stream, marks = flushed(-15, seed=5)
    data, (at,) = joined([stream], seed=12)
    for m in marks:
        assert zprobe.accept(data, at + m) is not None
    got = scan_of(ctx, data)
    assert got == expected(data)[0]
    assert [r for r in got if r[3] >= 24] == [(at, len(stream), 4500, 24)]


def test_an_anchored_record_wins():
    import antiz_amd
    payload = txt(31, 4000)
    body = zraw.raw_deflate(payload, 6, 8)
    entry = zraw.zip_entry(body, len(payload), name=b"a.txt", flags=zraw.ZIP_HINT_BITS[zraw.HINT_MAX])
    data, (at,) = joined([entry], seed=13)
    at += 30 + 5
    ref = ref_records(data)
    with antiz_amd.Context(device=0, containers=("zip",), probe=PROBE) as c:
        both = scan_of(c, data)
    with antiz_amd.Context(device=0, probe=PROBE) as c:
        alone = scan_of(c, data)
    assert [r for r in both if r[3] >= 24] == [(at, len(body), len(payload), 26)]
    assert [r for r in alone if r[3] >= 24] == [(at, len(body), len(payload), 24)]
    raw = zraw.raw_records(data, 1, [(o, cl) for o, cl, _, _ in ref])
    assert both == sorted(ref + raw + zprobe.probe_records(data, [(o, cl) for o, cl, _, _ in ref + raw]))
    assert alone == expected(data)[0]


def test_no_probe_record_inside_a_stitched_hull():
    import antiz_amd
    stream, marks = flushed(15, seed=20)
    cut = marks[1] - 100   # the second flush point, and all that follows it, lies in the second chunk
    data, first = zpng.png(stream, [cut, len(stream) - cut])
    p = first + marks[1] + zpng.FRAMING
    assert zprobe.probe_ok(data, p) and zprobe.accept(data, p) is not None
    ref = ref_records(data)
    prior = [(o, cl) for o, cl, _, _ in ref]
    with antiz_amd.Context(device=0, probe=PROBE) as c:
        alone = scan_of(c, data)
    # (without the stitch mask the probe records what decodes from the chain's first block on, framing and all)
    assert alone == expected(data)[0] and any(r[3] == 24 and r[0] <= p < r[0] + r[1] for r in alone)
    kept, _ = zpng.stitched_records(data, prior)
    assert len(kept) == 1 and kept[0]["offset"] == first
    st = [(r["offset"], r["comp_len"], r["infl_len"], r["type"]) for r in kept]
    hulls = prior + [(r["offset"], zpng.hull(r["pieces"])) for r in kept]
    with antiz_amd.Context(device=0, stitch=("png",), probe=PROBE) as c:
        both = scan_of(c, data)
    assert both == sorted(ref + st + zprobe.probe_records(data, hulls))
    assert not any(r[3] >= 24 for r in both)


# ---- 5. limits, slot loss ------------------------------------------------------------------------------------
def test_limits(ctx):
    def dyn(nbytes, seed):
        b = zraw.raw_deflate(zprobe.skewed(seed, nbytes), 6, 8)
        assert (b[0] >> 1) & 3 == 2
        return b

    long_payload = txt(41, 20000)
    whole = zraw.raw_deflate(long_payload, 6, 1)   # memLevel 1: a block every few hundred bytes
    fixed = zraw.raw_deflate(b"tiny input", 6, 8)
    stored = zraw.raw_deflate(txt(42, 3000), 0, 8)
    assert (whole[0] >> 1) & 3 == 2 and (fixed[0] >> 1) & 3 == 1 and (stored[0] >> 1) & 3 == 0
    items = [dyn(255, 1), dyn(256, 2), dyn(257, 3), whole[:len(whole) * 2 // 3], fixed, stored, whole]
    data, at = joined(items, seed=14)
    got = scan_of(ctx, data)
    assert got == expected(data)[0]
    assert [r for r in got if r[3] >= 24] == [(at[1], len(items[1]), 256, 24), (at[2], len(items[2]), 257, 24),
                                              (at[6], len(whole), len(long_payload), 24)]


def test_an_output_past_its_slot(ctx):
    payload = txt(43, 100000)
    body = zraw.raw_deflate(payload, 6, 8)
    data, (at,) = joined([body], seed=15)
    atz, st = ctx.precompress(data)
    assert st["n_inflate_retries"] >= 1   # the 64 KiB slot overflowed: decoded again with the 32 KiB ring
    d = {d["off"]: d for d in parse_atz(atz)[2]}[at]
    assert (d["c"], d["m"], d["cl"], d["il"], d["nd"]) == (0x40 | 6, 8, len(body), len(payload), 0)
    assert ctx.reconstruct(atz) == data


# ---- 6. a cap knob, errors ---------------------------------------------------------------------------------
CAPS = r"""
import hashlib, sys
sys.path.insert(0, %r)
import antiz_amd
data = open(sys.argv[1], "rb").read()
with antiz_amd.Context(device=0, probe=("deflate",)) as c:
    out, st = c.precompress(data)
    back = c.reconstruct(out)
print(int(back == data))
print(hashlib.sha256(out).hexdigest())
""" % ROOT


def test_a_small_cap_keeps_the_bytes(ctx, tmp_path):
    bodies = [zraw.raw_deflate(txt(50 + k, 30000 + 9000 * k), 6, 8) for k in range(3)]
    data, _ = joined(bodies + [zstrat.deflate(txt(60, 5000), 6, 15, 8, 0)], seed=16)
    atz, _ = ctx.precompress(data)
    assert atz[:4] == b"ATZ\3" and sum(1 for d in parse_atz(atz)[2] if d["c"] & 0x40) == 3
    path = str(tmp_path / "f.bin")
    with open(path, "wb") as f:
        f.write(data)
    r = subprocess.run([sys.executable, "-c", CAPS, path], env=dict(os.environ, ATZ_CAP_DIV="4096"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2] == "1" and lines[-1] == hashlib.sha256(atz).hexdigest()


def test_errors(ctx):
    import antiz_amd
    L = antiz_amd.lib()
    for bad in (2, 3, 1 << 31):
        with pytest.raises(antiz_amd.AtzError) as e:
            antiz_amd._check(L.atz_set_probe(ctx.h, bad))
        assert e.value.code == -1
    with antiz_amd.Context(device=0, containers=("zip",)) as c:   # the container switch keeps its own bits
        with pytest.raises(antiz_amd.AtzError):
            antiz_amd._check(L.atz_set_containers(c.h, 4))
    data = txt(1, 4096) + zstrat.deflate(txt(2, 3000), 6, 15, 8, 0)
    with dev_copy(data) as d:
        with pytest.raises(antiz_amd.AtzError) as e:
            ctx.shard_scan(d, data, 0, 1)
        assert e.value.code == -1
        with pytest.raises(antiz_amd.AtzError) as e:
            ctx.shard_sweep(d, data, [b""])
        assert e.value.code == -1
