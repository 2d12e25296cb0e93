"""The probe extension's host-side surface and its model, without a GPU: the rule is necessary
for every raw stream of zlib 1.2.8 whose first block is dynamic, holds at the file's end exactly as far as the
header's bits reach, lets no position of random bytes through to a record, and the merge keeps what it should."""
import ctypes as C
import os
import random
import subprocess

import pytest

import _libs
import zprobe
import zraw
import zstrat


def test_exports_are_listed_and_declared():
    import antiz_amd
    L = C.CDLL(antiz_amd.LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "atz_accel.h")).read()
    for name in ("atz_set_probe", "atz_probe_positions"):
        assert name in antiz_amd.EXPORTS
        assert getattr(L, name)
        assert "int %s(atz_ctx_t *ctx" % name in hdr


def test_probe_mask():
    import antiz_amd
    assert antiz_amd.PROBES == {"deflate": 0}
    assert antiz_amd.probe_mask(()) == 0 and antiz_amd.probe_mask("") == 0 and antiz_amd.probe_mask(",") == 0
    assert antiz_amd.probe_mask("deflate") == 1 and antiz_amd.probe_mask(("deflate",)) == 1
    assert antiz_amd.probe_mask("deflate,deflate") == 1
    for bad in ("brute", "deflate,zip", ("Deflate",)):
        with pytest.raises(ValueError):
            antiz_amd.probe_mask(bad)


def test_cli_refuses_an_unknown_word(tmp_path):
    """The words are parsed before the device is opened, so this needs none."""
    import antiz_amd
    f = str(tmp_path / "f")
    with open(f, "wb") as fh:
        fh.write(b"x" * 100)
    r = subprocess.run([antiz_amd.CLI_PATH, "-i", f], env=dict(os.environ, ATZ_PROBE="deflate,brute"),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Error Encountered: ATZ_PROBE: unknown probe brute" in r.stderr


# ---- the rule ---------------------------------------------------------------------------------------------
def scanlines(seed, nbytes):
    """Scanline-like bytes: rows of a slowly changing byte behind a filter-type byte."""
    r = random.Random(seed)
    out, v = bytearray(), 128
    while len(out) < nbytes:
        out.append(r.randrange(3))
        for _ in range(96):
            v = (v + r.randrange(-2, 3)) % 256
            out.append(v)
    return bytes(out[:nbytes])


INPUTS = [(kind, size) for kind in ("text", "scanlines") for size in (300, 4000, 70000)]


@pytest.mark.parametrize("kind,size", INPUTS)
def test_the_rule_is_necessary(kind, size):
    """Whenever libz128's raw body starts with a dynamic block, position 0 survives -- also with the body at
    offsets 0..17 of a file (every phase of a lane's 16-byte load)."""
    data = _libs.text(random.Random(size), size) if kind == "text" else scanlines(size, size)
    filler = random.Random(1).randbytes(17)
    n_dyn = 0
    seen = set()
    for lv in range(1, 10):
        for m in (1, 8, 9):
            for st in range(4):
                body = zstrat.deflate(data, lv, -15, m, st)
                if (body[0] >> 1) & 3 != 2 or body[:12] in seen:
                    continue
                seen.add(body[:12])
                n_dyn += 1
                assert zprobe.probe_ok(body, 0), (lv, m, st)
                for off in range(18):
                    f = filler[:off] + body + filler
                    assert zprobe.probe_ok(f, off), (lv, m, st, off)
                assert 0 in zprobe.positions(body)
    assert n_dyn >= 3, "the inputs are meant to give dynamic first blocks"


@pytest.mark.parametrize("nc", [4, 5, 12, 19])
def test_truncation(nc):
    r = random.Random(nc)
    for _ in range(20):
        h = zprobe.header(nc, r, bfinal=r.randrange(2))
        assert len(h) == zprobe.header_bytes(nc)
        for lead in (0, 1, 15, 16, 33):
            f = r.randbytes(lead) + h
            assert zprobe.probe_ok(f, lead)              # the last needed bit lies in the file's last byte
            assert not zprobe.probe_ok(f[:-1], lead)     # one byte shorter
            assert lead in zprobe.positions(f) and lead not in zprobe.positions(f[:-1])


def test_each_condition_rejects():
    r = random.Random(5)
    ok = zprobe.header(8, r, hlit=29, hdist=29) + bytes(8)
    assert zprobe.probe_ok(ok, 0)
    for bad in (zprobe.header(8, r, hlit=30), zprobe.header(8, r, hdist=30), zprobe.header(8, r, hdist=31),
                zprobe.header(8, r, lens=[1, 1, 1, 0, 0, 0, 0, 0]),      # over-subscribed
                zprobe.header(8, r, lens=[1, 2, 0, 0, 0, 0, 0, 0]),      # incomplete
                zprobe.header(8, r, lens=[0] * 8),                      # empty
                zprobe.header(8, r, lens=[1, 0, 0, 0, 0, 0, 0, 0])):     # a single code: incomplete for zlib's CODES table
        assert not zprobe.probe_ok(bad + bytes(8), 0)
    for btype in (0, 1, 3):
        b = bytearray(ok)
        b[0] = (b[0] & ~6) | (btype << 1)
        assert not zprobe.probe_ok(bytes(b), 0)
    # lengths past nc do not count
    h = bytearray(zprobe.header(4, r, lens=[1, 1, 0, 0]) + b"\xff" * 8)
    h[3] |= 0xe0
    assert zprobe.probe_ok(bytes(h), 0)


@pytest.fixture(scope="module")
def random_mib():
    return random.Random(20260).randbytes(1 << 20)


def test_positions_equal_the_rule(random_mib):
    data = random_mib[:70000]
    assert zprobe.positions(data) == [p for p in range(len(data)) if zprobe.probe_ok(data, p)]
    deflated = zstrat.deflate(_libs.text(random.Random(9), 200000), 6, -15, 8, 0)
    assert zprobe.positions(deflated) == [p for p in range(len(deflated)) if zprobe.probe_ok(deflated, p)]
    for n in range(0, 12):
        assert zprobe.positions(data[:n]) == [p for p in range(n) if zprobe.probe_ok(data[:n], p)]


def test_random_bytes_give_no_record(random_mib):
    st = {}
    assert zprobe.probe_records(random_mib, [], st) == []
    print("random 1 MiB:", st)
    # 1/4 (BTYPE) x (30/32)^2 (HLIT, HDIST) of the positions reach the Kraft sum; about 0.4 % of those pass it
    assert 300 <= st["survivors"] <= 3000 and st["decoded"] == st["survivors"] and st["accepted"] == 0


# ---- the merge -----------------------------------------------------------------------------------------------
def body_of(nbytes, seed=1, lv=6, m=8):
    payload = zprobe.skewed(seed, nbytes)
    body = zraw.raw_deflate(payload, lv, m)
    assert (body[0] >> 1) & 3 == 2, "first block must be dynamic"
    return body, payload


def test_minimum_output():
    fill = bytes(40)   # zeros: BTYPE 0 everywhere
    for nbytes, kept in ((255, False), (256, True), (257, True)):
        body, payload = body_of(nbytes, seed=nbytes)
        f = fill + body + fill
        want = [(40, len(body), nbytes, 24)] if kept else []
        assert zprobe.probe_records(f, []) == want, nbytes
        assert 40 in zprobe.positions(f)


def test_earlier_records_win():
    body, payload = body_of(3000)
    f = bytes(100) + body + bytes(100)
    rec = (100, len(body), 3000, 24)
    assert zprobe.probe_records(f, []) == [rec]
    # the start lies inside a record made before (its hull): not even decoded
    st = {}
    assert zprobe.probe_records(f, [(90, 20)], st) == [] and st["decoded"] < st["survivors"]
    # a record made before lies inside the candidate, or touches its last byte
    assert zprobe.probe_records(f, [(150, 10)]) == []
    assert zprobe.probe_records(f, [(100 + len(body) - 1, 5)]) == []
    # records that only touch it from outside leave it alone
    assert zprobe.probe_records(f, [(50, 50), (100 + len(body), 30)]) == [rec]


def test_greedy_in_ascending_offset():
    """A stream with a full flush: its second part is a stream of its own, byte-aligned, inside the first."""
    import zlib
    a, b = zprobe.skewed(1, 2000), zprobe.skewed(2, 2000)
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    first = z.compress(a) + z.flush(zlib.Z_FULL_FLUSH)
    whole = first + z.compress(b) + z.flush()
    f = bytes(64) + whole + bytes(64)
    assert zprobe.probe_ok(f, 64) and zprobe.probe_ok(f, 64 + len(first))
    assert zprobe.accept(f, 64 + len(first)) == (len(whole) - len(first), 2000)
    assert zprobe.probe_records(f, []) == [(64, len(whole), 4000, 24)]
    # two streams one after the other are both kept
    one, _ = body_of(1500, seed=3)
    two, _ = body_of(1600, seed=4)
    f = bytes(10) + one + two + bytes(10)
    assert zprobe.probe_records(f, []) == [(10, len(one), 1500, 24), (10 + len(one), len(two), 1600, 24)]


def test_the_walk_is_the_raw_walk_without_a_hint():
    assert zprobe.candidates() == zraw.candidates(zraw.HINT_NONE) and len(zprobe.candidates()) == 90
    body, payload = body_of(3000, lv=9, m=9)
    want = zprobe.rule(body, payload)
    assert want["ident"] == len(body) and want["diff_pos"] == [] and want["window"] == 15
