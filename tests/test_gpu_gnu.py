"""The deflater extension on the GPU: bodies written by GNU gzip and Info-ZIP's zip
(tests/golden/gnu.json, gnu.bin) against the GNU trial kernels -- the exact deflate, the raw walk end to end under the
container and probe switches, the ATZ5 file and its reader, the switch's off state, and the errors."""
import ctypes as C
import hashlib
import os
import random
import struct
import subprocess
import sys
import zlib

import pytest

import zgnu
import zraw
import zstrat
from test_gpu_strategy import dev_copy, hip, parse_atz, txt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = ("zip", "gzip")
G = zgnu.fixtures()
ENTRIES = [e for e in G["entries"] if e["class"] in "abcde"]
TAILS = [e for e in G["entries"] if e["class"] == "g"]
for _e in G["entries"]:
    _e["data"] = zlib.decompress(_e["body"], -15)
ZIP = G["zip"]["bytes"]


def ident(e):
    return "%s-L%d-%s" % (e["class"], e["level"], e["note"].split(":")[0].replace(" ", "_")[:24])


# ---- 1. the exact deflate ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain():
    import antiz_amd
    with antiz_amd.Context(device=0) as c:
        yield c


@pytest.mark.parametrize("e", ENTRIES, ids=ident)
def test_deflate_equals_the_binary(plain, e):
    assert plain.deflate(e["data"], e["level"], 15, 8, raw=True, deflater="gnu") == e["body"]


def test_deflate_equals_zip_members_in_one_batch(plain):
    mem = G["zip"]["members"]
    bodies = [ZIP[m["offset"]:m["offset"] + m["csize"]] for m in mem]
    datas = [zlib.decompress(b, -15) for b in bodies]
    buf, items, at = b"".join(datas), [], 0
    for m, d in zip(mem, datas):
        items.append((at, len(d), m["level"], 15, 3, 0, True, "gnu"))   # (the memLevel field is ignored)
        at += len(d)
    assert plain.deflate_batch(buf, items) == bodies


# ---- 2.-3. the raw walk end to end --------------------------------------------------------------------
def build_file(entries, seed=21, with_zip=True):
    """gzip members (no level hint) around the entries' bodies and the zip archive, random filler between
    -> (file, [(body offset, body, data, class, level)])"""
    r = random.Random(seed)
    parts, recs, pos = [], [], 0

    def put(blob, body_at, body, data, cls, level):
        nonlocal pos
        fill = r.randbytes(r.randrange(50, 200))
        parts.extend([fill, blob])
        recs.append((pos + len(fill) + body_at, body, data, cls, level))
        pos += len(fill) + len(blob)

    for e in entries:
        put(zraw.gzip_member(e["body"], e["data"]), 10, e["body"], e["data"], e["class"], e["level"])
    if with_zip:
        fill = r.randbytes(100)
        parts.append(fill)
        for m in G["zip"]["members"]:
            body = ZIP[m["offset"]:m["offset"] + m["csize"]]
            recs.append((pos + len(fill) + m["offset"], body, zlib.decompress(body, -15), "f", m["level"]))
        parts.append(ZIP)
        pos += len(fill) + len(ZIP)
    parts.append(r.randbytes(120))
    return b"".join(parts), recs


def swept(c, data):
    recs = c.scan(data)
    res, _ = c.sweep()
    return {r[0]: (r, q) for r, q in zip(recs, res)}


@pytest.fixture(scope="module")
def e2e():
    import antiz_amd
    data, recs = build_file(ENTRIES)
    out = dict(data=data, recs=recs)
    with antiz_amd.Context(device=0, containers=BOTH, deflaters=("gnu",)) as c:
        out["on"], out["st_on"] = c.precompress(data)
        out["res_on"] = swept(c, data)
    with antiz_amd.Context(device=0, containers=BOTH, deflaters=()) as c:
        out["zero"], out["st_zero"] = c.precompress(data)
        out["res_off"] = swept(c, data)
    return out


def test_bodies_are_recorded_as_gnus(e2e):
    import antiz_amd
    data, on = e2e["data"], e2e["on"]
    assert on[:4] == b"ATZ\5"
    ver, origlen, descs = parse_atz(on)
    assert ver == 5 and origlen == len(data)
    by = {d["off"]: d for d in descs}
    n_gnu = 0
    for at, body, payload, cls, level in e2e["recs"]:
        rec, res = e2e["res_on"][at]
        d = by[at]
        hint = rec[1] - 24   # (the gzip members here carry none; zip states its own)
        assert hint in (0, 1, 2) and rec[2] == len(body) and rec[3] == len(payload), (cls, level)
        assert res["recomp"] == 1 and res["n_diff"] == 0 and res["window"] == 15, (cls, level)
        assert (d["cl"], d["il"], d["nd"], d["w"]) == (len(body), len(payload), 0, 15)
        if cls == "a":   # zlib's own bytes: found earlier in the list, as without the switch
            off = e2e["res_off"][at][1]
            assert res["memlevel"] == 8 and res["n_trials"] <= 10 and (d["c"], d["m"]) == (res["clevel"], 8)
            assert [res[k] for k in ("clevel", "n_trials", "ident")] == [off[k] for k in ("clevel", "n_trials", "ident")]
        else:
            assert (res["clevel"], res["memlevel"], d["c"], d["m"]) == (0x40 | level, 0, 0x40 | level, 0), (cls, level)
            want = 11 + [lv for lv in zgnu.LEVELS[hint] if lv].index(level)   # the whole memLevel-8 group, then GNU's
            assert res["n_trials"] == want, (cls, level, res["n_trials"])
            n_gnu += 1
    assert n_gnu == len(ENTRIES) - 3 + 3
    with antiz_amd.Context(device=0) as c:   # any context reads the file
        assert c.reconstruct(on) == data
        with dev_copy(on) as dp:
            p, n = c.reconstruct_device(dp, on)
            back = C.create_string_buffer(n)
            assert hip().hipMemcpy(back, p, n, 2) == 0   # device to host
            assert back.raw == data


def test_reader_checks_gnu_descriptors(e2e, plain):
    import antiz_amd
    on = e2e["on"]
    _, _, descs = parse_atz(on)
    at, first = 28, None
    for d in descs:
        if d["m"] == 0 and first is None:
            first = at
        at += len(d["raw"])
    assert first is not None
    for magic in (b"ATZ\4", b"ATZ\3", b"ATZ\1"):   # memLevel 0 under an older magic
        with pytest.raises(antiz_amd.AtzError):
            plain.reconstruct(magic + on[4:])

    def mutated(off, val):
        b = bytearray(on)
        b[first + off] = val
        return bytes(b)

    c0 = on[first + 24]
    for off, val in ((24, c0 | 0x10), (24, c0 | 0x30), (24, c0 | 0x80), (24, c0 & 0x3f), (24, 0x40), (24, 0x4a), (25, 14),
                     (26, 10)):
        with pytest.raises(antiz_amd.AtzError):   # a strategy, stitched, not raw, level 0 / 10, window 14, memLevel 10
            plain.reconstruct(mutated(off, val))
    assert plain.reconstruct(on) == e2e["data"]


def test_mask_zero_is_no_mask(e2e):
    import antiz_amd
    data = e2e["data"]
    with antiz_amd.Context(device=0, containers=BOTH) as c:   # (ATZ_DEFLATERS is not set in the suite's environment)
        assert "ATZ_DEFLATERS" not in os.environ
        unset, _ = c.precompress(data)
    assert unset == e2e["zero"] and unset[:4] == b"ATZ\3"
    for at, body, payload, cls, level in e2e["recs"]:
        rec, res = e2e["res_off"][at]
        if cls == "a":
            assert res["recomp"] == 1 and res["n_diff"] == 0 and res["memlevel"] == 8
        elif cls in "bcde":
            assert not (res["recomp"] == 1 and res["n_diff"] == 0), (cls, level)
        assert not (res["recomp"] == 1 and res["memlevel"] == 0)
    with antiz_amd.Context(device=0, deflaters=("gnu",)) as c:   # alone the switch changes nothing
        alone, _ = c.precompress(data)
    with antiz_amd.Context(device=0) as c:
        none, _ = c.precompress(data)
    assert alone == none and none[:4] == b"ATZ\1"


# ---- 4. the tail near misses -----------------------------------------------------------------------------
def test_tails_are_near_misses():
    import antiz_amd
    data, recs = build_file(TAILS, seed=22, with_zip=False)
    with antiz_amd.Context(device=0, containers=BOTH, deflaters=("gnu",)) as c:
        atz, _ = c.precompress(data)
        res = swept(c, data)
        for at, body, payload, _, level in recs:
            rec, q = res[at]
            assert q["recomp"] == 1 and 0 < q["n_diff"] <= 128, q
        assert c.reconstruct(atz) == data


# ---- 5. the probe ----------------------------------------------------------------------------------------
def test_probe_finds_a_bare_body():
    import antiz_amd
    e = [x for x in ENTRIES if x["class"] == "b" and x["level"] == 6 and x["note"].startswith("pass")][0]
    assert (e["body"][0] >> 1) & 3 == 2   # a dynamic first block: what the probe looks for
    r = random.Random(23)
    pre = r.randbytes(777)
    data = pre + e["body"] + r.randbytes(333)
    with antiz_amd.Context(device=0, probe=("deflate",), deflaters=("gnu",)) as c:
        atz, _ = c.precompress(data)
        d = {d["off"]: d for d in parse_atz(atz)[2]}[len(pre)]
        assert atz[:4] == b"ATZ\5" and (d["c"], d["w"], d["m"], d["cl"], d["nd"]) == (0x40 | 6, 15, 0, len(e["body"]), 0)
        assert c.reconstruct(atz) == data


# ---- 6. errors ---------------------------------------------------------------------------------------------
def test_errors(plain):
    import antiz_amd
    L = antiz_amd.lib()
    with antiz_amd.Context(device=0, deflaters=("gnu",)) as c:
        for bad in (2, 3, 1 << 31):
            with pytest.raises(antiz_amd.AtzError) as e:
                antiz_amd._check(L.atz_set_deflaters(c.h, bad))
            assert e.value.code == -1
        data = txt(1, 4096) + zstrat.deflate(txt(2, 3000), 6, 15, 8, 0)
        with dev_copy(data) as d:
            with pytest.raises(antiz_amd.AtzError) as e:
                c.shard_scan(d, data, 0, 1)
            assert e.value.code == -1
            with pytest.raises(antiz_amd.AtzError) as e:
                c.shard_sweep(d, data, [b""])
            assert e.value.code == -1
        antiz_amd._check(L.atz_set_deflaters(c.h, 0))
        with dev_copy(data) as d:
            assert c.shard_scan(d, data, 0, 1)
    payload = txt(3, 2000)
    # (offset, length, level, window, memLevel, strategy, raw, deflater)
    for item in ((0, 2000, 6, 15, 8, 0, False, "gnu"), (0, 2000, 6, 14, 8, 0, True, "gnu"), (0, 2000, 0, 15, 8, 0, True, "gnu"),
                 (0, 2000, 10, 15, 8, 0, True, "gnu"), (0, 2000, 6, 15, 8, 1, True, "gnu"), (0, 2000, 6, 15, 8, 3, True, "gnu")):
        with pytest.raises(antiz_amd.AtzError) as e:
            plain.deflate_batch(payload, [item])
        assert e.value.code == -1, item
    with pytest.raises(ValueError):
        plain.deflate(payload, 6, 15, 8, raw=True, deflater="7zip")
    for m in (0, 8, 77):   # the memLevel field is ignored
        assert plain.deflate(payload, 6, 15, m, raw=True, deflater="gnu") == zraw.raw_deflate(payload, 6, 8)


# ---- 7. a cap knob, the CLI ----------------------------------------------------------------------------------
CAPS = r"""
import hashlib, sys
sys.path.insert(0, %r)
import antiz_amd
data = open(sys.argv[1], "rb").read()
with antiz_amd.Context(device=0, containers=("zip", "gzip")) as c:
    out, st = c.precompress(data)
    back = c.reconstruct(out)
print(int(back == data))
print(hashlib.sha256(out).hexdigest())
""" % ROOT


def test_a_small_cap_keeps_the_bytes(e2e, tmp_path):
    path = str(tmp_path / "f.bin")
    with open(path, "wb") as f:
        f.write(e2e["data"])
    r = subprocess.run([sys.executable, "-c", CAPS, path], env=dict(os.environ, ATZ_CAP_DIV="4096", ATZ_DEFLATERS="gnu"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2] == "1" and lines[-1] == hashlib.sha256(e2e["on"]).hexdigest()


def test_cli(e2e, tmp_path):
    import antiz_amd
    f = str(tmp_path / "f")
    with open(f, "wb") as fh:
        fh.write(e2e["data"])
    env = dict(os.environ, ATZ_CONTAINERS="zip,gzip", ATZ_DEFLATERS="gnu", ATZ_DEVICE="0")
    r = subprocess.run([antiz_amd.CLI_PATH, "-i", f], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    assert "OK! Restoration is bit by bit identical" in r.stdout
    assert open(f + ".atz", "rb").read() == e2e["on"]
    r = subprocess.run([antiz_amd.CLI_PATH, "-i", f], env=dict(env, ATZ_DEFLATERS="gnu,7zip"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 1 and "ATZ_DEFLATERS: unknown deflater 7zip" in r.stderr
