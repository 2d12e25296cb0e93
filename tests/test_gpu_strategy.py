"""The strategy extension on the GPU: exact deflate under Z_FILTERED / Z_RLE /
Z_HUFFMAN_ONLY against the reference's zlib 1.2.8 (tests/zstrat.py), the opt-in second walk end to end, its
rule against a Python model on that zlib, the caps, the ATZ2 reader, the CLI and the shard refusal.

Every expected byte comes from oracle/_ref/libz128.so; without it these tests fail, they do not skip.
"""
import ctypes as C
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

import _libs
import atzfile
import zstrat

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = 14   # filtered | huffman | rle
NAMES = ("filtered", "rle", "huffman")


# ---- payloads -------------------------------------------------------------------------------------
def gradient(seed, nbytes):
    """Scanline-filtered smooth image rows (datagen's PNG-like payload, before compression)."""
    rng = np.random.default_rng(seed)
    width = int(rng.integers(16, 120))
    rows = max(1, nbytes // (width * 3 + 1)) + 1
    img = np.cumsum(rng.integers(-3, 4, size=(rows, width * 3)), axis=1).astype(np.int64) % 256
    raw = bytearray()
    prev = np.zeros(width * 3, dtype=np.int64)
    for r in range(rows):
        f = int(rng.integers(0, 3))
        line = img[r]
        if f == 1:
            flt = (line - np.concatenate(([0, 0, 0], line[:-3]))) % 256
        elif f == 2:
            flt = (line - prev) % 256
        else:
            flt = line
        raw.append(f)
        raw += flt.astype(np.uint8).tobytes()
        prev = line
    return bytes(raw[:nbytes])


def runs(seed, nbytes):
    """Run-heavy bytes: runs of 1..600 of a random byte (lengths around 3 and 258 included)."""
    r = random.Random(seed)
    out = bytearray()
    while len(out) < nbytes:
        out += bytes([r.randrange(256)]) * r.choice((1, 1, 2, 3, 4, 5, 9, 40, 257, 258, 259, 600))
    return bytes(out[:nbytes])


def tiny(seed, strat):
    """40 bytes on which the strategy still parses differently from the default: a repeat of length 4
    (Z_FILTERED drops it), or repeats at distance 3 beside a run (Z_RLE and Z_HUFFMAN_ONLY do not code them)."""
    r = random.Random(seed)
    if strat == 1:
        w = r.randbytes(4)
        return w + r.randbytes(9) + w + r.randbytes(10) + w + r.randbytes(9)
    return r.randbytes(3) * 8 + r.randbytes(1) * 16


def rnd(seed, nbytes):
    return random.Random(seed).randbytes(nbytes)


def txt(seed, nbytes):
    return _libs.text(random.Random(seed), nbytes)


def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


class dev_copy:
    """`data` in device memory with the 4096 bytes of slack the device entry points ask for."""

    def __init__(self, data):
        self.data, self.d = data, C.c_void_p()

    def __enter__(self):
        assert hip().hipMalloc(C.byref(self.d), len(self.data) + 4096) == 0
        assert hip().hipMemcpy(self.d, self.data, len(self.data), 1) == 0   # host to device
        return self.d.value

    def __exit__(self, *a):
        hip().hipFree(self.d)


@pytest.fixture(scope="module")
def ctx():
    import antiz_amd
    with antiz_amd.Context(device=0) as c:
        yield c


# ---- 1. exact deflate -----------------------------------------------------------------------------
def kat_inputs():
    t = txt(7, 3000)
    ins = [t[:k] for k in range(5)]
    for L in (3, 4, 257, 258, 259, 260, 517):
        ins.append(b"x" + b"a" * L)            # after a different first byte, reaching the end of input
        ins.append(b"x" + b"a" * L + b"yz")
        ins.append(b"a" * L)                   # from position 0: the first byte is always a literal
    ins.append(b"q" + b"a" * 100 + b"b" * 300 + b"c")   # two runs back to back
    ins.append(t)                              # matches of length 3-5, lazy improvements; memLevel 1: > 400 symbols
    ins.append(gradient(11, 3000))
    ins.append(rnd(13, 2000))                  # the stored-block choice under Z_HUFFMAN_ONLY
    return ins


def test_exact_deflate_kats(ctx):
    import antiz_amd
    ins = kat_inputs()
    big = txt(17, 70000)                       # window slides at windowBits 9
    buf, offs = bytearray(), []
    for d in ins + [big]:
        offs.append(len(buf))
        buf += d
        buf += b"\0" * (-len(buf) % 16)
    items, want = [], []
    for strat in (1, 2, 3):
        for lv in (1, 3, 4, 5, 6, 7, 8, 9):
            for m in (1, 8, 9):
                for w in (9, 15):
                    for i, d in enumerate(ins):
                        items.append((offs[i], len(d), lv, w, m, strat))
                        want.append(zstrat.deflate(d, lv, w, m, strat))
                items.append((offs[len(ins)], len(big), lv, 9, m, strat))
                want.append(zstrat.deflate(big, lv, 9, m, strat))
    # stored blocks about as long as the window, so that blocks start just before and after each window
    # slide (a block whose start has slid out of the window cannot be stored: Z/deflate.c FLUSH_BLOCK_ONLY);
    # the slides of deflate_rle and deflate_huff come at other positions than deflate_slow's
    noise = [rnd(19, 5000), rnd(23, 1024), rnd(29, 1023 + 762), runs(31, 900) + rnd(37, 3000)]
    for d in noise:
        offs.append(len(buf))
        buf += d
        buf += b"\0" * (-len(buf) % 16)
    for strat in (1, 2, 3):
        for m in (1, 2, 3, 4):
            for w in (9, 10):
                for i, d in enumerate(noise):
                    items.append((offs[len(ins) + 1 + i], len(d), 6, w, m, strat))
                    want.append(zstrat.deflate(d, 6, w, m, strat))
    # Z_FILTERED only changes deflate_slow: at levels 1 and 3 the output is the default strategy's
    nf = len(items)
    for lv in (1, 3):
        for m in (1, 8, 9):
            for i, d in enumerate(ins):
                items.append((offs[i], len(d), lv, 15, m, 0))
                want.append(zstrat.deflate(d, lv, 15, m, 0))
                assert want[-1] == zstrat.deflate(d, lv, 15, m, 1)
    got = ctx.deflate_batch(bytes(buf), items)
    bad = [items[k] for k in range(len(items)) if got[k] != want[k]]
    print("kats: %d items, %d differ" % (len(items), len(bad)))
    assert not bad, bad[:20]
    by = {it: got[k] for k, it in enumerate(items)}
    for k in range(nf, len(items)):
        o, n, lv, w, m, _ = items[k]
        assert by[(o, n, lv, w, m, 1)] == got[k]
    assert ctx.deflate(ins[8], 6, 15, 8, strategy=3) == zstrat.deflate(ins[8], 6, 15, 8, 3)
    for strat in (2, 3):
        with pytest.raises(antiz_amd.AtzError) as e:
            ctx.deflate(b"abc", 0, 15, 8, strategy=strat)
        assert e.value.code == -1   # ATZ_E_ARG


# ---- 2. end to end --------------------------------------------------------------------------------
def default_list(header):
    """The reference's 81 default-strategy trials for a header (tryParams*, main.cpp:487-560), unordered."""
    w = (header[0] >> 4) + 8
    return [(lv, w, m) for lv in range(0, 10) for m in range(1, 10)]


def build_file(seed=5, strategy_streams=True):
    """-> (file bytes, [(offset, stream, payload, kind)]) ; kind 'd' default, else a strategy number."""
    r = random.Random(seed)
    parts, recs, pos = [], [], 0

    def put(stream, payload, kind):
        nonlocal pos
        fill = txt(r.randrange(1 << 30), r.randrange(20, 400))
        parts.append(fill)
        pos += len(fill)
        recs.append((pos, stream, payload, kind))
        parts.append(stream)
        pos += len(stream)

    dflt = [(lv, txt(100 + k, sz)) for k, (lv, sz) in enumerate(
        [(6, 4000), (9, 12000), (1, 3000), (6, 900), (4, 7000), (9, 300), (2, 5000), (6, 20000), (7, 2500),
         (5, 1500), (6, 64), (3, 10000)])]
    strat = []
    if strategy_streams:
        sizes = [40, 700, 1500, 3000, 6000, 9000, 14000, 20000]
        k = 0
        for m in (1, 8, 9):
            for lv in (4, 5, 6, 7, 8, 9):
                n = sizes[(k * 3 + 2) % 8]
                strat.append((1, lv, m, tiny(200 + k, 1) if n == 40 else gradient(200 + k, n)))
                k += 1
        for m in (1, 8, 9):
            for j in range(2):
                n3, n2 = sizes[(k + j) % 8], sizes[(k + 3 + j) % 8]
                strat.append((3, 6, m, tiny(300 + k, 3) if n3 == 40 else runs(300 + k, n3)))
                strat.append((2, 6, m, tiny(400 + k, 2) if n2 == 40 else (gradient if j else runs)(400 + k, n2)))
                k += 1
        strat.append((3, 6, 8, tiny(777, 3)))
        strat.append((1, 9, 8, gradient(999, 300000)))   # the large-stream path
    order = [("d", x) for x in dflt] + [("s", x) for x in strat]
    r.shuffle(order)
    for kind, x in order:
        if kind == "d":
            put(zstrat.deflate(x[1], x[0], 15, 8, 0), x[1], "d")
        else:
            put(zstrat.deflate(x[3], x[1], 15, x[2], x[0]), x[3], x[0])
    parts.append(txt(9, 333))
    return b"".join(parts), recs


def parse_atz(atz):
    """-> (version, origlen, [dict(off, cl, il, c, w, m, nd, raw)]) of an ATZ file (atzfile.parse's fields of these names)."""
    ver, origlen, descs, _ = atzfile.parse(atz)
    return ver, origlen, [{k: d[k] for k in ("off", "cl", "il", "c", "w", "m", "nd", "raw")} for d in descs]


@pytest.fixture(scope="module")
def e2e():
    import antiz_amd
    data, recs = build_file()
    with antiz_amd.Context(device=0) as c:
        off, _ = c.precompress(data)
    with antiz_amd.Context(device=0, strategies=NAMES) as c:
        on, st = c.precompress(data)
    rc, ref, stats = _libs.ora_precompress(data)
    assert rc == 0
    return dict(data=data, recs=recs, off=off, on=on, ref=ref, ora=stats, st=st)


def test_strategy_streams_differ_from_every_default_trial():
    """The premise of the end-to-end test, on the CPU: no strategy stream is a default-list trial's output."""
    _, recs = build_file()
    for _, stream, payload, kind in recs:
        if kind == "d":
            continue
        for lv, w, m in default_list(stream[:2]):
            assert zstrat.deflate(payload, lv, w, m, 0) != stream, (kind, len(payload), lv, m)


def test_end_to_end(e2e):
    import antiz_amd
    data, recs = e2e["data"], e2e["recs"]
    assert e2e["off"][:4] == b"ATZ\1" and e2e["off"] == e2e["ref"]
    ver, origlen, on = parse_atz(e2e["on"])
    _, _, off = parse_atz(e2e["off"])
    assert e2e["on"][:4] == b"ATZ\2" and ver == 2 and origlen == len(data)
    on_by, off_by = {d["off"]: d for d in on}, {d["off"]: d for d in off}
    ora = {s["offset"]: s for s in e2e["ora"]["streams"]}
    n_ext = n_strat = 0
    for pos, stream, payload, kind in recs:
        n_strat += kind != "d"
        if pos not in ora:   # (an 11-byte stream is below what the reference's scan records)
            assert kind != "d" and len(stream) < 20 and pos not in on_by
            continue
        if ora[pos]["recomp"]:
            # recorded by the reference walk -- every default stream, exactly; a strategy stream of a few
            # dozen bytes that some default trial misses by no more than recomp_tresh, with a diff list --
            # and left alone by the extension, byte for byte
            assert (kind == "d") == (off_by[pos]["nd"] == 0), pos
            assert kind == "d" or len(stream) <= 128 + 4, (kind, len(stream))
            assert on_by[pos]["raw"] == off_by[pos]["raw"], pos
            continue
        assert kind != "d" and pos not in off_by, pos
        d = on_by[pos]
        assert d["nd"] == 0 and d["cl"] == len(stream) and d["il"] == len(payload), (pos, d["c"])
        want = zstrat.rule(stream, payload, MASK)
        assert (d["c"] >> 4, d["c"] & 15, d["w"], d["m"]) == (want["strategy"], want["level"], want["window"], want["memlevel"])
        # (a Z_HUFFMAN_ONLY stream of a payload without runs is Z_RLE's output too, which the list tries first)
        assert want["strategy"] == kind or (kind, want["strategy"]) == (2, 3), pos
        n_ext += 1
    print("recorded by the extension: %d of %d strategy streams" % (n_ext, n_strat))
    assert len(on) == len(off) + n_ext and n_ext >= 24
    with antiz_amd.Context(device=0) as c:
        assert c.reconstruct(e2e["on"]) == data
        with dev_copy(e2e["on"]) as d:
            p, n = c.reconstruct_device(d, e2e["on"])
            out = C.create_string_buffer(n)
            assert hip().hipMemcpy(out, p, n, 2) == 0   # device to host
            assert out.raw == data


def test_default_streams_only_stay_atz1():
    import antiz_amd
    data, _ = build_file(seed=6, strategy_streams=False)
    with antiz_amd.Context(device=0) as c:
        off, _ = c.precompress(data)
    with antiz_amd.Context(device=0, strategies=NAMES) as c:
        on, _ = c.precompress(data)
    assert on == off and on[:4] == b"ATZ\1"


# ---- 3. the rule against the model ------------------------------------------------------------------
OPTS = [dict(), dict(mismatch_tol=0), dict(recomp_tresh=0), dict(sizediff_tresh=0)]


@pytest.mark.parametrize("opts", OPTS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()) or "defaults")
def test_rule_matches_the_model(opts):
    import antiz_amd
    data, recs = nearmiss_file()
    with antiz_amd.Context(device=0, strategies=NAMES, **opts) as c:
        scanned = c.scan(data)
        res, diffs = c.sweep()
    lists = _libs.diff_lists(res, diffs)
    rc, _, ora = _libs.ora_precompress(data, recomp=opts.get("recomp_tresh", 128), sizediff=opts.get("sizediff_tresh", 128),
                                       tol=opts.get("mismatch_tol", 2))
    assert rc == 0
    by = {s[0]: k for k, s in enumerate(scanned)}
    n_rec = 0
    for pos, stream, payload in recs:
        k = by[pos]
        assert scanned[k][2] == len(stream) and scanned[k][3] == len(payload)
        o = ora["streams"][k]
        if o["recomp"]:   # the reference walk's own: untouched
            assert (res[k]["clevel"], res[k]["ident"], res[k]["recomp"]) == (o["clevel"], o["ident"], 1)
            continue
        want = zstrat.rule(stream, payload, MASK, **opts)
        if want is None:
            assert res[k]["recomp"] == 0, pos
            continue
        n_rec += 1
        assert res[k]["recomp"] == 1, pos
        assert (res[k]["clevel"], res[k]["window"], res[k]["memlevel"], res[k]["ident"]) == \
               ((want["strategy"] << 4) | want["level"], want["window"], want["memlevel"], want["ident"]), pos
        assert lists[k][0] == want["diff_pos"] and bytes(lists[k][1]) == want["diff_val"], pos
    print("rule %s: %d of %d recorded by the extension" % (opts, n_rec, len(recs)))
    # four streams, each exact and 1, 3 and 140 bytes off: 140 > recomp_tresh is never recorded, and with
    # recomp_tresh 0 only the exact ones are
    assert n_rec == (4 if opts.get("recomp_tresh") == 0 else 12)


def padded(stream, k):
    """`stream` with k bytes altered past offset 600, still the same stream to inflate: bits that inflate
    ignores are set -- the padding between a stored block's header and its LEN field, and the padding after
    the last end-of-block code (nearmiss.walk_blocks) -- one byte each."""
    import nearmiss
    b = bytearray(stream)
    spots = []
    blocks = nearmiss.walk_blocks(stream)
    for hdr, btype, lo, hi, end in blocks:
        if btype == 0 and hi > lo and (lo >> 3) > 600:
            spots.append((lo, hi))
    end = blocks[-1][4]
    if end % 8 and (end >> 3) > 600:
        spots.append((end, (end | 7) + 1))
    assert len(spots) >= k, (len(spots), k)
    at = set()
    for lo, hi in (spots[-1:] + spots[:-1])[:k]:   # the last byte's padding first
        at.add(nearmiss._set_bits(b, lo, hi))
    assert len(at) == k and sum(1 for x, y in zip(b, stream) if x != y) == k
    return bytes(b)


def nearmiss_file():
    """Strategy streams at memLevel 1 whose payload has a long random stretch (stored blocks, one ignored
    padding field each) between compressible ends (where the default strategy parses differently), each as
    made and with 1, 3 and 140 bytes altered; and one stream whose size is more than sizediff_tresh away
    from every candidate's (the same payload under Z_FIXED, which no candidate produces).
    -> (file, [(offset, stream, payload)])"""
    r = random.Random(31)
    base = [(1, 9, gradient(501, 5000) + rnd(1, 20000) + gradient(502, 4000)),
            (1, 6, gradient(503, 6000) + rnd(2, 19000) + gradient(504, 3000)),
            (3, 6, runs(505, 5000) + rnd(3, 20000) + runs(506, 4000)),
            (2, 6, txt(507, 4000) + rnd(4, 20000) + txt(508, 3000))]
    parts, recs, pos = [], [], 0

    def put(s, payload):
        nonlocal pos
        fill = txt(r.randrange(1 << 30), 100)
        parts.append(fill)
        pos += len(fill)
        recs.append((pos, s, payload))
        parts.append(s)
        pos += len(s)

    for strat, lv, payload in base:
        good = zstrat.deflate(payload, lv, 15, 1, strat)
        put(good, payload)
        for k in (1, 3, 140):
            put(padded(good, k), payload)
    put(zstrat.deflate(base[2][2], 6, 15, 8, 4), base[2][2])
    parts.append(txt(3, 200))
    return b"".join(parts), recs


# ---- 4. caps --------------------------------------------------------------------------------------
CAPS = r"""
import hashlib, sys
sys.path.insert(0, %r)
import antiz_amd
data = open(sys.argv[1], "rb").read()
with antiz_amd.Context(device=0, strategies=("filtered", "rle", "huffman")) as c:
    out, st = c.precompress(data)
    back = c.reconstruct(out)
print(int(back == data))
print(hashlib.sha256(out).hexdigest())
""" % ROOT


@pytest.mark.parametrize("div", ["4096", "1000000000"])
def test_caps_keep_the_bytes(e2e, tmp_path, div):
    import hashlib
    path = str(tmp_path / "f.bin")
    with open(path, "wb") as f:
        f.write(e2e["data"])
    r = subprocess.run([sys.executable, "-c", CAPS, path], env=dict(os.environ, ATZ_CAP_DIV=div),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-2] == "1"
    assert lines[-1] == hashlib.sha256(e2e["on"]).hexdigest()


# ---- 5. the ATZ2 reader -----------------------------------------------------------------------------
def test_atz2_reader_survives_mutations(e2e):
    import antiz_amd
    good = e2e["on"]
    origlen = struct.unpack_from("<Q", good, 12)[0]
    r = random.Random(2024)
    hot = 28 + 43 * 40   # descriptors cluster at the front; half the mutations go there
    accepted = refused = 0
    with antiz_amd.Context(device=0) as c:
        for k in range(200):
            b = bytearray(good)
            if k % 4 == 3:
                b = b[:r.randrange(0, len(b))]
            else:
                at = r.randrange(0, hot) if k % 2 else r.randrange(0, len(b))
                b[at] ^= 1 << r.randrange(8)
            try:
                out = c.reconstruct(bytes(b))
            except antiz_amd.AtzError:
                refused += 1
                continue
            accepted += 1
            assert len(out) == origlen
        assert accepted > 0 and refused > 0, (accepted, refused)
        assert c.reconstruct(good) == e2e["data"]


# ---- 6. CLI -----------------------------------------------------------------------------------------
def test_cli_strategies(e2e, tmp_path):
    import antiz_amd
    f = str(tmp_path / "f")
    with open(f, "wb") as fh:
        fh.write(e2e["data"])
    env = dict(os.environ, ATZ_STRATEGIES="filtered,rle,huffman", ATZ_DEVICE="0")
    r = subprocess.run([antiz_amd.CLI_PATH, "-i", f], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    assert "OK! Restoration is bit by bit identical" in r.stdout
    assert open(f + ".atz", "rb").read() == e2e["on"]
    r = subprocess.run([antiz_amd.CLI_PATH, "-r", "-i", f + ".atz", "-o", f + ".back"], env=dict(os.environ, ATZ_DEVICE="0"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    assert open(f + ".back", "rb").read() == e2e["data"]
    r = subprocess.run([antiz_amd.CLI_PATH, "-i", f], env=dict(env, ATZ_STRATEGIES="filtered,lzma"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 1 and "lzma" in r.stderr


# ---- 7. shard refusal -------------------------------------------------------------------------------
def test_shard_scan_refuses_a_mask():
    import antiz_amd
    data = txt(1, 4096) + zstrat.deflate(txt(2, 3000), 6, 15, 8, 0)
    with antiz_amd.Context(device=0, strategies=("rle",)) as c:
        with dev_copy(data) as d:
            with pytest.raises(antiz_amd.AtzError) as e:
                c.shard_scan(d, data, 0, 1)
            assert e.value.code == -1
    with antiz_amd.Context(device=0) as c:
        with dev_copy(data) as d:
            assert c.shard_scan(d, data, 0, 1)
