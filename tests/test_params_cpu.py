"""antiz_amd/csrc/atz_params.h on the CPU: the candidate lists, the reader's and the batch API's verdicts and the
conversions between a params word, the descriptor bytes and DeflSpec, against models.  tests/params_dump.cpp
(stand-alone, includes only that header) is built with -fsanitize=address,undefined and run directly.

The list models are the extensions' own (zstrat, zraw, zgnu); the verdicts and conversions are modelled here from
INTEGRATION.md s3.1-3.7 and include/atz_accel.h, not from the C++."""
import os
import subprocess

import pytest

import zgnu
import zraw
import zstrat

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "antiz_amd", "csrc")
WINDOWS = list(range(17)) + [0x80, 0x8E, 0x8F, 0xFF]
MEMLEVELS = range(11)
TM_RAW, TM_FLUSH = 2, 64   # antiz_amd/csrc/atz_device.h


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("params") / "params_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(HERE, "params_dump.cpp"), "-o", exe],
                   check=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    lines = {}
    for ln in r.stdout.splitlines():
        lines.setdefault(ln[0], []).append(ln[2:])
    return lines


# ---- models ----------------------------------------------------------------------------------------------
def word_of(level, window, memlevel, strategy=0, raw=False, gnu=False, flush=False):
    """The params word of include/atz_accel.h; a GNU word carries bit 29 and a memLevel field of 0."""
    return (flush << 30) | (gnu << 29) | (raw << 28) | (strategy << 24) | (level << 16) | (window << 8) | \
        (0 if gnu else memlevel)


def spec_fields(level, window, memlevel, strategy=0, raw=False, gnu=False, flush=False):
    """What params_dump prints for a DeflSpec: the fields (a GNU deflate's memLevel is 8, whose tables it reads),
    table_memlevel, needs_tables (level > 0 and strategy < 2), the TM_RAW / TM_FLUSH bits."""
    m = 8 if gnu else memlevel
    return [level, window, m, strategy, int(raw), int(gnu), int(flush), m, int(level > 0 and strategy < 2),
            (TM_RAW if raw else 0) | (TM_FLUSH if flush else 0)]


def desc_ok(version, c, w, m):
    """INTEGRATION.md s3.7."""
    level, strategy, raw, stitched = c & 15, (c >> 4) & 3, bool(c & 0x40), bool(c & 0x80)
    if level > 9 or (strategy >= 2 and level < 1):
        return False
    allowed = {1: 0x0f, 2: 0x3f, 3: 0x7f}.get(version, 0xff)
    if c & ~allowed or (raw and stitched):
        return False
    plain_raw = raw and not stitched and strategy == 0
    if m == 0:
        return version >= 5 and plain_raw and 1 <= level <= 9 and w == 15
    if w & 0x80:
        return version >= 6 and w == 0x8F and plain_raw and 1 <= m <= 9
    return 8 <= w <= 15 and 1 <= m <= 9


def api_ok(p, ex):
    """-> None, or the deflate's (level, window, memlevel, strategy, raw, gnu, flush); INTEGRATION.md s3.7."""
    w, m = (p >> 8) & 0xff, p & 0xff
    if not ex:
        level, strategy, raw, gnu, flush = p >> 16, 0, False, False, False
    else:
        level, strategy = (p >> 16) & 0xff, (p >> 24) & 15
        raw, gnu, flush = bool(p >> 28 & 1), bool(p >> 29 & 1), bool(p >> 30 & 1)
        if p >> 31:
            return None
    if level > 9 or strategy > 3 or (strategy >= 2 and level < 1) or not 8 <= w <= 15:
        return None
    if gnu and not (raw and strategy == 0 and w == 15 and level >= 1):
        return None
    if not gnu and not 1 <= m <= 9:
        return None
    if flush and not (raw and not gnu and strategy == 0 and w >= 9):
        return None
    return level, 9 if w == 8 else w, 8 if gnu else m, strategy, raw, gnu, flush


def ints(s, base=10):
    return [int(x, base) for x in s.split()]


# ---- the lists -------------------------------------------------------------------------------------------
def test_strategy_lists_are_the_model(dump):
    got = {}
    for ln in dump["S"]:
        head, _, tail = ln.partition(":")
        got[tuple(ints(head)[:2])] = ints(tail, 16)
    assert len(got) == 24 * 8
    for ty in range(24):
        header = bytes([((10 + ty // 4 - 8) << 4) | 8, (ty % 4) << 6])
        for mask in range(0, 16, 2):
            want = [word_of(lv, w, m, strategy=st) for st, lv, w, m in zstrat.candidates(header, mask)]
            assert got[(ty, mask)] == want, (ty, mask)


def test_raw_lists_are_the_model(dump):
    got = {}
    for ln in dump["R"]:
        head, _, tail = ln.partition(":")
        got[tuple(ints(head))] = ints(tail, 16)
    assert len(got) == 3 * 2 * 2
    for hint in range(3):
        zl = [zgnu.packed(cd) for cd in zgnu.candidates(hint, False)]
        assert zl == [(1 << 28) | (lv << 16) | (w << 8) | m for lv, w, m in zraw.candidates(hint)]
        gl = [zgnu.packed(cd) for cd in zgnu.candidates(hint, True)]
        fl = [e | (1 << 30) for e in zl]   # a flush list: zlib's with bit 30 on every entry, no GNU entry
        assert (len(zl), len(gl), len(fl)) == (90, 99, 90)
        assert got[(24 + hint, 0, 0)] == zl
        assert got[(24 + hint, 1, 0)] == gl
        assert got[(24 + hint, 0, 1)] == fl and got[(24 + hint, 1, 1)] == fl


def test_list_entries_decode_to_their_parameters(dump):
    """Every entry of every list: the DeflSpec it decodes to (a memLevel field of 0 is GNU) and the word that writes."""
    n = 0
    for ln in dump["E"]:
        e, rest = ln.split(" ", 1)
        e = int(e, 16)
        *f, word = rest.split()
        gnu = (e & 0xff) == 0
        args = ((e >> 16) & 0xff, (e >> 8) & 0xff, e & 0xff, (e >> 24) & 3, bool(e >> 28 & 1), gnu, bool(e >> 30 & 1))
        assert [int(x) for x in f] == spec_fields(*args), hex(e)
        assert int(word, 16) == word_of(*args), hex(e)
        assert gnu or int(word, 16) == e
        n += 1
    assert n > 3 * (90 + 99 + 90 + 90)


# ---- the reader's verdicts -------------------------------------------------------------------------------
def test_valid_desc_is_the_model(dump):
    assert len(dump["D"]) == 6 * 256
    accepted = 0
    for ln in dump["D"]:
        v, c, bits = ln.split()
        v, c = int(v), int(c)
        want = "".join("1" if desc_ok(v, c, w, m) else "0" for w in WINDOWS for m in MEMLEVELS)
        assert bits == want, (v, c)
        accepted += bits.count("1")
    assert accepted > 6 * 10 * 8 * 9


def test_descriptor_round_trips(dump):
    triples = [(c, w, m) for c in range(256) for w in WINDOWS for m in MEMLEVELS if desc_ok(6, c, w, m)]
    assert len(dump["X"]) == len(triples)
    for ln, (c, w, m) in zip(dump["X"], triples):
        *g, word, minv = ln.split()
        g = [int(x) for x in g]
        assert g[:3] == [c, w, m]
        stitched, gnu, flush = bool(c & 0x80), m == 0, bool(w & 0x80)
        args = (c & 15, w & 0x7f, m, (c >> 4) & 3, bool(c & 0x40), gnu, flush)
        assert g[3:13] == spec_fields(*args), ln
        assert g[13] == int(stitched)
        assert g[14:17] == [c, w, m], ln    # desc -> spec -> desc
        assert g[17:20] == [c, w, m], ln    # desc -> spec -> word -> spec -> desc
        assert int(word, 16) == word_of(*args), ln
        want_v = 6 if flush else 5 if gnu else 4 if stitched else 3 if c & 0x40 else 2 if c >> 4 else 1
        assert int(minv) == want_v, ln
        # the lowest version is the lowest reader that accepts the bytes
        assert [v for v in range(1, 7) if desc_ok(v, c, w, m)][0] == want_v, ln


# ---- the batch API's verdicts ----------------------------------------------------------------------------
def test_valid_api_is_the_model(dump):
    words = [(ex, (hi << 24) | (lv << 16) | (w << 8) | m) for ex in (0, 1) for hi in range(256)
             for lv in (0, 1, 9, 10, 255) for w in (7, 8, 9, 14, 15, 16) for m in (0, 1, 8, 9, 10)]
    assert len(dump["A"]) == len(words)
    accepted = 0
    for ln, (ex, p) in zip(dump["A"], words):
        t = ln.split()
        assert (int(t[0]), int(t[1], 16)) == (ex, p)
        want = api_ok(p, ex)
        assert int(t[2]) == (want is not None), ln
        if want is None:
            continue
        accepted += 1
        assert [int(x) for x in t[3:13]] == spec_fields(*want), ln
        assert int(t[13], 16) == int(t[14], 16) == word_of(*want), ln   # spec -> word (-> spec -> word)
        level, window, memlevel, strategy, raw, gnu, flush = want
        assert [int(x) for x in t[15:18]] == [raw << 6 | strategy << 4 | level, window | flush << 7, 0 if gnu else memlevel]
        if ex and (p >> 8) & 0xff != 8 and not gnu:
            assert word_of(*want) == p   # word -> spec -> word
    assert accepted > 2 * 3 * 4 * 3
