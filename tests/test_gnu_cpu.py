"""The deflater extension without a GPU: the fixtures written by GNU gzip and Info-ZIP's zip
against the premises the GNU trial kernels rest on -- the parse is zlib's at memLevel 8, only the block
boundaries differ, and tests/zgnu.py's restatement of ct_tally predicts them -- and the host-side surface."""
import ctypes as C
import os
import zlib

import pytest

import zgnu
import zraw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = zgnu.fixtures()
AF = [e for e in G["entries"] if e["class"] in "abcde"]
TAILS = [e for e in G["entries"] if e["class"] == "g"]


def zlib_raw(data, level):
    """zlib's raw deflate at (level, 15, memLevel 8): the reference's 1.2.8 where built, else the interpreter's"""
    import zstrat
    if os.path.exists(zstrat.Z128_SO):
        return zraw.raw_deflate(data, level, 8)
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
    return z.compress(data) + z.flush()


def ident(e):
    return "%s-L%d-%s" % (e["class"], e["level"], e["note"].split(":")[0].replace(" ", "_")[:24])


def zip_members():
    z = G["zip"]
    return [(m, z["bytes"][m["offset"]:m["offset"] + m["csize"]]) for m in z["members"]]


def test_fixture_classes():
    cls = [(e["class"], e["level"]) for e in G["entries"]]
    assert [c for c in cls if c[0] == "a"] == [("a", 1), ("a", 6), ("a", 9)]
    assert sorted(c for c in cls if c[0] == "b") == [("b", lv) for lv in (3, 3, 4, 4, 6, 6, 9, 9)]
    assert sorted(c for c in cls if c[0] == "d") == [("d", 1), ("d", 2), ("d", 6)]
    assert sum(c[0] == "c" for c in cls) >= 1 and sum(c[0] == "e" for c in cls) == 1 and len(TAILS) == 2
    assert len(G["zip"]["members"]) == 3 and "gzip" in G["versions"]["gzip"] and "Zip" in G["versions"]["zip"]
    size = os.path.getsize(zgnu.GOLDEN) + os.path.getsize(zgnu.GOLDEN[:-5] + ".bin")
    assert size < os.path.getsize(os.path.join(ROOT, "tests", "golden", "inflate_edges.json"))


def check(body, level, blocks_want):
    blocks, data, used = zgnu.tokenize(body)
    assert used == len(body) and data == zlib.decompress(body, -15)
    toks = zgnu.flat_tokens(blocks, data)
    zb, zd, _ = zgnu.tokenize(zlib_raw(data, level))
    assert zd == data and toks == zgnu.flat_tokens(zb, data)   # zlib's parse
    trace = []
    assert zgnu.gnu_blocks(toks, level, trace) == zgnu.symbol_counts(blocks) == blocks_want   # the rule's blocks
    return blocks, trace


@pytest.mark.parametrize("e", AF, ids=ident)
def test_tokens_are_zlibs_and_blocks_the_models(e):
    blocks, trace = check(e["body"], e["level"], e["blocks"])
    counts = e["blocks"]
    fires = [t[1] < t[0] // 2 and t[2] < t[3] // 2 for t in trace]
    if e["class"] == "a":
        assert sum(counts) < 4096 and e["body"] == zlib_raw(zlib.decompress(e["body"], -15), e["level"])
    elif e["class"] == "b":   # one evaluation at 4 096 symbols, decided by at most two bytes
        last_lit, last_dist, out, inl = trace[0]
        assert last_lit == 4096 and last_dist < 2048
        if e["note"].startswith("pass"):
            assert 0 < inl // 2 - out <= 2 and counts[0] == 4096
        else:
            assert 0 <= out - inl // 2 <= 2 and counts[0] == 8192 and fires[:2] == [False, True]
    elif e["class"] == "c":
        assert fires[:3] == [True, False, False] or fires[:2] == [False, True]
    elif e["class"] == "d":
        assert counts[0] == 32767 and not any(fires) and bool(trace) == (e["level"] > 2)
    else:
        types = [b["btype"] for b in blocks]
        assert 0 in types[1:-1] and types[0] == 2 and types[-1] == 2


def test_zip_members_are_the_same_family():
    for m, body in zip_members():
        check(body, m["level"], m["blocks"])
        assert m["blocks"][0] == 4096


@pytest.mark.parametrize("e", TAILS, ids=ident)
def test_tails_differ_only_at_the_end(e):
    """Not modelled: GNU's longest_match compares past the end of input.  The difference stays in the last 258
    positions, so such a stream is a near miss for the diff list."""
    blocks, data, _ = zgnu.tokenize(e["body"])
    a = zgnu.flat_tokens(blocks, data)
    zb, _, _ = zgnu.tokenize(zlib_raw(data, e["level"]))
    b = zgnu.flat_tokens(zb, data)
    assert a != b
    k = 0
    while a[k] == b[k]:
        k += 1
    assert a[k][0] >= len(data) - 258 and b[k][0] >= len(data) - 258


def test_rule_edges():
    lit = lambda p: (p, 0, 65)
    # levels 1 and 2 never evaluate; the buffer's flush comes at 32 767 symbols, and an exact fit leaves an empty block
    toks = [lit(p) for p in range(40000)]
    assert zgnu.gnu_blocks(toks, 1) == zgnu.gnu_blocks(toks, 6) == [32767, 7233]
    assert zgnu.gnu_blocks(toks[:32767], 2) == [32767, 0]
    # 40 long matches, then literals: fires at 4 096 symbols for level 3 on, never for levels 1 and 2
    run = [(258 * k, 258, 1) for k in range(40)] + [lit(10320 + p) for p in range(4057)]
    assert zgnu.gnu_blocks(run, 2) == [4097] and zgnu.gnu_blocks(run, 3) == zgnu.gnu_blocks(run, 4) == [4096, 1]
    # the one-step-late tally: 17 matches of distance 1 give out = (4096 * 8 + 17 * 5) >> 3 = 4106, and the 4 096th
    # symbol, a literal, starts at q = 2 * out + 1: in / 2 = out for deflate_fast (strstart = q), out + 1 for the lazy parse
    toks, p = [], 0
    for ln in [258] * 16 + [7] + [0] * (4096 - 17):
        toks.append((p, ln, 1) if ln else lit(p))
        p += ln if ln else 1
    assert toks[-1][0] == 2 * 4106 + 1
    toks.append(lit(p))
    assert zgnu.gnu_blocks(toks, 3) == [4097] and zgnu.gnu_blocks(toks, 4) == [4096, 1]
    # half the symbols matches: never fires
    toks, p = [], 0
    for k in range(4096):
        toks.append((p, 258, 1) if k & 1 else lit(p))
        p += 258 if k & 1 else 1
    assert zgnu.gnu_blocks(toks + [lit(p)], 6) == [4097]


def test_list_order():
    for hint in (0, 1, 2):
        plain, gnu = zgnu.candidates(hint, False), zgnu.candidates(hint, True)
        assert plain == zraw.candidates(hint) and len(plain) == 90 and len(gnu) == 99 == len(set(gnu))
        assert gnu[:10] == plain[:10] and gnu[19:] == plain[10:]
        assert [lv for lv, _, m in gnu[10:19]] == [lv for lv in zgnu.LEVELS[hint] if lv]
        assert all(w == 15 and m == 0 for _, w, m in gnu[10:19])
    assert [lv for lv, _, _ in zgnu.candidates(0, True)[10:19]] == [6, 9, 1, 5, 7, 8, 4, 3, 2]
    assert zgnu.packed((6, 15, 0)) == (1 << 28) | (6 << 16) | (15 << 8)


def test_header_and_exports():
    import antiz_amd
    with open(os.path.join(ROOT, "include", "atz_accel.h")) as f:
        assert "int atz_set_deflaters(atz_ctx_t *ctx, uint32_t mask);" in f.read()
    assert "atz_set_deflaters" in antiz_amd.EXPORTS
    assert getattr(C.CDLL(antiz_amd.LIB_PATH), "atz_set_deflaters")


def test_deflater_mask():
    import antiz_amd
    assert antiz_amd.DEFLATERS == {"gnu": 0}
    assert antiz_amd.deflater_mask(()) == 0 == antiz_amd.deflater_mask("")
    assert antiz_amd.deflater_mask(("gnu",)) == 1 == antiz_amd.deflater_mask("gnu")
    for bad in ("zlib", "gnu,7zip", ("GNU",)):
        with pytest.raises(ValueError):
            antiz_amd.deflater_mask(bad)
