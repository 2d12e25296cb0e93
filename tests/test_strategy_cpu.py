"""CPU-side checks of the strategy extension: the two new entry points are exported,
the ATZ2 clevel byte packs and unpacks, the candidate lists have the documented shape, and -- as
information -- whether the interpreter's zlib agrees with the reference's zlib 1.2.8 under each strategy."""
import re
import subprocess
import zlib

import pytest

import antiz_amd
from antiz_amd import build as B

import zstrat


def test_new_symbols_are_exported():
    B.build()
    out = subprocess.run(["nm", "-D", "--defined-only", B.LIB], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (atz_\w+)", out))
    for name in ("atz_deflate_batch_ex", "atz_set_strategies"):
        assert name in exported and name in antiz_amd.EXPORTS


def test_clevel_byte_round_trips():
    seen = set()
    for strat in range(4):
        for lv in range(10):
            if strat >= 2 and lv == 0:
                with pytest.raises(ValueError):
                    antiz_amd.pack_clevel(strat, lv)
                continue
            b = antiz_amd.pack_clevel(strat, lv)
            assert 0 <= b < 256 and b not in seen
            seen.add(b)
            assert antiz_amd.unpack_clevel(b) == (strat, lv)
            assert (b <= 9) == (strat == 0)   # an ATZ1 reader's check (c > 9) refuses every strategy byte
    for bad in ((4, 6), (1, 10), (-1, 6)):
        with pytest.raises(ValueError):
            antiz_amd.pack_clevel(*bad)


def test_strategy_mask_words():
    assert antiz_amd.strategy_mask(()) == 0 and antiz_amd.strategy_mask("") == 0
    assert antiz_amd.strategy_mask(("filtered", "rle", "huffman")) == 14
    assert antiz_amd.strategy_mask("rle,filtered") == 10
    with pytest.raises(ValueError):
        antiz_amd.strategy_mask("filtered,lzma")


def test_candidate_lists():
    counts = {0x01: 18, 0x5e: 18, 0x9c: 9, 0xda: 27}   # FLEVEL 0..3 at windowBits 15
    for flg, n in counts.items():
        cands = zstrat.candidates(bytes([0x78, flg]), 14)
        assert len(cands) == n and len(set(cands)) == n
        assert all(w == 15 for _, _, w, _ in cands)
        first = [m for st, _, _, m in cands if st == cands[0][0]]
        assert list(dict.fromkeys(first)) == list(zstrat.MEMLEVELS)   # memLevel 8, 9, 7..1, levels inside
    assert [c[0] for c in zstrat.candidates(b"\x78\x01", 14)] == [3] * 9 + [2] * 9
    assert zstrat.candidates(b"\x78\x01", 1 << 2) == [(2, 6, 15, m) for m in zstrat.MEMLEVELS]
    assert zstrat.candidates(b"\x78\xda", 1 << 3) == []
    assert [c[1] for c in zstrat.candidates(b"\x48\xda", 2)[:3]] == [9, 8, 7] and zstrat.candidates(b"\x48\xda", 2)[0][2] == 12


def test_header_flevel_follows_the_strategy():
    d = b"abcabcabcabc" * 40
    for lv, want in ((1, 0), (4, 1), (6, 2), (9, 3)):
        assert zstrat.deflate(d, lv, 15, 8, zstrat.Z_FILTERED)[1] >> 6 == want
        assert zstrat.deflate(d, lv, 15, 8, zstrat.Z_RLE)[1] >> 6 == 0
        assert zstrat.deflate(d, lv, 15, 8, zstrat.Z_HUFFMAN_ONLY)[1] >> 6 == 0


@pytest.mark.parametrize("strategy", [zstrat.Z_FILTERED, zstrat.Z_HUFFMAN_ONLY, zstrat.Z_RLE], ids=lambda s: zstrat.NAMES[s])
def test_system_zlib_against_1_2_8(strategy):
    """Information only: the tests take their expected bytes from libz128 whatever this shows."""
    d = b"abcabcabcabcabd" * 30 + b"z" * 300 + bytes(range(256))
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, strategy)
    mine = co.compress(d) + co.flush()
    if mine != zstrat.deflate(d, 6, 15, 8, strategy):
        pytest.xfail("zlib %s differs from 1.2.8 under %s" % (zlib.ZLIB_RUNTIME_VERSION, zstrat.NAMES[strategy]))
