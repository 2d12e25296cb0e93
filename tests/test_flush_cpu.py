"""The segment extension's premises and model on the CPU, against the reference's zlib 1.2.8:
P1 a full-flushed stream is the concatenation of independent deflates of its segments; P2 a flushed segment has
the blocks and tokens of the finishing deflate of the same bytes, but for its end; the model's decoder and chain
rule (tests/zflush.py); the mask parser."""
import random
import zlib

import pytest

import _libs
import zflush
import zgnu
import zraw

LEVELS = range(10)


def rnd(seed, n):
    return random.Random(seed).randbytes(n)


def txt(seed, n):
    return _libs.text(random.Random(seed), n)


# ---- P1 ------------------------------------------------------------------------------------------------
TRIPLES = [("text", (300, 5000, 70000)), ("tiny", (1, 2, 3)), ("rand", (127, 254, 255)), ("full", (16383, 1, 32767)),
           ("stored-edge", (65535, 65536, 10))]


def triple(kind, sizes):
    gen = rnd if kind in ("rand", "full") else txt
    return [gen(40 + i, n) for i, n in enumerate(sizes)]


@pytest.mark.parametrize("memlevel", (1, 8, 9))
@pytest.mark.parametrize("level", LEVELS)
def test_p1_a_flushed_stream_is_its_segments_side_by_side(level, memlevel):
    for kind, sizes in TRIPLES:
        segs = triple(kind, sizes)
        stream, ends = zflush.flush_stream(segs, level, memlevel, -15)
        want = b"".join(zflush.flushed_deflate(s, level, memlevel) for s in segs[:-1]) + \
            zraw.raw_deflate(segs[-1], level, memlevel)
        assert stream == want, (kind, level, memlevel)
        assert ends[0] == len(zflush.flushed_deflate(segs[0], level, memlevel))


# ---- P2 ------------------------------------------------------------------------------------------------
def p2_inputs(level):
    common = [rnd(1, 127), rnd(2, 254), rnd(3, 255), rnd(4, 16383), rnd(5, 32767), txt(6, 5000)]
    # (levels 4-9 tally their last literal behind the parse loop, where no block ends: 127 literals are one block
    # there.  126 literals and a closing match put the block's end at the input's end for every level above 0.)
    r = rnd(9, 126)
    return common + ([txt(7, 65535), txt(8, 65536)] if level == 0 else [txt(7, 300), r + r[1:4]])   # (position 0 is zlib's NIL: never a match)


def p2_case(data, level, memlevel):
    """-> True when the finishing deflate's last block is empty (and so absent from the flushed segment)"""
    fin = zraw.raw_deflate(data, level, memlevel)
    flu = zflush.flushed_deflate(data, level, memlevel)
    fb, fout, fcons = zgnu.tokenize(fin)
    # (a final empty stored block behind the segment makes it a complete stream for the tokenizer)
    gb, gout, gcons = zgnu.tokenize(flu + b"\x01\x00\x00\xff\xff")
    assert fout == data and gout == data and fcons == len(fin) and gcons == len(flu) + 5
    assert flu[-4:] == zflush.MARKER
    mark, tail = gb[-2], gb[-1]
    assert (mark["btype"], mark["last"], mark["start"], mark["end"]) == (0, 0, len(data), len(data))
    assert (tail["btype"], tail["last"]) == (0, 1)
    gb = gb[:-2]
    assert all(b["last"] == 0 for b in gb)
    absent = fb[-1]["start"] == fb[-1]["end"]
    if absent:
        fb = fb[:-1]
    assert [(b["btype"], b["start"], b["end"], b["tokens"]) for b in fb] == \
        [(b["btype"], b["start"], b["end"], b["tokens"]) for b in gb], (level, memlevel, len(data))
    # three zero bits, padding, the marker: the segment is at most 1 + 4 bytes longer than its blocks
    st, consumed, out, am = zflush.seg_inflate(flu)
    assert (st, consumed, out, am) == (zflush.END, len(flu), data, True)
    return absent


@pytest.mark.parametrize("level", LEVELS)
def test_p2_a_flushed_segment_has_the_finishing_deflates_blocks(level):
    absent = 0
    for memlevel in (1, 2, 8, 9):
        for data in p2_inputs(level):
            absent += p2_case(data, level, memlevel)
    assert absent >= 1, "the grid lost the 'last block absent' case at level %d" % level


def test_p2_the_absent_block_cases():
    # the symbol count stands on a block boundary: 2^(memLevel + 6) - 1 literals under deflate_fast
    # (16 383 and 32 767 random bytes hold a few chance matches, so their counts fall short of a boundary)
    assert p2_case(rnd(1, 127), 1, 1) and p2_case(rnd(1, 127), 3, 1)
    assert p2_case(rnd(2, 254), 1, 1) and not p2_case(rnd(3, 255), 1, 1)   # 254 = 2 x 127
    # the lazy parse tallies its last literal behind the loop, where no block ends; a closing match ends one
    r = rnd(9, 126)
    assert not p2_case(rnd(1, 127), 6, 1) and p2_case(r + r[1:4], 6, 1)
    assert p2_case(txt(7, 65535), 0, 9)             # level 0: strstart == block_start after a full stored block
    assert not p2_case(txt(8, 65536), 0, 9)


# ---- the model's decoder -------------------------------------------------------------------------------
@pytest.mark.parametrize("level", (0, 1, 4, 6, 9))
def test_decoder_walks_whole_chains_as_zlib_does(level):
    segs = [txt(11, 300), rnd(12, 700), txt(13, 5000), txt(14, 40000)]
    stream, ends = zflush.flush_stream(segs, level, 8, -15)
    z = zlib.decompressobj(-15)
    assert z.decompress(stream) == b"".join(segs) and z.eof
    at, outs = 0, []
    for i, seg in enumerate(segs):
        st, consumed, out, am = zflush.seg_inflate(stream[at:])
        assert st == zflush.END and out == seg and am == (i < len(segs) - 1)
        at += consumed
        assert at == ends[i]
    assert at == len(stream)


def test_decoder_status():
    body = zflush.flushed_deflate(txt(15, 2000), 6, 8)
    for cut in (1, 2, 3, 4):   # a truncated marker needs input
        assert zflush.seg_inflate(body[:-cut])[0] == zflush.NEED
    assert zflush.seg_inflate(b"\x01\x00\x00\xff\xff") == (zflush.END, 5, b"", False)   # a final empty stored block
    assert zflush.seg_inflate(b"\x00\x00\x00\xff\xff") == (zflush.END, 5, b"", True)
    assert zflush.seg_inflate(b"\x00\x00\x00\xff\xfe")[0] == zflush.ERROR


# ---- the chain rule ------------------------------------------------------------------------------------
def raw_rec(pre, stream, n, typ=24):
    return (len(pre), typ, len(stream), n, 0)


def test_chain_completes_and_is_replaced():
    segs = [txt(21, 300), txt(22, 5000), txt(23, 7000)]
    stream, ends = zflush.flush_stream(segs, 6, 8, -15)
    pre = rnd(24, 100)
    data = pre + stream + rnd(25, 50)
    got = zflush.split(data, [raw_rec(pre, stream, 12300, 26)])
    at = [len(pre)] + [len(pre) + e for e in ends[:-1]]
    assert got == [(at[0], 26, ends[0], 300, 128), (at[1], 26, ends[1] - ends[0], 5000, 128),
                   (at[2], 26, ends[2] - ends[1], 7000, 0)]
    # a zlib parent: header and trailer leave the records; FLEVEL maps to the hint
    for level, typ in ((1, 25), (2, 25), (6, 24), (9, 26)):
        zs, ze = zflush.flush_stream(segs, level, 8, 15)
        data = pre + zs
        got = zflush.split(data, [(len(pre), 20 + (zs[1] >> 6), len(zs), 12300, 0)])
        assert [(r[1], r[3], r[4]) for r in got] == [(typ, 300, 128), (typ, 5000, 128), (typ, 7000, 0)]
        assert got[0][0] == len(pre) + 2 and got[-1][0] + got[-1][2] == len(data) - 4
        assert all(a[0] + a[2] == b[0] for a, b in zip(got, got[1:]))


def test_chains_that_do_not_complete():
    a, b = txt(31, 3000), txt(32, 4000)
    stream, ends = zflush.flush_stream([a, b], 6, 8, -15)
    rec = [(0, 24, len(stream), 7000, 0)]
    assert len(zflush.split(stream, rec)) == 2
    # a marker byte changed: the chain breaks, the record stays (whatever its decode now says)
    bad = bytearray(stream)
    bad[ends[0] - 1] = 0xfe
    assert zflush.split(bytes(bad), rec) == rec
    # the sum of the outputs is not the record's
    assert zflush.split(stream, [(0, 24, len(stream), 7001, 0)]) == [(0, 24, len(stream), 7001, 0)]
    # k = 1: a stored block whose payload holds the pattern makes the record eligible, and no more
    one = zraw.raw_deflate(rnd(33, 500) + zflush.MARKER + rnd(34, 500), 0, 8)
    assert zflush.markers(one) and zflush.split(one, [(0, 24, len(one), 1004, 0)]) == [(0, 24, len(one), 1004, 0)]
    # a zero-length middle segment breaks the chain
    fa = zflush.flushed_deflate(a, 6, 8)
    mid = fa + b"\x00" + zflush.MARKER + zraw.raw_deflate(b, 6, 8)
    assert zflush.seg_inflate(mid[len(fa):])[:2] == (zflush.END, 5)
    assert zflush.split(mid, [(0, 24, len(mid), 7000, 0)]) == [(0, 24, len(mid), 7000, 0)]
    # a zero-length final segment is allowed and makes no record
    fin = fa + b"\x03\x00"
    assert zlib.decompressobj(-15).decompress(fin) == a
    assert zflush.split(fin, [(0, 24, len(fin), 3000, 0)]) == [(0, 24, len(fa), 3000, 128)]
    # sync flush: the second segment's matches reach into the first
    sync, se = zflush.flush_stream([a, a], 6, 8, -15, zflush.Z_SYNC_FLUSH)
    assert sync[se[0] - 4:se[0]] == zflush.MARKER and zflush.seg_inflate(sync[se[0]:])[0] == zflush.ERROR
    assert zflush.split(sync, [(0, 24, len(sync), 6000, 0)]) == [(0, 24, len(sync), 6000, 0)]
    # other windows, stitched records and types past 26 are left alone
    z14, _ = zflush.flush_stream([a, b], 6, 8, 14)
    assert zflush.split(z14, [(0, 16 + (z14[1] >> 6), len(z14), 7000, 0)])[0][2] == len(z14)
    z15, _ = zflush.flush_stream([a, b], 6, 8, 15)
    assert zflush.split(z15, [(0, 22, len(z15), 7000, 64)]) == [(0, 22, len(z15), 7000, 64)]
    assert len(zflush.split(z15, [(0, 22, len(z15), 7000, 2)])) == 2


def test_a_stored_payload_that_ends_in_the_pattern_is_no_stop():
    a, b = rnd(41, 600) + zflush.MARKER, rnd(42, 300)
    stream, ends = zflush.flush_stream([a, b], 0, 8, -15)
    assert len(zflush.markers(stream)) == 2
    st, consumed, out, am = zflush.seg_inflate(stream)
    assert (st, consumed, out, am) == (zflush.END, ends[0], a, True)
    assert zflush.split(stream, [(0, 24, len(stream), 904, 0)]) == [(0, 24, ends[0], 604, 128),
                                                                    (ends[0], 24, ends[1] - ends[0], 300, 0)]


def test_markers():
    assert zflush.markers(b"") == [] and zflush.markers(zflush.MARKER[:3]) == []
    assert zflush.markers(zflush.MARKER * 2 + b"\x00\x00\xff") == [0, 4]
    assert zflush.markers(b"\x00" + zflush.MARKER) == [1]


def test_walk_rule_on_a_segment():
    data = txt(51, 3000)
    body = zflush.flushed_deflate(data, 4, 1)
    got = zflush.rule(body, data, 0, True)
    assert got is not None and (got["level"], got["memlevel"], got["diff_pos"]) == (4, 1, [])
    near = zflush.rule(body, data, 0, False)   # a finishing trial misses the segment's end
    assert near is None or near["diff_pos"]


# ---- the mask parser -----------------------------------------------------------------------------------
def test_segments_mask():
    import antiz_amd
    assert antiz_amd.segments_mask(()) == 0 and antiz_amd.segments_mask("") == 0
    assert antiz_amd.segments_mask(("flush",)) == 1 and antiz_amd.segments_mask("flush,") == 1
    with pytest.raises(ValueError):
        antiz_amd.segments_mask("flush,sync")
