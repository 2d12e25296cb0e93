"""The stitch extension's host-side surface and its Python model, without a GPU."""
import ctypes as C
import random
import struct
import zlib

import pytest

import _libs
import zpng
import zstrat


def test_exports_are_listed():
    import antiz_amd
    L = C.CDLL(antiz_amd.LIB_PATH)
    for name in ("atz_set_stitch", "atz_stitch_anchors", "atz_stitch_pieces"):
        assert name in antiz_amd.EXPORTS
        assert getattr(L, name)


def test_stitch_mask():
    import antiz_amd
    assert antiz_amd.STITCHERS == {"png": 0}
    assert antiz_amd.CONTAINERS == {"zip": 0, "gzip": 1}   # the stitch switch is no bit of the container mask
    assert antiz_amd.stitch_mask(()) == 0 and antiz_amd.stitch_mask("") == 0
    assert antiz_amd.stitch_mask(("png",)) == 1 and antiz_amd.stitch_mask("png") == 1 and antiz_amd.stitch_mask("png,png") == 1
    for bad in ("apng", "png,zip", ("PNG",)):
        with pytest.raises(ValueError):
            antiz_amd.stitch_mask(bad)
    with pytest.raises(ValueError):
        antiz_amd.container_mask("png")


def test_clevel_bytes_of_versions_3_and_4():
    import antiz_amd
    v3 = set()
    for raw in (False, True):
        for strat in range(4):
            for lv in range(1 if strat >= 2 else 0, 10):
                b = antiz_amd.pack_clevel(strat, lv, raw)
                assert antiz_amd.pack_clevel4(strat, lv, raw) == b   # not stitched: the version 3 byte
                assert antiz_amd.unpack_clevel4(b) == (False, raw, strat, lv)
                assert antiz_amd.unpack_clevel3(b) == (raw, strat, lv)
                v3.add(b)
    assert len(v3) == 76 and max(v3) < 128
    stitched = set()
    for strat in range(4):
        for lv in range(1 if strat >= 2 else 0, 10):
            b = antiz_amd.pack_clevel4(strat, lv, stitched=True)
            assert b == 0x80 | antiz_amd.pack_clevel(strat, lv)
            assert antiz_amd.unpack_clevel4(b) == (True, False, strat, lv)
            stitched.add(b)
            with pytest.raises(ValueError):
                antiz_amd.pack_clevel4(strat, lv, raw=True, stitched=True)
    # a stitched byte is none of version 3's, and never carries bit 6
    assert len(stitched) == 38 and not stitched & v3 and all(b & 0x80 and not b & 0x40 for b in stitched)


def test_header_types():
    seen = {}
    for b0 in range(256):
        for b1 in range(256):
            t = zpng.header_type(b0, b1)
            if t >= 0:
                seen[t] = (b0, b1)
    assert sorted(seen) == list(range(24))
    assert seen[22] == (0x78, 0x9c) and seen[0] == (0x28, 0x15) and seen[19] == (0x68, 0xde)
    for lv, w, flevel in ((1, 15, 0), (4, 13, 1), (6, 15, 2), (9, 10, 3)):   # what zlib 1.2.8 writes
        s = zstrat.deflate(b"abc" * 50, lv, w, 8, 0)
        assert zpng.header_type(s[0], s[1]) == (w - 10) * 4 + flevel


def build(stream, lens, junk=b""):
    return zpng.png(stream + junk, lens)


def test_model_on_hand_built_files():
    """The model's own pieces agree with each other: a built chain is found chunk by chunk, joined, accepted, and
    its pieces, hull, descriptor and residue put the file together again."""
    payload = _libs.text(random.Random(4), 9000)
    stream = zstrat.deflate(payload, 6, 15, 8, 0)
    n = len(stream)
    assert zlib.decompress(stream) == payload and n > 2000
    for lens, junk in (([1, n - 1], b""), ([n - 1, 1], b""), ([n - 3, 3], b""), ([1000, 0, n - 1000], b""),
                       ([0, 0, 700, n - 700], b""), ([1] * 40 + [n - 40], b""), ([900, n - 900 + 57], bytes(57)),
                       (zpng.split(n, 1024), b"")):
        data, first = build(stream, lens, junk)
        anch = zpng.anchors(data)
        assert len(anch) == len(lens) and anch[0] == first - 4
        ch, = zpng.chains(data)
        assert [x for _, x in ch] == lens
        (cch, t), = zpng.candidates(data)
        assert t == 22 and [x for _, x in cch] == [x for x in lens][next(i for i, x in enumerate(lens) if x):]
        (rec,), dropped = zpng.stitched_records(data)
        assert not dropped
        assert (rec["comp_len"], rec["infl_len"], rec["stream"], rec["payload"]) == (n, len(payload), stream, payload)
        pcs = rec["pieces"]
        assert len(pcs) >= 2 and pcs[0][1] >= 1 and pcs[-1][1] >= 1 and sum(x for _, x in pcs) == n
        assert rec["offset"] == pcs[0][0] == cch[0][0]
        for k in range(1, len(pcs)):   # piece i starts 12 framing bytes behind the end of piece i - 1
            assert pcs[k][0] == pcs[k - 1][0] + pcs[k - 1][1] + 12
        assert b"".join(data[o:o + x] for o, x in pcs) == stream
        assert zpng.hull(pcs) == n + 12 * (len(pcs) - 1) and rec["offset"] + zpng.hull(pcs) <= len(data)
        # the descriptor and the residue hold the file: scatter the stream, fill the gaps
        d = zpng.descriptor(rec, 6, 15, 8)
        assert d[24] == 0x86 and len(d) == 35 + len(payload) + 4 + 4 * len(pcs)
        assert struct.unpack_from("<I", d, 35 + len(payload))[0] == len(pcs)
        res = zpng.residue(data, pcs)
        assert len(res) == len(data) - n
        back, ri = bytearray(), 0
        for o, x in pcs:
            gap = o - len(back)
            back += res[ri:ri + gap] + data[o:o + x]
            ri += gap
        back += res[ri:]
        assert bytes(back) == data
        # a record made before that meets the hull drops it; one that only touches its ends does not
        lo, hi = rec["offset"], rec["offset"] + zpng.hull(pcs)
        assert zpng.stitched_records(data, [(pcs[1][0] - 6, 3)]) == ([], [rec])   # inside the framing
        assert zpng.stitched_records(data, [(lo - 5, 5), (hi, 9)]) == ([rec], [])
        # the flat twin holds the same stream in one chunk, where the plain scan finds it
        twin, where = zpng.flat_twin(data)
        assert len(zpng.anchors(twin)) == 1 and twin[where[rec["offset"]]:][:n] == stream
        assert zpng.stitched_records(twin) == ([], [])
    # a stream that ends inside its first chunk, one chunk alone, no zlib header, a broken Adler-32
    for data in (build(stream, [n + 5, 20], bytes(25))[0], build(stream, [n])[0],
                 build(b"\x78\x9d" + stream[2:], [5, n - 5])[0], build(stream[:-1] + bytes([stream[-1] ^ 1]), [5, n - 5])[0]):
        assert zpng.stitched_records(data) == ([], [])


def test_cursor_walk_never_gathers_more_than_the_file():
    """Fake IDAT type fields inside a payload, each with a length that would reach far over the chunks behind it:
    the cursor skips every anchor inside a chain, so the chains are disjoint."""
    r = random.Random(11)
    inner = bytearray(r.randbytes(6000))
    spots = list(range(100, 5900, 97))
    for k, at in enumerate(spots):   # nested anchors: each claims everything up to a later real chunk end
        inner[at:at + 8] = struct.pack(">I", 5000 - k) + b"IDAT"
    stream = zstrat.deflate(bytes(inner), 0, 15, 8, 0)   # stored: the fake fields survive into the stream
    assert stream.count(b"IDAT") >= len(spots)
    tail = zstrat.deflate(_libs.text(r, 20000), 6, 15, 8, 0)
    data = zpng.png(stream, zpng.split(len(stream), 512))[0] + zpng.png(tail, zpng.split(len(tail), 2048))[0] + bytes(9000)
    anch = zpng.anchors(data)
    inside = [a for a in anch if struct.unpack_from(">I", data, a - 4)[0] > 4000]
    assert len(inside) >= 30   # fake anchors that pass the kernel's rule
    chs = zpng.chains(data)
    spans = sorted((ch[0][0], ch[-1][0] + ch[-1][1]) for ch in chs)
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0
    assert sum(n for ch in chs for _, n in ch) <= len(data)
    assert zpng.gathered_bytes(data) <= len(data)
    # without the cursor (every anchor starts a chain) the same file would gather more than its size
    assert sum(struct.unpack_from(">I", data, a - 4)[0] for a in anch) > len(data)
    kept, dropped = zpng.stitched_records(data)
    assert [x["comp_len"] for x in kept] == [len(stream), len(tail)] and not dropped
