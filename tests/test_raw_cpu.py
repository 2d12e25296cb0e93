"""The container extension's host-side surface and the premise its trial kernels rest on,
without a GPU: a raw deflate body of zlib 1.2.8 is its zlib stream without the 2-byte header and the
Adler-32 trailer."""
import ctypes as C
import random

import pytest

import _libs
import zraw
import zstrat


def test_exports_are_listed():
    import antiz_amd
    L = C.CDLL(antiz_amd.LIB_PATH)
    for name in ("atz_set_containers", "atz_container_anchors"):
        assert name in antiz_amd.EXPORTS
        assert getattr(L, name)


def test_container_mask():
    import antiz_amd
    assert antiz_amd.CONTAINERS == {"zip": 0, "gzip": 1}
    assert antiz_amd.container_mask(()) == 0 and antiz_amd.container_mask("") == 0
    assert antiz_amd.container_mask(("zip",)) == 1 and antiz_amd.container_mask("gzip") == 2
    assert antiz_amd.container_mask("zip,gzip") == 3 and antiz_amd.container_mask(["gzip", "zip"]) == 3
    for bad in ("rar", "zip,rar", ("gzip", "ZIP")):
        with pytest.raises(ValueError):
            antiz_amd.container_mask(bad)


def test_clevel_bytes():
    import antiz_amd
    atz2 = set()
    for strat in range(4):
        for lv in range(10):
            if strat >= 2 and lv < 1:
                with pytest.raises(ValueError):
                    antiz_amd.pack_clevel(strat, lv, raw=True)
                continue
            plain = antiz_amd.pack_clevel(strat, lv)
            assert plain == antiz_amd.pack_clevel(strat, lv, raw=False) == (strat << 4) | lv
            assert antiz_amd.unpack_clevel3(plain) == (False, strat, lv)
            atz2.add(plain)
    raws = set()
    for strat in range(4):
        for lv in range(1 if strat >= 2 else 0, 10):
            b = antiz_amd.pack_clevel(strat, lv, raw=True)
            assert antiz_amd.unpack_clevel3(b) == (True, strat, lv)
            assert b > 9 and b < 128 and b not in atz2
            raws.add(b)
    assert len(raws) == 38


@pytest.mark.parametrize("hint", [zraw.HINT_NONE, zraw.HINT_FAST, zraw.HINT_MAX])
def test_candidate_lists(hint):
    cands = zraw.candidates(hint)
    assert len(cands) == 90 == len(set(cands))
    assert [m for _, _, m in cands[::10]] == [8, 9, 7, 6, 5, 4, 3, 2, 1]
    order = {zraw.HINT_NONE: [6, 9, 1, 5, 7, 8, 4, 3, 2, 0], zraw.HINT_FAST: [1, 2, 3, 4, 5, 6, 7, 8, 9, 0],
             zraw.HINT_MAX: [9, 8, 7, 6, 5, 4, 3, 2, 1, 0]}[hint]
    for k in range(0, 90, 10):
        assert [lv for lv, _, _ in cands[k:k + 10]] == order
        assert {m for _, _, m in cands[k:k + 10]} == {cands[k][2]}
    assert {w for _, w, _ in cands} == {15}


@pytest.mark.parametrize("size", [0, 1, 5, 300, 5000, 40000])
def test_raw_body_is_the_stream_without_its_wrapper(size):
    """On the reference's zlib 1.2.8: deflate(d, lv, -15, m, st) == deflate(d, lv, 15, m, st)[2:-4], level 0
    (deflate_stored, blocks longer than the pending buffer at memLevel 1) included."""
    r = random.Random(size)
    data = _libs.text(r, size * 2 // 3) + r.randbytes(size - size * 2 // 3)
    for lv in range(10):
        for m in (1, 8, 9):
            for st in range(4):
                assert zstrat.deflate(data, lv, -15, m, st) == zstrat.deflate(data, lv, 15, m, st)[2:-4], (lv, m, st)


def test_model_on_hand_built_containers():
    """The model's own pieces agree with each other: a built entry is found, parsed, accepted and walked back
    to the parameters of its body's first reproducing candidate."""
    payload = _libs.text(random.Random(3), 3000)
    body = zraw.raw_deflate(payload, 6, 8)
    z = b"abc" + zraw.zip_entry(body, len(payload), name=b"a/b.txt", extra=b"\1\2\3\4", flags=zraw.ZIP_HINT_BITS[zraw.HINT_MAX])
    g = zraw.gzip_member(body, payload, name=b"f", xfl=zraw.GZIP_XFL[zraw.HINT_FAST])
    data = z + b"--" + g + b"tail"
    assert zraw.anchors(data, 3) == [(3, zraw.ZIP), (len(z) + 2, zraw.GZIP)]
    assert zraw.anchors(data, 1) == [(3, zraw.ZIP)] and zraw.anchors(data, 0) == []
    recs = zraw.raw_records(data, 3, [])
    assert recs == [(3 + 30 + 7 + 4, len(body), 3000, 26), (len(z) + 2 + 12, len(body), 3000, 25)]
    assert zraw.raw_records(data, 3, [(recs[0][0] + 5, 20)]) == recs[1:]
    for hint in (zraw.HINT_NONE, zraw.HINT_FAST, zraw.HINT_MAX):
        want = zraw.rule(body, payload, hint)
        assert want["ident"] == len(body) and want["diff_pos"] == [] and want["window"] == 15
