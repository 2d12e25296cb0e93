"""The block-boundary inputs (tests/blockedges.py) on the CPU: the oracle gives the real zlib 1.2.8's and the real
reference's results (tests/golden/blockedges.json) on every item and file, and the inputs are what they are named
for -- the premises below are read off the oracle's streams with edges.walk_symbols, so an input that stopped
standing on its block boundary (another seed, another text, a stale tuned triple) fails here and not silently on
the GPU."""
import functools
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor

import _libs
import blockedges as B
import edges as E
import nearmiss


def sha(b):
    return hashlib.sha256(b).hexdigest()


@functools.lru_cache(maxsize=None)
def streams():
    """The oracle's stream of every item of blockedges.items(), by position."""
    return [_libs.ora_deflate(it.data, it.level, it.window, it.memlevel)[0] for it in B.items()]


@functools.lru_cache(maxsize=None)
def blocks():
    return [E.walk_symbols(s) for s in streams()]


@functools.lru_cache(maxsize=None)
def oracle_runs():
    """{(family, setting): (ATZ1, stats)} of the oracle; it runs outside the interpreter lock."""
    jobs = [(fam, s) for fam in B.FAMILIES for s in B.settings_of(fam)]

    def run(job):
        rc, atz, st = _libs.ora_precompress(B.files()[job[0]][0], **nearmiss.flags_kwargs(B.SETTINGS[job[1]]))
        assert rc == 0, job
        return atz, st

    with ThreadPoolExecutor(4) as ex:
        return dict(zip(jobs, ex.map(run, jobs)))


# ---- the generator ----------------------------------------------------------------------------------
def test_generator_counts_and_dropped_share():
    """The families have the sizes the generator defines, every B1 / B3 length is a listed one, every listed
    (memLevel, target, level, ending) of B2 is there unless its target was dropped, and at most 2 % of the B2
    targets (and of B3's) were dropped."""
    assert (B.N_B1, B.N_B2_TARGETS, B.N_B3_PLAIN, B.N_B3_TARGETS) == (1280, 576, 640, 288)
    tl, tr = B.target_list(), B.tuned()
    assert len(tl) == len(tr) == 864
    for fam, total in (("B2", 576), ("B3", 288)):
        dropped = sum(t[0] == fam and x is None for t, x in zip(tl, tr))
        print("%s: %d of %d targets dropped" % (fam, dropped, total))
        assert dropped <= 0.02 * total, (fam, dropped)
    assert B.fixture()["unreached"] <= sum(x is None for x in tr)
    n2 = sum(t[0] == "B2" and x is not None for t, x in zip(tl, tr))
    n3 = sum(t[0] == "B3" and x is not None for t, x in zip(tl, tr))
    assert [len(B.family(f)) for f in B.FAMILIES] == [1280, n2, 640 + n3]
    assert B.fixture()["seed"] == B.SEED and len(B.fixture()["deflate"]) == len(B.items())
    for m in range(1, 10):
        L = 1 << (m + 6)
        P, P3 = max(1024, 2 * L), max(3072, 2 * L)
        want = {L - 2, L - 1, L, L + 1, 2 * (L - 1), 2 * (L - 1) + 1, 4 * (L - 1), 4 * (L - 1) + 1} | \
            set(range(P - 1, P + 4)) | set(range(P3 - 1, P3 + 4))
        for tag in ("uniq3", "skew3"):
            mine = [it for _, it in B.family("B1") if it.memlevel == m and it.tag == tag]
            assert {len(it.data) for it in mine} == {n for n in want if n <= 70000}, (m, tag)
            assert {it.level for it in mine} == {1, 3, 4, 6, 9} and {it.window for it in mine} == {15}
    for _, it in B.family("B2"):
        L = 1 << (it.memlevel + 6)
        assert it.target in (L - 2, L - 1, L, 2 * (L - 1), 2 * (L - 1) + 1, 4 * (L - 1)) and it.window == 15
        assert it.level in (1, 2, 3, 4, 6, 9) and 1 <= it.memlevel <= 8
    for w, ms in ((10, (1, 2, 3, 4)), (12, (3, 4, 5, 6))):
        mine = [it for _, it in B.family("B3") if it.window == w]
        assert {it.memlevel for it in mine} == set(ms)
        assert {B.regime(it) for it in mine} == {"unchecked", "checked", "slides"}
        for tag in ("uniq3", "skew3", "tuned"):    # every content reaches every regime at this window
            assert {B.regime(it) for it in mine if it.tag == tag} == {"unchecked", "checked", "slides"}, (w, tag)
    assert all(len(it.data) <= 70000 for it in B.items() if it.tag != "tuned")


# ---- premises ---------------------------------------------------------------------------------------
def test_plain_streams_have_no_match():
    """B1 and the plain part of B3: n literals at every level.  Every B1 uniq3 block of 100 literals and more is
    stored, so the flush position is in the output -- but for the second full block at memLevel 9, which starts one
    byte below the window after the slide and is dynamic (zlib cannot store it); skew3 is never stored."""
    n = 0
    for k, it in enumerate(B.items()):
        if it.tag == "tuned":
            continue
        bl = blocks()[k]
        assert not any(b.matches for b in bl) and sum(b.nlit for b in bl) == len(it.data) == it.target, B.E.label(it)
        if it.tag == "uniq3" and it.family == "B1":
            slid = it.memlevel == 9 and len(it.data) >= 2 * 32767
            assert all(b.btype == (2 if slid and i == 1 else 0) for i, b in enumerate(bl) if b.nlit >= 100), B.E.label(it)
            assert any(b.btype == 0 for b in bl)
            n += 1
        if it.tag == "skew3":
            assert all(b.btype != 0 for b in bl), B.E.label(it)
    assert n == 640


def test_tuned_streams_have_exactly_t_symbols():
    """B2 and the tuned part of B3: no stored block, exactly T symbols, matches among them, and the last symbol is
    what the item says."""
    n = 0
    for k, it in enumerate(B.items()):
        if it.tag != "tuned":
            continue
        got = B.symbols(streams()[k])
        assert got == (it.target, it.ending == "match"), (B.E.label(it), it.target, it.ending, got)
        nm = sum(len(b.matches) for b in blocks()[k])
        assert nm >= (it.ending == "match") and (it.target < 1000 or nm >= it.target // 50), (B.E.label(it), nm)
        n += 1
    assert n == sum(x is not None for x in B.tuned())
    endings = {(it.memlevel, it.target, it.ending) for _, it in B.family("B2")}
    assert len(endings) >= 2 * 6 * 8 - 4       # both endings of (nearly) every (memLevel, T)


def test_block_model():
    """Every stream's per-block symbol counts are blockedges.model_blocks(): full blocks of L - 1 symbols and a last
    one, empty after deflate_fast or a final match when T is a multiple of L - 1, full after deflate_slow's pending
    literal."""
    seen = set()
    for k, it in enumerate(B.items()):
        bl = blocks()[k]
        assert [b.final for b in bl] == [0] * (len(bl) - 1) + [1]
        counts = [b.nlit + len(b.matches) for b in bl]
        assert counts == B.model_blocks(it.target, it.level, it.memlevel, it.ending), (B.E.label(it), it.target, it.ending)
        full = (1 << (it.memlevel + 6)) - 1
        if it.target % full == 0:
            seen.add((it.level > 3, it.ending, counts[-1] == 0))
    # an exact multiple ends in an empty block except after deflate_slow's pending literal
    assert seen == {(False, "match", True), (False, "literal", True), (True, "match", True), (True, "literal", False)}


# ---- the oracle equals the fixture ------------------------------------------------------------------
def test_oracle_equals_fixture_on_every_item():
    fx = B.fixture()["deflate"]
    bad = [(k, B.E.label(it)) for k, (it, s) in enumerate(zip(B.items(), streams())) if [len(s), E.sha16(s)] != fx[k]]
    assert not bad, bad[:10]


def test_oracle_equals_fixture_on_every_file():
    """Every file x setting: the oracle's ATZ1 is the reference's (SHA-256, length, recompressed count), its default
    stream table is the reference's, every generated stream is found at its offset and reproduced exactly
    (ident == comp_len, no diffs), and the corpus keeps its size limit."""
    fx = B.fixture()["files"]
    assert sum(len(d) for d, _ in B.files().values()) < 16 << 20
    for fam in B.FAMILIES:
        data, recs = B.files()[fam]
        assert (sha(data), len(data), len(recs)) == (fx[fam]["input_sha256"], fx[fam]["input_bytes"], fx[fam]["n_streams"])
        assert sorted(fx[fam]["runs"]) == sorted(B.settings_of(fam))
        for s in B.settings_of(fam):
            atz, st = oracle_runs()[(fam, s)]
            e = fx[fam]["runs"][s]
            tail = "recompressed:%d/%d" % (sum(x["recomp"] for x in st["streams"]), len(st["streams"]))
            assert (sha(atz), len(atz), tail) == (e["atz_sha256"], e["atz_bytes"], e["tail"]), (fam, s)
            by = {x["offset"]: x for x in st["streams"]}
            for off, n, k, infl in recs:
                x = by[off]
                assert (x["comp_len"], x["infl_len"], x["recomp"], x["n_diff"], x["ident"]) == (n, infl, 1, 0, n), \
                    (fam, s, B.E.label(B.items()[k]))
        atz, st = oracle_runs()[(fam, "default")]
        table = [[x[k] for k in ("offset", "comp_len", "c", "w", "m", "n_diff", "first_diff")] for x in nearmiss.parse_atz1(atz)]
        assert table == fx[fam]["table"]
        assert table == [[x["offset"], x["comp_len"], x["clevel"], x["window"], x["memlevel"], x["n_diff"],
                          x["first_diff"] if x["n_diff"] else -1] for x in st["streams"] if x["recomp"]]
        assert _libs.ora_reconstruct(atz) == (0, data)


def test_files_hold_every_regime():
    """What the GPU tests' counter conditions rest on: each file has streams a sweep may replay unchecked (at most
    MAX_DIST bytes), streams it may replay only checked, and streams longer than every trial's table prefix."""
    for fam in B.FAMILIES:
        its = [B.items()[k] for _, _, k, _ in B.files()[fam][1]]
        assert {"unchecked", "checked"} <= {B.regime(it) for it in its}, fam
        assert any(len(it.data) > B.prefix(9, 3072) for it in its) or fam == "B3"        # past every trial's prefix
        assert any(len(it.data) > B.prefix(it.memlevel, 3072) for it in its), fam         # past its own memLevel's
    assert "slides" in {B.regime(B.items()[k]) for _, _, k, _ in B.files()["B3"][1]}


# ---- the fixture is the reference's -----------------------------------------------------------------
def test_fixture_is_the_reference_on_a_sample():
    """Where the reference build is there (oracle/_ref): the real zlib gives the fixture's stream on every 7th item,
    the tuning finds the recorded triple on every 24th target, and oracle/_ref/uncomp the recorded default ATZ1 of
    the smallest file."""
    if not (_libs.have_zref() and os.path.exists(_libs.REF_UNCOMP)):
        return
    fx = B.fixture()
    for k, it in list(enumerate(B.items()))[::7]:
        s = _libs.zref_deflate(it.data, it.level, it.window, it.memlevel)
        assert [len(s), E.sha16(s)] == fx["deflate"][k], B.E.label(it)
    for k, t in list(enumerate(B.target_list()))[::24]:
        if fx["tuned"][k] is not None:
            assert list(B.tune(k, t)) == fx["tuned"][k], t
    import sys
    sys.path.insert(0, os.path.dirname(B.FIXTURE))
    import make_blockedges
    atz, tail = make_blockedges.ref_run(B.files()["B3"][0], [])
    e = fx["files"]["B3"]["runs"]["default"]
    assert (sha(atz), len(atz), tail) == (e["atz_sha256"], e["atz_bytes"], e["tail"])
