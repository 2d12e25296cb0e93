"""The block-boundary inputs (tests/blockedges.py) on the MI355X, through the code that cuts blocks inside a sweep:
parse_replay re-cutting a saved symbol sequence into another memLevel's blocks, the replays that are not launched
at all (at most lit_bufsize - 2 symbols), multi-wave trials handing block after block to their flushers (the
slots wrap at the fourth block; an empty last block is a hand-over of no symbols), and trials that parse past their
match-table prefix and run again.  Everything is bit-exact against the real zlib 1.2.8 and the real reference
(tests/golden/blockedges.json, made by make_blockedges.py); tests/test_blockedges_cpu.py shows on the CPU that the
oracle gives the same and that every stream has the symbol count and the blocks it is named for.

The schedule switches (ATZ_MW, ATZ_REPLAY, ...) are read once per process, so each schedule runs in a process
of its own; a schedule's run is shared by the tests that read it."""
import functools
import hashlib
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import pytest

import _libs
import blockedges as B
import edges as E
import nearmiss

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULES = {"default": {}, "big": {"ATZ_PIPES": "3", "ATZ_MHINT": "1", "ATZ_PREFIX_MIN": "3072"},
             "mw4_deep": {"ATZ_MW": "4", "ATZ_TARGET": "16384"}, "mw0": {"ATZ_MW": "0"}, "mw9": {"ATZ_MW": "9"},
             "noreplay": {"ATZ_REPLAY": "0", "ATZ_DEDUP": "0"}, "replay3": {"ATZ_REPLAY": "3"},
             "target65536": {"ATZ_TARGET": "65536"}, "nostopflag": {"ATZ_STOPFLAG": "0"},
             "smallcaps": {"ATZ_CAP_DIV": "4096"}}
COUNTERS = ("n_trials_replayed", "n_replay_checked", "n_trials_duplicate", "n_trials_rerun")
CTX_NAMES = ("recomp_tresh", "sizediff_tresh", "shortcut_len", "mismatch_tol", "brute_window")

RUN = r"""
import hashlib, json, os, sys, time
sys.path.insert(0, %r)
import antiz_amd
d, settings = sys.argv[1], json.loads(sys.argv[2])
for name in sorted(settings):
    data = open(os.path.join(d, name + ".bin"), "rb").read()
    for sname, kw in settings[name].items():
        with antiz_amd.Context(device=0, **kw) as c:
            t0 = time.time()
            out, st = c.precompress(data)
            t1 = time.time()
            restored = c.reconstruct(out) == data
        print(json.dumps({"file": name, "setting": sname, "sha": hashlib.sha256(out).hexdigest(), "n": len(out),
                          "tail": "recompressed:%%d/%%d" %% (st["n_recomp"], st["n_streams"]), "restored": restored,
                          "seconds": round(t1 - t0, 3), "counters": {k: st[k] for k in %r}}), flush=True)
""" % (ROOT, COUNTERS)

KAT = r"""
import hashlib, json, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import antiz_amd
import blockedges as B
import edges as E
groups = [(f, [it for _, it in B.family(f)]) for f in B.FAMILIES] + [("D3", [it for _, it in E.family("D3")])]
with antiz_amd.Context(device=0) as c:
    for name, its in groups:
        outs = c.deflate_batch(*B.pack(its))
        print(json.dumps({"group": name, "rows": [[len(o), E.sha16(o)] for o in outs]}), flush=True)
""" % (ROOT, os.path.join(ROOT, "tests"))


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def atz():
    import antiz_amd
    from antiz_amd import build
    build.build()
    return antiz_amd


@pytest.fixture(scope="module")
def ctx(atz):
    with atz.Context(device=0) as c:
        yield c


def wanted(group):
    """(items, the fixture's [length, hash] per item) of a family of blockedges, or of edges' D3."""
    mod = E if group == "D3" else B
    pos, its = zip(*mod.family(group))
    fx = mod.fixture()["deflate"]
    return list(its), [fx[k] for k in pos]


def check(group, rows):
    its, want = wanted(group)
    assert len(rows) == len(its)
    bad = [k for k, (r, w) in enumerate(zip(rows, want)) if list(r) != w]
    print("%s: %d items, %d differ" % (group, len(its), len(bad)))
    report = ["%s T=%s ending=%s: lengths %d / %d" % (E.label(its[k]), getattr(its[k], "target", "-"),
                                                      getattr(its[k], "ending", "-"), rows[k][0], want[k][0]) for k in bad[:10]]
    assert not bad, "%d differ:\n%s" % (len(bad), "\n".join(report))


# ---- deflate ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", B.FAMILIES)
def test_deflate_kats(ctx, fam):
    """Every item of a family as one whole-stream trial, in one batch: zlib's bytes."""
    its, _ = wanted(fam)
    t0 = time.time()
    outs = ctx.deflate_batch(*B.pack(its))
    print("%s: deflate_batch %.2f s" % (fam, time.time() - t0))
    check(fam, [[len(o), E.sha16(o)] for o in outs])


@pytest.mark.parametrize("mw", ["0", "4", "9"])
def test_deflate_kats_multiwave(atz, mw):
    """The same items and the D3 items of tests/edges.py under ATZ_MW=0, 4 and 9: multi-wave trials at no memLevel,
    up to 4 and at every one -- blocks of exactly lit_bufsize - 1 symbols, the empty last block, streams of more
    than three blocks (the hand-over slots wrap) at memLevels 3-9, which the library's own choice for
    deflate_batch (memLevels 1-2) never runs multi-wave."""
    t0 = time.time()
    r = subprocess.run([sys.executable, "-u", "-c", KAT], env=dict(os.environ, ATZ_MW=mw), capture_output=True,
                       text=True, timeout=300)
    print("ATZ_MW=%s: %.2f s" % (mw, time.time() - t0))
    assert r.returncode == 0, r.stderr[-3000:]
    got = {g["group"]: g["rows"] for g in map(json.loads, (ln for ln in r.stdout.splitlines() if ln.startswith("{")))}
    assert sorted(got) == sorted(B.FAMILIES + ("D3",))
    for group in B.FAMILIES + ("D3",):
        check(group, got[group])


# ---- precompress ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("blockedges")
    for fam, (data, _) in B.files().items():
        (d / (fam + ".bin")).write_bytes(data)
    return str(d)


@functools.lru_cache(maxsize=None)
def schedule_run(name, corpus, fams=B.FAMILIES):
    """One process under SCHEDULES[name]: every file of `fams` x fixture setting -> [result dict]."""
    fx = B.fixture()
    for fam, (data, recs) in B.files().items():
        assert (sha(data), len(recs)) == (fx["files"][fam]["input_sha256"], fx["files"][fam]["n_streams"]), fam
    settings = {fam: {s: nearmiss.flags_kwargs(B.SETTINGS[s], CTX_NAMES) for s in B.settings_of(fam)} for fam in fams}
    t0 = time.time()
    r = subprocess.run([sys.executable, "-u", "-c", RUN, corpus, json.dumps(settings)],
                       env=dict(os.environ, **SCHEDULES[name]), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    print("%s: %.2f s; precompress seconds %s" % (name, time.time() - t0,
                                                  {g["file"] + "/" + g["setting"]: g["seconds"] for g in got}))
    return got


# a process per schedule; with the caps divided down a precompress takes a second, so there a process per file
CASES = [(s, B.FAMILIES) for s in SCHEDULES if s != "smallcaps"] + [("smallcaps", (fam,)) for fam in B.FAMILIES]


@pytest.mark.parametrize("schedule,fams", CASES, ids=[s if len(f) > 1 else s + "-" + f[0] for s, f in CASES])
def test_precompress_identical_to_reference(atz, corpus_dir, schedule, fams):
    """Every file x fixture setting under one schedule: the ATZ1's SHA-256, length and recompressed count are the
    reference's and reconstruct restores the file."""
    fx = B.fixture()["files"]
    got = schedule_run(schedule, corpus_dir, fams)
    assert [(g["file"], g["setting"]) for g in got] == [(fam, s) for fam in sorted(fams) for s in B.settings_of(fam)]
    bad = []
    for g in got:
        e = fx[g["file"]]["runs"][g["setting"]]
        if (g["sha"], g["n"], g["tail"]) != (e["atz_sha256"], e["atz_bytes"], e["tail"]) or not g["restored"]:
            bad.append((g["file"], g["setting"], g["tail"], e["tail"], g["n"], e["atz_bytes"], g["restored"]))
    assert not bad, "ATZ1 differs from the reference's under %s: %s" % (schedule, bad)


@pytest.mark.parametrize("fam", B.FAMILIES)
def test_sweep_takes_every_path(atz, corpus_dir, fam):
    """Conditions, not measurements: under the library's own schedule the sweep of each file replays saved
    sequences unchecked and checked, leaves duplicates unlaunched and reruns trials that parsed past their prefix;
    under ATZ_REPLAY=0 it replays nothing."""
    run = {(g["file"], g["setting"]): g["counters"] for g in schedule_run("default", corpus_dir, B.FAMILIES)}
    print(fam, run[(fam, "default")])
    for k in COUNTERS:
        assert run[(fam, "default")][k] > 0, (fam, k, run[(fam, "default")])
    off = {(g["file"], g["setting"]): g["counters"] for g in schedule_run("noreplay", corpus_dir, B.FAMILIES)}
    for s in B.settings_of(fam):
        assert off[(fam, s)]["n_trials_replayed"] == 0, (fam, s, off[(fam, s)])


# ---- scan and sweep ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle():
    """{(family, setting): the oracle's streams} for the default options and --mismatch-tol 0."""
    jobs = [(fam, s) for fam in B.FAMILIES for s in ("default", "tol0")]

    def run(job):
        rc, _, st = _libs.ora_precompress(B.files()[job[0]][0], **nearmiss.flags_kwargs(B.SETTINGS[job[1]]))
        assert rc == 0
        return st["streams"]

    with ThreadPoolExecutor(6) as ex:     # the oracle runs outside the interpreter lock
        return dict(zip(jobs, ex.map(run, jobs)))


@pytest.mark.parametrize("fam", B.FAMILIES)
def test_scan_and_sweep_match_oracle(atz, fam):
    """atz_scan + atz_sweep under the default options and --mismatch-tol 0: the stream table and each stream's
    (clevel, window, memlevel, ident, recomp, n_trials) -- the exact rule, with the number of trials it runs --
    are the oracle's, and every generated stream is reproduced whole."""
    data, recs = B.files()[fam]
    for s in ("default", "tol0"):
        ora = oracle()[(fam, s)]
        with atz.Context(device=0, **nearmiss.flags_kwargs(B.SETTINGS[s], CTX_NAMES)) as c:
            t0 = time.time()
            got = c.scan(data)
            assert [r[:4] for r in got] == [(x["offset"], x["type"], x["comp_len"], x["infl_len"]) for x in ora]
            res, diffs = c.sweep()
            print("%s %s: scan + sweep %.2f s, %d trials" % (fam, s, time.time() - t0, sum(r["n_trials"] for r in res)))
        keys = ("clevel", "window", "memlevel", "ident", "recomp", "n_trials")
        bad = [(x["offset"], [r[k] for k in keys], [x[k] for k in keys]) for r, x in zip(res, ora)
               if [r[k] for k in keys] != [x[k] for k in keys]]
        assert not bad and len(res) == len(ora), (s, len(bad), bad[:10])
        by = {x["offset"]: r for r, x in zip(res, ora)}
        assert all(by[off]["ident"] == n and by[off]["recomp"] == 1 and by[off]["n_diff"] == 0 for off, n, _, _ in recs)
        assert len(diffs[0]) == sum(x["n_diff"] for x in ora)
