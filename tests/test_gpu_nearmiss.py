"""Near-miss streams (tests/nearmiss.py) on the MI355X: streams that a trial reproduces almost exactly.

They run what exact streams and hopeless ones never reach: k_diffs and the diff list over 1 to 128
mismatches deep in the stream and past the trial's end (the DiffJob sizing cap = C - ident and its
cross-check against the trial kernels' fused compare), the recompress threshold at C - ident = 127 / 128 /
129 against the eligibility floor, the first-improving rule over whole trial lists with
ties and successive improvements, the tolerance stop at exactly the number of diffs and one below (the
tolstop streams, where stopping changes the chosen trial; elsewhere through the trial counts that the sweep
test compares), the brute-window entry, sizediff_tresh at the exact size difference, and k_inflate on set
padding bits.

tests/golden/nearmiss.json holds the REAL reference's ATZ1 (SHA-256, length, recompressed count) of every
file under eleven settings (tools/make_nearmiss_golden.py); the generated corpus must be the fixture's byte
for byte (nearmiss.check_pinned).  The schedule switches are read once per process, so each
schedule runs in its own:
  default   the library's own choice
  big       ATZ_PIPES=3 ATZ_MHINT=1 ATZ_PREFIX_MIN=3072: the policies of a > 16 000-stream sweep
  mw4       ATZ_MW=4 ATZ_TARGET=16384: deep speculative rounds of multi-wave trials
  elig0     ATZ_ELIG=0: no eligibility floor
  noreplay  ATZ_REPLAY=0 ATZ_DEDUP=0: every trial parses, duplicates and level twins run
"""
import ctypes
import functools
import hashlib
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import _libs
import nearmiss as NM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = {"default": {}, "big": {"ATZ_PIPES": "3", "ATZ_MHINT": "1", "ATZ_PREFIX_MIN": "3072"},
        "mw4": {"ATZ_MW": "4", "ATZ_TARGET": "16384"}, "elig0": {"ATZ_ELIG": "0"},
        "noreplay": {"ATZ_REPLAY": "0", "ATZ_DEDUP": "0"}}

RUN = r"""
import hashlib, json, os, sys
sys.path.insert(0, %r)
import antiz_amd
d, settings = sys.argv[1], json.loads(sys.argv[2])
files = {f[:-4]: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".bin")}
for sname, kw in settings.items():
    with antiz_amd.Context(device=0, **kw) as c:
        for name, data in files.items():
            out, st = c.precompress(data)
            print(json.dumps({"file": name, "setting": sname, "sha": hashlib.sha256(out).hexdigest(), "n": len(out),
                              "tail": "recompressed:%%d/%%d" %% (st["n_recomp"], st["n_streams"]),
                              "restored": c.reconstruct(out) == data}), flush=True)
""" % ROOT

CTX_NAMES = ("recomp_tresh", "sizediff_tresh", "shortcut_len", "mismatch_tol", "brute_window")


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def atz():
    import antiz_amd
    from antiz_amd import build
    build.build()
    return antiz_amd


@functools.lru_cache(maxsize=None)
def _oracle(name, sname="default"):
    fx = NM.fixture()
    rc, a, st = _libs.ora_precompress(NM.files()[name][0], **NM.flags_kwargs(fx["settings"][sname]))
    assert rc == 0
    return a, st


@pytest.fixture(scope="module")
def corpus_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("nearmiss")
    for name, (data, _) in NM.files().items():
        (d / (name + ".bin")).write_bytes(data)
    return str(d)


def _expected(fx, name, sname):
    e = fx["files"][name]["runs"][sname]
    return e["atz_sha256"], e["atz_bytes"], e["tail"]


@pytest.mark.parametrize("env", list(ENVS))
def test_precompress_identical_to_reference(atz, corpus_dir, env):
    """Every file x setting under one schedule: the ATZ1 bytes are the reference's and reconstruct restores
    the input."""
    fx = NM.fixture()
    NM.check_pinned(fx)
    settings = {s: NM.flags_kwargs(f, CTX_NAMES) for s, f in fx["settings"].items()}
    r = subprocess.run([sys.executable, "-u", "-c", RUN, corpus_dir, json.dumps(settings)],
                       env=dict(os.environ, **ENVS[env]), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(got) == len(settings) * len(NM.NAMES) == 99
    bad = []
    for g in got:
        want = _expected(fx, g["file"], g["setting"])
        if (g["sha"], g["n"], g["tail"]) != want or not g["restored"]:
            bad.append((g["file"], g["setting"], g["tail"], want[2], g["n"], want[1], g["restored"]))
    assert not bad, "ATZ1 differs from the reference's under %s: %s" % (env, bad)


SWEEP_SETTINGS = ("default", "tol0", "tolT", "tolT-1", "floor_off", "strict_shortcut")
BRUTE_SETTINGS = ("brute", "brute_tol0")   # six times the trials: on the files of small streams only
BRUTE_FILES = ("storedpad_small", "eobpad", "strategy", "tolstop", "wrongwin")


@pytest.mark.parametrize("name", NM.NAMES)
def test_scan_and_sweep_match_oracle(atz, name):
    """atz_scan + atz_sweep (the exact rule for every stream) under the default options, the three
    tolerances, the floor's off branch, the strict shortcut and the brute-window phase with and without a
    tolerance: the stream table, each stream's chosen (clevel, window, memlevel), ident, recomp and the
    number of trials the reference's rule runs (its stops: main.cpp:700, 590), and for every recompressed
    stream first_diff, n_diff and the absolute diff positions and values decoded from diff_off / diff_val
    equal the oracle's."""
    fx = NM.fixture()
    data, streams = NM.files()[name]
    snames = SWEEP_SETTINGS + (BRUTE_SETTINGS if name in BRUTE_FILES else ())
    with ThreadPoolExecutor(8) as ex:     # the oracle runs outside the interpreter lock
        oracle = dict(zip(snames, ex.map(lambda s: _oracle(name, s)[1], snames)))
    bad = []
    for sname in snames:
        st = oracle[sname]
        with atz.Context(device=0, **NM.flags_kwargs(fx["settings"][sname], CTX_NAMES)) as c:
            recs = c.scan(data)
            assert [r[:4] for r in recs] == [(s["offset"], s["type"], s["comp_len"], s["infl_len"]) for s in st["streams"]]
            res, diffs = c.sweep()
        assert {g.offset for g in streams} <= {r[0] for r in recs}
        for r, s, (pos, val) in zip(res, st["streams"], _libs.diff_lists(res, diffs)):
            got = (r["clevel"], r["window"], r["memlevel"], r["ident"], r["recomp"], r["n_trials"], r["n_diff"], pos, val)
            want = (s["clevel"], s["window"], s["memlevel"], s["ident"], s["recomp"], s["n_trials"], s["n_diff"],
                    s["diff_pos"], s["diff_val"])
            if got != want or (s["n_diff"] and r["first_diff"] != s["first_diff"]):
                bad.append((sname, s["offset"], got[:7], r["first_diff"], want[:7], s["first_diff"]))
        assert len(diffs[0]) == sum(s["n_diff"] for s in st["streams"])
    assert not bad, bad[:5]


def test_inflate_batch_ignores_padding_bits(atz):
    """atz_inflate_batch on every stream of the corpus, at unaligned offsets and with bytes after it: set
    padding bits after a stored block's header and after the last end-of-block code change nothing."""
    cases = NM.mutated_streams()
    buf, ranges = bytearray(), []
    for s, _ in cases:
        buf += bytes((len(buf) * 7 + 3) % 5)
        ranges.append((len(buf), len(s) + 3))
        buf += s + b"\xff\xff\xff"
    with atz.Context(device=0) as c:
        got = c.inflate_batch(bytes(buf), ranges)
    bad = [(i, tuple(got[i]), (0, len(s), n)) for i, (s, n) in enumerate(cases)
           if not tuple(got[i]) == _libs.ora_inflate(s + b"\xff\xff\xff") == (0, len(s), n)]
    assert not bad, bad[:10]


def test_reconstruct_device_roundtrip_with_diffs(atz):
    """atz_reconstruct_device on ATZ1 files whose streams carry diff lists: up to 128 entries each
    (storedpad_big) and entries past the end of the re-deflated stream (tailflush)."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    with atz.Context(device=0) as c:
        for name in ("storedpad_big", "tailflush"):
            data = NM.files()[name][0]
            a, st = c.precompress(data)
            assert a == _oracle(name)[0] and st["n_recomp"] > 0
            d = ctypes.c_void_p()
            assert hip.hipMalloc(ctypes.byref(d), len(a) + 4096) == 0
            try:
                assert hip.hipMemcpy(d, a, len(a), 1) == 0                      # host to device
                p, n = c.reconstruct_device(d.value, a)
                assert n == len(data)
                out = ctypes.create_string_buffer(n)
                assert hip.hipMemcpy(out, p, n, 2) == 0                         # device to host
                assert out.raw == data
            finally:
                hip.hipFree(d)


def test_three_ranks_equal_one(atz, corpus_dir):
    """The shard path (tests/test_gpu_shard.py: three ranks sharing the GPU) on the midflush file with
    chunks of 20 000 bytes (two per rank; the reference loses most streams that cross a chunk boundary,
    main.cpp:413, so smaller chunks would leave none to recompress): rank 0's ATZ1, with the diff lists of
    streams on both sides of recomp_tresh, equals one rank's and the oracle's."""
    from test_gpu_shard import _run
    data = NM.files()["midflush"][0]
    rc, ref, _ = _libs.ora_precompress(data, chunksize=20000)
    assert rc == 0
    with atz.Context(chunksize=20000, device=0) as c:
        one, st = c.precompress(data)
    assert one == ref and 0 < st["n_recomp"] < st["n_streams"]
    res = _run(3, os.path.join(corpus_dir, "midflush.bin"), 20000)
    assert res[0][0] == one
    assert sum(v[1] for v in res.values()) == st["n_streams"] and sum(v[2] for v in res.values()) == st["n_recomp"]
