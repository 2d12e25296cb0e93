"""Writes tests/golden/nearmiss.json: the REAL reference's results (oracle/_ref/uncomp --notest, built by
oracle/build_ref.sh) on the near-miss corpus (tests/nearmiss.py) under the settings of nearmiss.settings():
for each file and setting the input SHA-256, the ATZ1 SHA-256 and length and the `recompressed:K/N`
line; for the default setting also the stream table parsed from the reference's ATZ1 (offset, comp_len,
c, w, m, n_diff, first_diff of every recompressed stream).  Recorded output only.

T (the tolerance settings) is the diff count of most of the tailflush file's SYNC streams, read from the
reference's default ATZ1, and D (the size-difference settings) the number of bytes by which most of them
are longer than their chosen trial's output.

The maker fails unless the corpus shows what it is for (checked with the CPU oracle, whose default run
must equal the reference's), and unless the tolerance stop and the brute-window phase change the
reference's bytes: see check_corpus() and check_stops().
Build container only.  Run: python3 tools/make_nearmiss_golden.py   (under a minute)."""
import collections
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _libs  # noqa: E402
import nearmiss as N  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "nearmiss.json")


def sha(b):
    return hashlib.sha256(b).hexdigest()


def run_ref(path, flags):
    out = path + "." + hashlib.md5(" ".join(flags).encode()).hexdigest()[:10] + ".atz"
    r = subprocess.run([_libs.REF_UNCOMP, "-i", path, "-o", out, "--notest"] + flags, capture_output=True, text=True)
    assert r.returncode == 0, (path, flags, r.returncode, r.stderr[-500:])
    with open(out, "rb") as f:
        a = f.read()
    os.remove(out)
    tail = [ln for ln in r.stdout.splitlines() if ln.startswith("recompressed:")]
    assert len(tail) == 1, r.stdout[-500:]
    return a, tail[0]


def check_corpus(files):
    """The properties the corpus exists for, on the oracle's default run."""
    full = far = tail = 0
    mid_lo = mid_hi = 0
    pad_ks = collections.Counter()
    for name, (data, streams) in files.items():
        rc, _, st = _libs.ora_precompress(data)
        assert rc == 0, name
        by = {s["offset"]: s for s in st["streams"]}
        for g in streams:
            o = by[g.offset]
            assert o["comp_len"] == g.length, (name, g)
            miss = g.length - o["ident"]
            whole = o["n_trials"] >= 81
            full += whole and o["recomp"]
            far += o["recomp"] and o["first_diff"] > 4096
            if o["recomp"] and o["n_diff"]:
                infl = zlib.decompress(data[g.offset:g.offset + g.length])
                L = len(_libs.ora_deflate(infl, o["clevel"], o["window"], o["memlevel"])[0])
                tail += o["diff_pos"][-1] >= L
            if g.family == "storedpad":
                k = len(g.pads)
                assert miss == k, (g, miss)
                assert bool(o["recomp"]) == (k <= 128), g
                if o["recomp"]:
                    assert o["n_diff"] == k and o["diff_pos"] == list(g.pads), g
                    pad_ks[k] += 1
            if g.family == "midflush":
                mid_lo += 113 <= miss <= 128
                mid_hi += 129 <= miss <= 144
    assert all(pad_ks[k] >= 1 for k in N.PAD_KS if k <= 128), pad_ks
    assert mid_lo >= 5 and mid_hi >= 5, (mid_lo, mid_hi)
    assert full >= 20 and far >= 10 and tail >= 10, (full, far, tail)
    return dict(whole_list_recompressed=int(full), first_diff_past_4096=int(far), tail_diffs=int(tail),
                midflush_113_128=mid_lo, midflush_129_144=mid_hi)


def check_stops(files, settings, runs):
    """Stopping must matter: the tolerance stop (main.cpp:700) and the brute-window entry (main.cpp:590)
    change the chosen trial of several streams, in the oracle's tables and in the reference's bytes."""
    def table(name, s):
        rc, _, st = _libs.ora_precompress(files[name][0], **N.flags_kwargs(settings[s]))
        assert rc == 0
        return [(x["clevel"], x["window"], x["memlevel"], x["recomp"], x["n_diff"]) for x in st["streams"]]

    for a, b, name in (("tolT", "tolT-1", "tolstop"), ("default", "tol0", "tolstop"), ("brute", "brute_tol0", "tolstop"),
                       ("default", "tolT", "tolstop"), ("default", "brute", "wrongwin")):
        n = sum(x != y for x, y in zip(table(name, a), table(name, b)))
        assert n >= 3, (a, b, name, n)
        assert runs[(name, a)][0] != runs[(name, b)][0], (a, b, name)


def sync_T_D(data, streams, table):
    """T and D of the tailflush file from the reference's default stream table."""
    by = {e["offset"]: e for e in table}
    nd, sd = collections.Counter(), collections.Counter()
    for g in streams:
        if g.tag != "sync":
            continue
        e = by[g.offset]
        infl = zlib.decompress(data[g.offset:g.offset + g.length])
        nd[e["n_diff"]] += 1
        sd[g.length - len(_libs.ora_deflate(infl, e["c"], e["w"], e["m"])[0])] += 1
    (T, nt), (D, nD) = nd.most_common(1)[0], sd.most_common(1)[0]
    assert nt >= 3 and nD >= 3 and T >= 2 and D >= 1, (nd, sd)
    return T, D


def main():
    files = N.files()
    props = check_corpus(files)
    print(props, flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        paths = {}
        for name, (data, _) in files.items():
            paths[name] = os.path.join(tmp, name + ".bin")
            with open(paths[name], "wb") as f:
                f.write(data)
        default = {name: run_ref(paths[name], []) for name in files}
        T, D = sync_T_D(*files["tailflush"], N.parse_atz1(default["tailflush"][0]))
        settings = N.settings(T, D)
        jobs = [(name, s) for name in files for s in settings if s != "default"]
        with ThreadPoolExecutor(6) as ex:
            runs = dict(zip(jobs, ex.map(lambda j: run_ref(paths[j[0]], settings[j[1]]), jobs)))
    for name in files:
        runs[(name, "default")] = default[name]
    check_stops(files, settings, runs)
    res = {"seed": N.SEED, "T": T, "D": D, "settings": settings, "corpus": props, "files": {}}
    for name, (data, streams) in files.items():
        rc, atz, _ = _libs.ora_precompress(data)
        assert rc == 0 and atz == default[name][0], "the oracle's default ATZ1 differs from the reference's: " + name
        table = [[e[k] for k in ("offset", "comp_len", "c", "w", "m", "n_diff", "first_diff")]
                 for e in N.parse_atz1(default[name][0])]
        res["files"][name] = {
            "input_sha256": sha(data), "input_bytes": len(data), "n_generated": len(streams), "table": table,
            "runs": {s: {"atz_sha256": sha(runs[(name, s)][0]), "atz_bytes": len(runs[(name, s)][0]),
                         "tail": runs[(name, s)][1]} for s in settings}}
        print(name, len(data), {s: res["files"][name]["runs"][s]["tail"] for s in settings}, flush=True)
    with open(OUT, "w") as f:
        text = json.dumps(res, indent=1)
        f.write(text.replace("[\n     ", "[").replace(",\n     ", ", ").replace("\n    ]", "]") + "\n")   # one table row per line
    N.check_pinned(N.fixture())
    print("wrote", OUT, os.path.getsize(OUT), "bytes; T = %d, D = %d" % (T, D))


if __name__ == "__main__":
    main()
