#!/usr/bin/env python3
"""Generate tests/golden/blockedges.json from the inputs of tests/blockedges.py.

Needs the reference build (oracle/build_ref.sh -> oracle/_ref/libzref.so, uncomp).  The fixture holds recorded
results and numbers only; the inputs are regenerated from seeds:
  "tuned"    per target of blockedges.target_list(), by position: the [text length, tail length, variant] that
             blockedges.tune() found, or null for a target that is left out -- one that TUNE_STEPS streams did not
             reach, or one whose stream the reference's rule leaves at a near miss (a trial within --mismatch-tol
             ends its search before the exact one), so that it would not be reproduced exactly
  "deflate"  per item of blockedges.items(), by position: [length, first 16 hex digits of the SHA-256] of the real
             zlib 1.2.8's stream (_libs.zref_deflate)
  "files"    per family: the SHA-256 and length of blockedges.files() built from the real zlib's streams, its stream
             count, what oracle/_ref/uncomp --notest writes for it under each setting of blockedges.settings_of()
             (ATZ1 SHA-256, length and the `recompressed:K/N` line), and the stream table of its default ATZ1
             ([offset, comp_len, c, w, m, n_diff, first_diff] per recompressed stream)
The recorder fails unless every generated stream is in the reference's default table, whole (no diff), and the
oracle's default ATZ1 is the reference's.  A rerun writes the same bytes.  Run: python3 tests/golden/make_blockedges.py
(about a minute)."""
import hashlib
import json
import multiprocessing
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _libs  # noqa: E402
import blockedges as B  # noqa: E402
import nearmiss  # noqa: E402


def sha(b):
    return hashlib.sha256(b).hexdigest()


def ref_run(data, flags):
    """-> (ATZ1 bytes, `recompressed:K/N`) of the reference."""
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.atz")
        with open(src, "wb") as f:
            f.write(data)
        r = subprocess.run([_libs.REF_UNCOMP, "-i", src, "-o", dst, "--notest"] + flags, capture_output=True, text=True)
        assert r.returncode == 0, (flags, r.returncode, r.stderr[-500:])
        tail = [ln for ln in r.stdout.splitlines() if ln.startswith("recompressed:")]
        assert len(tail) == 1, r.stdout[-500:]
        with open(dst, "rb") as f:
            return f.read(), tail[0]


def _tune(k):
    return B.tune(k, B.target_list()[k])


def tune_all():
    """The triples, with the targets taken out whose stream the oracle's default rule does not reproduce whole."""
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        triples = pool.map(_tune, range(len(B.target_list())), chunksize=4)
    unreached = sum(t is None for t in triples)
    for _ in range(3):
        B.set_tuned(triples)
        its, drop = B.items(), set()
        for fam in ("B2", "B3"):
            data, recs = B.files()[fam]
            rc, _, st = _libs.ora_precompress(data)
            assert rc == 0
            by = {s["offset"]: s for s in st["streams"]}
            drop |= {k for off, n, k, _ in recs if not (off in by and by[off]["recomp"] and by[off]["ident"] == n)}
        if not drop:
            break
        assert all(its[k].tag == "tuned" for k in drop), [B.E.label(its[k]) for k in drop]
        live = [j for j, t in enumerate(triples) if t is not None]     # the tuned items, in the order of items()
        tuned_pos = [k for k, it in enumerate(its) if it.tag == "tuned"]
        for k in drop:
            triples[live[tuned_pos.index(k)]] = None
    else:
        raise AssertionError("near misses keep appearing")
    return triples, unreached


def record():
    """The fixture as a dict, from the real zlib and the real reference."""
    triples, unreached = tune_all()
    B.set_tuned(triples)
    deflate = []
    for it in B.items():
        s = _libs.zref_deflate(it.data, it.level, it.window, it.memlevel)
        deflate.append([len(s), B.E.sha16(s)])
    files = B.files(_libs.zref_deflate)
    jobs = [(fam, s) for fam in B.FAMILIES for s in B.settings_of(fam)]
    with ThreadPoolExecutor(6) as ex:
        runs = dict(zip(jobs, ex.map(lambda j: ref_run(files[j[0]][0], B.SETTINGS[j[1]]), jobs)))
    out = {}
    for fam in B.FAMILIES:
        data, recs = files[fam]
        atz = runs[(fam, "default")][0]
        table = nearmiss.parse_atz1(atz)
        by = {e["offset"]: e for e in table}
        lost = [(off, n) for off, n, _, _ in recs if not (off in by and by[off]["comp_len"] == n and by[off]["n_diff"] == 0)]
        assert not lost, "%s: the reference does not reproduce %d streams: %s" % (fam, len(lost), lost[:5])
        rc, ora, _ = _libs.ora_precompress(data)
        assert rc == 0 and ora == atz, "the oracle's default ATZ1 differs from the reference's: " + fam
        out[fam] = {"input_sha256": sha(data), "input_bytes": len(data), "n_streams": len(recs),
                    "runs": {s: {"atz_sha256": sha(runs[(fam, s)][0]), "atz_bytes": len(runs[(fam, s)][0]),
                                 "tail": runs[(fam, s)][1]} for s in B.settings_of(fam)},
                    "table": [[e[k] for k in ("offset", "comp_len", "c", "w", "m", "n_diff", "first_diff")] for e in table]}
    return {"source": "zlib 1.2.8 as vendored by the reference (oracle/_ref/libzref.so) and oracle/_ref/uncomp; "
                      "inputs from tests/blockedges.py; generated by tests/golden/make_blockedges.py",
            "seed": B.SEED, "settings": B.SETTINGS, "unreached": unreached,
            "tuned": [None if t is None else list(t) for t in triples], "deflate": deflate, "files": out}


def dumps(fx):
    """One recorded result a line."""
    def rows(v):
        return "[\n" + ",\n".join(json.dumps(x, separators=(",", ":")) for x in v) + "\n]"
    parts = ["%s: %s" % (json.dumps(k), json.dumps(fx[k])) for k in ("source", "seed", "settings", "unreached")]
    parts += ["%s: %s" % (json.dumps(k), rows(fx[k])) for k in ("tuned", "deflate")]
    fams = []
    for fam, e in fx["files"].items():
        head = ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in e.items() if k != "table")
        fams.append("%s: {\n%s,\n  \"table\": %s}" % (json.dumps(fam), head, rows(e["table"])))
    parts.append("\"files\": {\n%s\n}" % ",\n".join(fams))
    return "{\n" + ",\n".join(parts) + "\n}\n"


def main():
    if not (_libs.have_zref() and os.path.exists(_libs.REF_UNCOMP)):
        sys.exit("oracle/_ref missing: run oracle/build_ref.sh first")
    text = dumps(record())
    assert json.loads(text) and len(text) < 400 * 1024, len(text)
    with open(B.FIXTURE, "w") as f:
        f.write(text)
    print("%s: %d bytes" % (B.FIXTURE, len(text)))


if __name__ == "__main__":
    main()
