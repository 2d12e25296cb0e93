#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ from the REAL reference (oracle/_ref, built by
oracle/build_ref.sh from /root/reference).  Run in the build container only; the outputs are data
(inputs + expected outputs) and are committed, so the GPU box never needs /root/reference.

  G1 zt/            the reference's own binary vectors (`includes, tools, stuff/zlib test/bin/Release/*.bin`)
                    + kat.json: expected .atz SHA-256 and stream table of input.bin ++ the 5 streams
  G2 deflate_kat.json  zlib-1.2.8 deflate length+SHA-256 for c0-9 x w9-15 x m1-9 on 4 inputs,
                    full bytes for the text input at w15 (deflate_kat_*.bin)
  G3/G4/G5 cases.json  end-to-end cases (inputs given by generator+seed or committed file, option set,
                    expected input SHA-256, expected .atz SHA-256, stream table) exercising the sweep
                    stop rule, brute-window, threshold wrap, chunk-boundary loss, <=16-byte skip,
                    EOF-multiple-of-chunk, and small C1-C4 configs.
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from antiz_amd import datagen  # noqa: E402
import _libs  # noqa: E402
import atzfile  # noqa: E402

ZT = "/root/reference/includes, tools, stuff/zlib test/bin/Release"
ZT_FILES = ["input.bin", "zlibtest_out_c1.bin", "zlibtest_out_2k.bin", "zlibtest_out_c5.bin",
            "zlibtest_out_c6.bin", "zlibtest_out_c9.bin"]


def sha(b):
    return hashlib.sha256(b).hexdigest()


def parse_atz(atz):
    """stream descriptors of an ATZ1 file (main.cpp:1031-1063)"""
    return [dict(offset=d["off"], comp_len=d["cl"], infl_len=d["il"], clevel=d["c"], window=d["w"], memlevel=d["m"],
                 n_diff=d["nd"]) for d in atzfile.parse(atz)[2]]


def run_ref(data, opts):
    d = tempfile.mkdtemp()
    try:
        p = os.path.join(d, "in.bin")
        with open(p, "wb") as f:
            f.write(data)
        args = [_libs.REF_UNCOMP, "-i", p, "-o", p + ".atz"]
        for k, v in opts.items():
            if k == "brute_window":
                if v:
                    args.append("--brute-window")
            else:
                args += ["--" + k.replace("_", "-"), str(v)]
        r = subprocess.run(args, capture_output=True, text=True, timeout=3600)
        atz = open(p + ".atz", "rb").read() if os.path.exists(p + ".atz") else b""
        return r.returncode, r.stdout, atz
    finally:
        shutil.rmtree(d)


def g1():
    os.makedirs(os.path.join(HERE, "zt"), exist_ok=True)
    blobs = []
    for f in ZT_FILES:
        b = open(os.path.join(ZT, f), "rb").read()
        shutil.copyfile(os.path.join(ZT, f), os.path.join(HERE, "zt", f))
        blobs.append(b)
    kat = b"".join(blobs)
    rc, out, atz = run_ref(kat, {})
    assert rc == 0 and "bit by bit identical" in out, out
    json.dump(dict(files=ZT_FILES, input_sha256=sha(kat), atz_sha256=sha(atz), atz_len=len(atz),
                   streams=parse_atz(atz), stdout=out), open(os.path.join(HERE, "zt", "kat.json"), "w"), indent=1)


def g2():
    import numpy as np
    rng = np.random.default_rng(2024)
    inputs = {
        "asd": b"asd" * 4608,
        "text4k": datagen.text(rng, 4096),
        "rand5k": rng.integers(0, 256, size=5000, dtype=np.uint8).tobytes(),
        "input8k": open(os.path.join(ZT, "input.bin"), "rb").read()[:8192],
    }
    kat = {"inputs": {k: sha(v) for k, v in inputs.items()}, "results": {}}
    os.makedirs(os.path.join(HERE, "kat"), exist_ok=True)
    for k, v in inputs.items():
        with open(os.path.join(HERE, "kat", k + ".bin"), "wb") as f:
            f.write(v)
    full = {}
    for name, d in inputs.items():
        for c in range(10):
            for w in range(9, 16):
                for m in range(1, 10):
                    s = _libs.zref_deflate(d, c, w, m)
                    kat["results"]["%s/%d/%d/%d" % (name, c, w, m)] = [len(s), sha(s)]
                    if name == "text4k" and w == 15:
                        full["%d/%d" % (c, m)] = s.hex()
    json.dump(kat, open(os.path.join(HERE, "deflate_kat.json"), "w"))
    json.dump(full, open(os.path.join(HERE, "deflate_kat_text4k_w15.json"), "w"))


def find_w10_tolerance_case():
    """A w10 c2 m8 stream where c3 lands within 2 diffs (SURVEY.md s0 'first in sweep order wins')."""
    import numpy as np
    for seed in range(5000):
        rng = np.random.default_rng(10_000 + seed)
        d = datagen.text(rng, int(rng.integers(800, 4000)))
        s2 = datagen.zstream(d, 2, 10, 8)
        s3 = datagen.zstream(d, 3, 10, 8)
        if len(s2) == len(s3) and s2 != s3 and sum(a != b for a, b in zip(s2, s3)) <= 2:
            return s2, seed
    raise RuntimeError("no tolerance case found")


def g345():
    import numpy as np
    cases = []

    def add(name, data, opts, gen=None, commit_input=True):
        rc, out, atz = run_ref(data, opts)
        case = dict(name=name, opts=opts, input_sha256=sha(data), input_len=len(data), ref_rc=rc,
                    atz_sha256=sha(atz) if rc == 0 else None, atz_len=len(atz),
                    streams=parse_atz(atz) if rc == 0 and atz else None, stdout=out)
        if gen:
            case["gen"] = gen
        if commit_input:
            fn = "case_%s.bin" % name
            with open(os.path.join(HERE, "cases", fn), "wb") as f:
                f.write(data)
            case["file"] = fn
        cases.append(case)
        print(name, rc, len(data), "->", len(atz), flush=True)

    os.makedirs(os.path.join(HERE, "cases"), exist_ok=True)
    # G3 sweep semantics
    s, seed = find_w10_tolerance_case()
    body = b"HDR" + s + b"TAIL"
    add("w10_tol_default", body, {})
    add("w10_tol_zero", body, {"mismatch_tol": 0})
    rng = np.random.default_rng(31)
    pieces = []
    for w in (10, 11, 12, 13, 14):
        d = datagen.text(rng, 6000)
        pieces.append(datagen.zstream(d, 6, w, 8))
    # brute-window: re-label the CINFO of a w12 stream as w14 so the header class is wrong
    d = datagen.text(rng, 5000)
    s12 = bytearray(datagen.zstream(d, 9, 12, 8))
    hdr = (0x68 << 8) | 0xC0
    hdr += 31 - (hdr % 31)
    s12[0], s12[1] = hdr >> 8, hdr & 0xff
    pieces.append(bytes(s12))
    brute = b"".join(pieces)
    add("brute_off", brute, {})
    add("brute_on", brute, {"brute_window": 1})
    add("brute_on_tol0", brute, {"brute_window": 1, "mismatch_tol": 0})
    c4s = datagen.gen_c4(seed=41, n_streams=12, workers=1)
    add("recomp_wrap", c4s, {"recomp_tresh": 1000})
    add("tiny_shortcut", c4s, {"shortcut_len": 64, "recomp_tresh": 16, "sizediff_tresh": 8})
    png = datagen._png_like(np.random.default_rng(5), 20000)
    add("filtered_exhaust", b"IDAT" + png + b"IEND", {})
    # G4 scan semantics
    c2 = datagen.gen_c2(seed=7, n=40)
    add("chunk_default", c2, {})
    add("chunk_4096", c2, {"chunksize": 4096})
    add("chunk_777", c2, {"chunksize": 777})
    add("chunk_big", c2, {"chunksize": 1 << 24})
    tiny = datagen.zstream(b"a", 6) + b"xx" + datagen.zstream(b"hello hello hello", 9) + b"zz" + \
        datagen.zstream(datagen.text(np.random.default_rng(3), 3000), 6)
    add("tiny_streams", tiny, {})
    rng = np.random.default_rng(99)
    noise = bytearray(rng.integers(0, 256, size=60000, dtype=np.uint8).tobytes())
    for k in range(0, 60000, 997):                       # plant false headers
        h = [0x7801, 0x785e, 0x789c, 0x78da, 0x2815, 0x68de][k % 6]
        noise[k], noise[k + 1] = h >> 8, h & 0xff
    add("false_headers", bytes(noise) + c2[:20000] + bytes(noise[:5000]), {"chunksize": 16384})
    cs = 4096
    base = datagen.gen_c2(seed=8, n=8)
    size = cs + 5 * (cs - 1)
    eofm = (base * 4)[:size]
    add("eof_multiple", eofm, {"chunksize": cs})
    add("eof_multiple_minus1", eofm[:-1], {"chunksize": cs})
    # G5 small configs
    add("c1", datagen.gen_c1(), {}, gen=dict(config="c1"), commit_input=False)
    add("c2_n300", datagen.gen_c2(n=300), {}, gen=dict(config="c2", n=300), commit_input=False)
    add("c3_1mb", datagen.gen_c3(total=1_000_000, workers=4), {}, gen=dict(config="c3", total=1_000_000),
        commit_input=False)
    add("c4_n200", datagen.gen_c4(n_streams=200, workers=4), {}, gen=dict(config="c4", n_streams=200),
        commit_input=False)
    add("c5_n120", datagen.gen_c5(n_streams=120, workers=4), {"brute_window": 1},
        gen=dict(config="c5", n_streams=120), commit_input=False)
    json.dump(cases, open(os.path.join(HERE, "cases.json"), "w"), indent=1)


if __name__ == "__main__":
    assert os.path.exists(_libs.REF_UNCOMP), "run oracle/build_ref.sh first"
    what = sys.argv[1:] or ["g1", "g2", "g345"]
    for w in what:
        globals()[w]()
