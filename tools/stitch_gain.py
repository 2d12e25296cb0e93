#!/usr/bin/env python3
"""C3 with its PNG-like streams cut into 8 KiB IDAT chunks (datagen.gen_c3_chunked) precompressed under
ATZ_STRATEGIES=filtered,rle,huffman without and with the stitch extension: records, the PNG-like
streams among them (stitched or in one chunk; exact = no diff byte), ATZ bytes, MB/s and sweep_ms of 3 interleaved
host calls each after a warm-up (upload included), and from one ATZ_TIMING=1 child run the times of the anchor
pass, the stitch gather and the stitched inflate.
usage: python tools/stitch_gain.py [cache_dir]   -> one JSON line"""
import json
import os
import re
import struct
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import antiz_amd
from antiz_amd import datagen

STRATS = ("filtered", "rle", "huffman")
cache = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "/tmp/atz_bench_cache"
data = open(datagen.cached("c3_chunked", cache), "rb").read()

if "--timing-child" in sys.argv:   # (run with ATZ_TIMING=1: the library prints its phase times on stderr)
    with antiz_amd.Context(device=0, strategies=STRATS, stitch=("png",)) as c:
        c.precompress(data)
        sys.stderr.write("atz: measured call\n")
        c.precompress(data)
    sys.exit(0)


def summary(atz):
    """-> (descriptors, stitched, stitched exact, one-chunk PNG-like, one-chunk exact)"""
    n, pos = struct.unpack_from("<Q", atz, 20)[0], 28
    st = st_exact = one = one_exact = 0
    for _ in range(n):
        off, _, il = struct.unpack_from("<QQQ", atz, pos)
        c = atz[pos + 24]
        nd = struct.unpack_from("<Q", atz, pos + 27)[0]
        pos += 35 + (8 + 9 * nd if nd else 0) + il
        if atz[3] == 4 and c & 0x80:
            pos += 4 + 4 * struct.unpack_from("<I", atz, pos)[0]
            st += 1
            st_exact += nd == 0
        elif data[off - 4:off] == b"IDAT":
            one += 1
            one_exact += nd == 0
    return n, st, st_exact, one, one_exact


out = {"file_bytes": len(data), "idat_chunks": data.count(b"IDAT"),
       "png_streams": open(datagen.cached("c3", cache), "rb").read().count(b"IDAT")}
ctxs = {tag: antiz_amd.Context(device=0, strategies=STRATS, stitch=names) for tag, names in (("off", ()), ("on", ("png",)))}
runs = {tag: [] for tag in ctxs}
last = {}
for tag, c in ctxs.items():   # (buffers sized, kernels loaded; the first context of a process runs slower)
    c.precompress(data)
    c.precompress(data)
for _ in range(3):
    for tag, c in ctxs.items():
        t0 = time.perf_counter()
        atz, st = c.precompress(data)
        runs[tag].append((time.perf_counter() - t0, st["sweep_ms"], st["scan_ms"]))
        last[tag] = (atz, st)
for tag, c in ctxs.items():
    atz, st = last[tag]
    n, stitched, st_exact, one, one_exact = summary(atz)
    out[tag] = {"magic": atz[3], "n_streams": st["n_streams"], "n_recomp": st["n_recomp"], "png_stitched": stitched,
                "png_stitched_exact": st_exact, "png_one_chunk": one, "png_one_chunk_exact": one_exact,
                "atz_bytes": len(atz), "n_trials": st["n_trials"],
                "MB_per_s": [round(len(data) / 1e6 / dt, 1) for dt, _, _ in runs[tag]],
                "sweep_ms": [round(x, 1) for _, x, _ in runs[tag]], "scan_ms": [round(x, 1) for _, _, x in runs[tag]],
                "dev_bytes_peak": st["dev_bytes_peak"], "roundtrip_ok": c.reconstruct(atz) == data}
    c.close()
r = subprocess.run([sys.executable, os.path.abspath(__file__), cache, "--timing-child"], env=dict(os.environ, ATZ_TIMING="1"),
                   capture_output=True, text=True)
log = r.stderr.split("atz: measured call\n")[-1]
m = re.search(r"k_anchors_ordered: (\d+) anchors, kernels ([\d.]+) ms", log)
g = re.search(r"stitch: (\d+) candidates, (\d+) bytes in (\d+) segments, k_gather ([\d.]+) ms, k_inflate ([\d.]+) ms", log)
if r.returncode == 0 and m and g:
    out["timing"] = {"anchors": int(m.group(1)), "anchor_pass_ms": float(m.group(2)),
                     "anchor_pass_ms_per_GB": round(float(m.group(2)) / (len(data) / 1e9), 3),
                     "candidates": int(g.group(1)), "stitch_bytes": int(g.group(2)), "segments": int(g.group(3)),
                     "gather_ms": float(g.group(4)), "stitched_inflate_ms": float(g.group(5))}
print(json.dumps(out))
