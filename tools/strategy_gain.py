#!/usr/bin/env python3
"""C3 (datagen's 100 MB PDF / PNG-like Z_FILTERED / JAR mix) precompressed without and with the strategy
trials: recorded streams, the share of the PNG-like ones among them, MB/s (best of 3 host
calls after a warm-up, upload included).  usage: python tools/strategy_gain.py [cache_dir]   -> one JSON line"""
import json
import os
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import antiz_amd
from antiz_amd import datagen

data = open(datagen.cached("c3", sys.argv[1] if len(sys.argv) > 1 else "/tmp/atz_bench_cache"), "rb").read()
png, at = set(), data.find(b"IDAT")
while at >= 0:   # (every PNG-like piece: length, "IDAT", the stream)
    png.add(at + 4)
    at = data.find(b"IDAT", at + 4)
out = {"file_bytes": len(data), "png_streams": len(png)}
with antiz_amd.Context(device=0, strategies=()) as c:   # the first context of a process runs slower than later ones
    c.precompress(data)
for tag, names in (("off", ()), ("on", ("filtered", "rle", "huffman"))):
    with antiz_amd.Context(device=0, strategies=names) as c:
        c.precompress(data)   # (buffers sized, kernels loaded)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            atz, st = c.precompress(data)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        back = c.reconstruct(atz) == data
        if not names:   # how many of the pieces the scan records as streams at all (the sweep sees only those)
            out["png_scanned"] = sum(1 for r in c.scan(data) if r[0] in png)
            antiz_amd.lib().atz_free(c._cands[0])
    n, pos, rec = struct.unpack_from("<Q", atz, 20)[0], 28, 0
    for _ in range(n):
        off, _, il = struct.unpack_from("<QQQ", atz, pos)
        nd = struct.unpack_from("<Q", atz, pos + 27)[0]
        rec += off in png
        pos += 35 + (8 + 9 * nd if nd else 0) + il
    out[tag] = {"magic": atz[3], "n_streams": st["n_streams"], "n_recomp": st["n_recomp"], "png_recorded": rec,
                "atz_bytes": len(atz), "n_trials": st["n_trials"], "MB_per_s": round(len(data) / 1e6 / best, 1),
                "sweep_ms": round(st["sweep_ms"], 1), "roundtrip_ok": back}
print(json.dumps(out))
