"""zlib 1.2.8 deflate with a strategy, from the reference's own zlib (oracle/_ref/libz128.so, built by
build()): the expected bytes of the strategy tests, and a Python model of the strategy extension's
candidate list and rule on top of it.

Python's zlib is whatever the system ships; whether it matches 1.2.8 bit for bit under Z_FILTERED, Z_RLE
and Z_HUFFMAN_ONLY is recorded by tests/test_strategy_cpu.py, not assumed.
"""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z128_SO = os.path.join(ROOT, "oracle", "_ref", "libz128.so")

Z_DEFAULT, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE = 0, 1, 2, 3
Z_FINISH, Z_STREAM_END, Z_DEFLATED = 4, 1, 8
NAMES = {Z_FILTERED: "filtered", Z_HUFFMAN_ONLY: "huffman", Z_RLE: "rle"}


class ZStream(C.Structure):   # z_stream (zlib.h), LP64
    _fields_ = [("next_in", C.c_void_p), ("avail_in", C.c_uint), ("total_in", C.c_ulong),
                ("next_out", C.c_void_p), ("avail_out", C.c_uint), ("total_out", C.c_ulong),
                ("msg", C.c_char_p), ("state", C.c_void_p), ("zalloc", C.c_void_p), ("zfree", C.c_void_p),
                ("opaque", C.c_void_p), ("data_type", C.c_int), ("adler", C.c_ulong), ("reserved", C.c_ulong)]


_z = None


def z128():
    """The reference's zlib 1.2.8; raises (the tests fail, they do not skip) when it was not built."""
    global _z
    if _z is None:
        # RTLD_DEEPBIND: the library's own deflateReset / deflateEnd, not those of a system zlib that the
        # interpreter has already loaded (the state structures differ between versions)
        L = C.CDLL(Z128_SO, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        L.zlibVersion.restype = C.c_char_p
        assert L.zlibVersion() == b"1.2.8", L.zlibVersion()
        L.deflateInit2_.argtypes = [C.POINTER(ZStream), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p,
                                    C.c_int]
        L.deflate.argtypes = [C.POINTER(ZStream), C.c_int]
        L.deflateEnd.argtypes = [C.POINTER(ZStream)]
        L.deflateBound.argtypes = [C.POINTER(ZStream), C.c_ulong]
        L.deflateBound.restype = C.c_ulong
        _z = L
    return _z


def deflate(data, level, window, memlevel, strategy=Z_DEFAULT):
    """One deflateInit2 / deflate(Z_FINISH) / deflateEnd, as the reference's doDeflate (main.cpp:976-1003)."""
    L = z128()
    zs = ZStream()
    r = L.deflateInit2_(C.byref(zs), level, Z_DEFLATED, window, memlevel, strategy, b"1.2.8", C.sizeof(ZStream))
    assert r == 0, r
    cap = L.deflateBound(C.byref(zs), len(data)) + 64
    src = C.create_string_buffer(bytes(data), max(len(data), 1))
    out = C.create_string_buffer(cap)
    zs.next_in = C.cast(src, C.c_void_p)
    zs.avail_in = len(data)
    zs.next_out = C.cast(out, C.c_void_p)
    zs.avail_out = cap
    r = L.deflate(C.byref(zs), Z_FINISH)
    n = zs.total_out
    L.deflateEnd(C.byref(zs))
    assert r == Z_STREAM_END, r
    return out.raw[:n]


# ---- the extension's candidate list and rule ---------------------------------------------------
MEMLEVELS = (8, 9, 7, 6, 5, 4, 3, 2, 1)


def candidates(header, mask):
    """(strategy, level, window, memlevel) in the extension's order for a stream with this 2-byte header:
    bounded by FLEVEL, which zlib writes from level and strategy (Z/deflate.c:738-750)."""
    window = (header[0] >> 4) + 8
    flevel = header[1] >> 6
    groups = {0: [(Z_RLE, (6,)), (Z_HUFFMAN_ONLY, (6,))], 1: [(Z_FILTERED, (5, 4))], 2: [(Z_FILTERED, (6,))],
              3: [(Z_FILTERED, (9, 8, 7))]}[flevel]
    out = []
    for strat, levels in groups:
        if not (mask >> strat) & 1:
            continue
        for m in MEMLEVELS:
            for lv in levels:
                out.append((strat, lv, window, m))
    return out


def rule(stream, inflated, mask, recomp_tresh=128, sizediff_tresh=128, mismatch_tol=2, shortcut_len=512):
    """testDeflateParams and the stop rule (main.cpp:616-700) restarted with identBytes = 0 over candidates();
    -> None if the stream is not recorded (main.cpp:454), else dict(strategy, level, window, memlevel, ident,
    diff_pos, diff_val)."""
    C_ = len(stream)
    best, ident = None, 0
    for cand in candidates(stream[:2], mask):
        strat, lv, w, m = cand
        out = deflate(inflated, lv, w, m, strat)
        if C_ > shortcut_len:   # main.cpp:632-653 (the threshold is an unsigned difference)
            head = out[:shortcut_len]
            if sum(1 for x, y in zip(head, stream) if x == y) < (shortcut_len - recomp_tresh) % (1 << 64):
                continue
        if abs(len(out) - C_) > sizediff_tresh:
            continue
        k = min(len(out), C_)
        same = sum(1 for a, b in zip(out[:k], stream[:k]) if a == b)
        if same > ident:
            ident, best = same, (cand, out)
            if same == C_ or same + mismatch_tol >= C_:
                break
    if best is None or not (C_ - ident <= recomp_tresh and ident > 0):
        return None
    (strat, lv, w, m), out = best
    # main.cpp:699-714: positions below min(len) that differ, then every position the shorter output lacks
    pos = [i for i in range(C_) if i >= len(out) or out[i] != stream[i]]
    return dict(strategy=strat, level=lv, window=w, memlevel=m, ident=ident, diff_pos=pos,
                diff_val=bytes(stream[i] for i in pos))
