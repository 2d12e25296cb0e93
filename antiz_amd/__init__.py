"""antiz_amd -- MI355X-native zlib-stream precompressor (drop-in for AntiZ's precompress/reconstruct path).

The product is the C ABI library antiz_amd/_build/libatz_accel.so (HIP kernels for gfx950, see
include/atz_accel.h) and the `uncomp` CLI built beside it.  This module is the thin Python host
mirror used by tests and bench.py: it loads that library and raises if it is missing -- there is
no CPU fallback.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ATZ_LIB") or os.path.join(HERE, "_build", "libatz_accel.so")   # ATZ_LIB: diagnostic builds
CLI_PATH = os.path.join(HERE, "_build", "uncomp")

u64 = C.c_uint64
u8p = C.POINTER(C.c_uint8)


class Opts(C.Structure):
    _fields_ = [("recomp_tresh", u64), ("sizediff_tresh", u64), ("shortcut_len", u64), ("mismatch_tol", u64),
                ("chunksize", u64), ("brute_window", C.c_int32), ("device", C.c_int32)]


class Cand(C.Structure):
    _fields_ = [("offset", u64), ("comp_len", u64), ("infl_len", u64), ("type", C.c_int32), ("flags", C.c_uint32)]


class Result(C.Structure):
    _fields_ = [("clevel", C.c_uint8), ("window", C.c_uint8), ("memlevel", C.c_uint8), ("recomp", C.c_uint8),
                ("n_trials", C.c_uint32), ("ident", u64), ("first_diff", C.c_int64), ("n_diff", u64),
                ("diff_index", u64)]


class Stats(C.Structure):
    _fields_ = [(k, u64) for k in ("file_bytes", "n_streams", "n_recomp", "n_trials", "n_trials_shortcut",
                                   "n_rounds", "atz_bytes", "n_candidates", "n_continuations", "n_hazard")] + \
               [(k, C.c_double) for k in ("scan_ms", "sweep_ms", "write_ms", "total_ms", "k_trial_ms",
                                          "k_inflate_ms", "k_chains_ms", "k_other_ms")] + \
               [(k, u64) for k in ("k_trial_launches", "k_inflate_launches", "k_chains_launches",
                                   "k_trial_alg_bytes", "k_inflate_alg_bytes", "k_chains_alg_bytes",
                                   "trial_parsed_bytes")] + \
               [("k_match_ms", C.c_double)] + \
               [(k, u64) for k in ("k_match_launches", "k_match_positions", "n_trials_rerun", "n_fast_fallbacks",
                                   "trial_cyc_total", "trial_cyc_tree", "trial_cyc_emit", "trial_blocks",
                                   "trial_cyc_heap", "trial_cyc_fallback", "trial_symbols",
                                   "n_trials_speculative", "n_reinflated", "n_inflate_retries", "n_trials_replayed", "n_replay_checked",
                                   "n_trials_duplicate", "n_fast_restarts", "dev_bytes_peak", "dev_bytes_held",
                                   "n_trials_skipped")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


EXPORTS = ["atz_open", "atz_close", "atz_strerror", "atz_free", "atz_default_opts", "atz_scan", "atz_sweep",
           "atz_precompress", "atz_precompress_device", "atz_reconstruct", "atz_deflate", "atz_deflate_batch",
           "atz_inflate_batch", "atz_deflate_bound", "atz_shard_scan", "atz_shard_sweep", "atz_shard_piece",
           "atz_shard_assemble", "atz_reconstruct_device", "atz_deflate_batch_ex", "atz_set_strategies",
           "atz_set_containers", "atz_container_anchors", "atz_set_stitch", "atz_stitch_anchors",
           "atz_stitch_pieces", "atz_set_probe", "atz_probe_positions", "atz_set_deflaters",
           "atz_set_segments", "atz_flush_markers", "atz_inflate_segments", "atz_set_nesting", "atz_nest_stats"]

# zlib's strategy numbers (Z_FIXED, 4, is not supported); a strategy mask has bit k set for strategy k
STRATEGIES = {"filtered": 1, "huffman": 2, "rle": 3}


def _mask(names, table, noun):
    """Words (a sequence, or a comma-separated string) -> the mask with bit table[w] set for each; ValueError on an unknown word."""
    if isinstance(names, str):
        names = [w for w in names.split(",") if w]
    mask = 0
    for w in names:
        if w not in table:
            raise ValueError("unknown %s %r (known: %s)" % (noun, w, ", ".join(sorted(table))))
        mask |= 1 << table[w]
    return mask


def strategy_mask(names):
    """("filtered", "rle", ...) or a comma-separated string -> atz_set_strategies mask; ValueError on an unknown word."""
    return _mask(names, STRATEGIES, "strategy")


# containers whose raw deflate bodies a container mask makes the scan look for: bit number of each
CONTAINERS = {"zip": 0, "gzip": 1}


def container_mask(names):
    """("zip", "gzip") or a comma-separated string -> atz_set_containers mask; ValueError on an unknown word."""
    return _mask(names, CONTAINERS, "container")


# what a stitch mask makes the scan put together: bit number of each
STITCHERS = {"png": 0}


def stitch_mask(names):
    """("png",) or a comma-separated string -> atz_set_stitch mask; ValueError on an unknown word."""
    return _mask(names, STITCHERS, "stitcher")


# what a probe mask makes the scan test every byte position for: bit number of each
PROBES = {"deflate": 0}


def probe_mask(names):
    """("deflate",) or a comma-separated string -> atz_set_probe mask; ValueError on an unknown word."""
    return _mask(names, PROBES, "probe")


# deflater families beside zlib's that a deflater mask adds to the raw walk: bit number of each
DEFLATERS = {"gnu": 0}


def deflater_mask(names):
    """("gnu",) or a comma-separated string -> atz_set_deflaters mask; ValueError on an unknown word."""
    return _mask(names, DEFLATERS, "deflater")


# what a segments mask makes the scan split streams at: bit number of each
SEGMENTS = {"flush": 0}


def segments_mask(names):
    """("flush",) or a comma-separated string -> atz_set_segments mask; ValueError on an unknown word."""
    return _mask(names, SEGMENTS, "segment kind")


# The clevel byte of a descriptor: stitched << 7 | raw << 6 | strategy << 4 | level (csrc/atz_params.h).
def nest_depth(text):
    """ATZ_NEST's text (or an int) -> the nesting depth, 0-4; ValueError on anything else.  Empty text: 0."""
    if isinstance(text, bool):
        raise ValueError("nesting depth %r" % (text,))
    if isinstance(text, int):
        depth = text
    else:
        if text == "":
            return 0
        if not (text.isascii() and text.isdigit()):
            raise ValueError("nesting depth %r is not a decimal number" % (text,))
        depth = int(text)
    if not 0 <= depth <= 4:
        raise ValueError("nesting depth %d (0 to 4)" % depth)
    return depth


def _pack(strategy, level, raw, stitched):
    if raw and stitched:
        raise ValueError("a descriptor is raw or stitched, not both")
    if not (0 <= strategy <= 3 and 0 <= level <= 9) or (strategy >= 2 and level < 1):
        raise ValueError("strategy %d with level %d" % (strategy, level))
    return (int(bool(stitched)) << 7) | (int(bool(raw)) << 6) | (strategy << 4) | level


def _unpack(b):
    return bool(b & 0x80), bool(b & 0x40), (b >> 4) & 3, b & 15


def pack_clevel(strategy, level, raw=False):
    """The clevel byte of an ATZ2 / ATZ3 descriptor (and of atz_sweep's results): raw << 6 | strategy << 4 | level."""
    return _pack(strategy, level, raw, False)


def unpack_clevel(b):
    """-> (strategy, level) of a clevel byte."""
    return b >> 4, _unpack(b)[3]


def unpack_clevel3(b):
    """-> (raw, strategy, level) of an ATZ3 clevel byte."""
    return _unpack(b)[1:]


def pack_clevel4(strategy, level, raw=False, stitched=False):
    """The clevel byte of an ATZ4 descriptor: stitched << 7 | raw << 6 | strategy << 4 | level (never both)."""
    return _pack(strategy, level, raw, stitched)


def unpack_clevel4(b):
    """-> (stitched, raw, strategy, level) of an ATZ4 clevel byte."""
    return _unpack(b)


_lib = None


class AtzError(RuntimeError):
    """A libatz_accel call failed; `code` is its negative ATZ_E_* value (include/atz_accel.h), 0 if none."""

    def __init__(self, msg, code=0):
        super().__init__(msg)
        self.code = code


def lib():
    """Load libatz_accel.so; raise if it was not built (never fall back to the CPU)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AtzError("libatz_accel.so not built: run `python -m antiz_amd.build` (no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.atz_open.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Opts)]
        L.atz_close.argtypes = [C.c_void_p]
        L.atz_strerror.restype = C.c_char_p
        L.atz_strerror.argtypes = [C.c_int]
        L.atz_free.argtypes = [C.c_void_p]
        L.atz_default_opts.argtypes = [C.POINTER(Opts)]
        L.atz_scan.argtypes = [C.c_void_p, C.c_char_p, u64, C.POINTER(C.POINTER(Cand)), C.POINTER(u64)]
        L.atz_sweep.argtypes = [C.c_void_p, C.POINTER(Cand), u64, C.POINTER(Result), C.POINTER(C.POINTER(u64)),
                                C.POINTER(u8p), C.POINTER(u64)]
        L.atz_precompress.argtypes = [C.c_void_p, C.c_char_p, u64, C.POINTER(u8p), C.POINTER(u64), C.POINTER(Stats)]
        L.atz_precompress_device.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, u64, C.POINTER(C.c_void_p),
                                             C.POINTER(u64), C.POINTER(Stats)]
        L.atz_reconstruct.argtypes = [C.c_void_p, C.c_char_p, u64, C.POINTER(u8p), C.POINTER(u64)]
        L.atz_deflate.argtypes = [C.c_void_p, C.c_char_p, u64, C.c_int, C.c_int, C.c_int, C.c_char_p, u64,
                                  C.POINTER(u64)]
        L.atz_inflate_batch.argtypes = [C.c_void_p, C.c_char_p, u64, C.POINTER(u64), C.POINTER(u64), u64,
                                        C.POINTER(C.c_uint32), C.POINTER(u64), C.POINTER(u64)]
        L.atz_deflate_batch.argtypes = [C.c_void_p, C.c_char_p, u64, C.POINTER(u64), C.POINTER(u64),
                                        C.POINTER(C.c_uint32), u64, C.c_char_p, C.POINTER(u64), C.POINTER(u64),
                                        C.POINTER(u64)]
        L.atz_deflate_batch_ex.argtypes = L.atz_deflate_batch.argtypes
        L.atz_set_strategies.argtypes = [C.c_void_p, C.c_uint32]
        L.atz_set_containers.argtypes = [C.c_void_p, C.c_uint32]
        L.atz_container_anchors.argtypes = [C.c_void_p, C.c_char_p, u64, C.c_uint32, C.POINTER(C.POINTER(u64)),
                                            C.POINTER(u64)]
        L.atz_set_stitch.argtypes = [C.c_void_p, C.c_uint32]
        L.atz_stitch_anchors.argtypes = L.atz_container_anchors.argtypes
        L.atz_stitch_pieces.argtypes = [C.c_void_p, u64, C.POINTER(C.POINTER(u64)), C.POINTER(C.POINTER(u64)),
                                        C.POINTER(u64)]
        L.atz_set_probe.argtypes = [C.c_void_p, C.c_uint32]
        L.atz_probe_positions.argtypes = [C.c_void_p, C.c_char_p, u64, C.POINTER(C.POINTER(u64)), C.POINTER(u64)]
        L.atz_set_deflaters.argtypes = [C.c_void_p, C.c_uint32]
        L.atz_set_segments.argtypes = [C.c_void_p, C.c_uint32]
        L.atz_flush_markers.argtypes = L.atz_probe_positions.argtypes
        L.atz_inflate_segments.argtypes = [C.c_void_p, C.c_char_p, u64, C.POINTER(u64), C.POINTER(u64), u64,
                                           C.POINTER(C.c_uint32), C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_uint8)]
        L.atz_set_nesting.argtypes = [C.c_void_p, C.c_int]
        L.atz_nest_stats.argtypes = [C.c_void_p, C.c_int, C.POINTER(Stats)]
        L.atz_deflate_bound.restype = u64
        L.atz_deflate_bound.argtypes = [u64, C.c_int, C.c_int]
        L.atz_shard_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, u64, C.c_int, C.c_int, C.POINTER(u8p),
                                     C.POINTER(u64)]
        L.atz_shard_sweep.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, u64, C.POINTER(C.c_char_p),
                                      C.POINTER(u64), C.c_int, C.POINTER(u64), C.POINTER(u8p), C.POINTER(u64),
                                      C.POINTER(u64), C.POINTER(Stats)]
        L.atz_shard_piece.argtypes = [C.c_void_p, C.c_void_p]
        L.atz_reconstruct_device.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, u64, C.POINTER(C.c_void_p),
                                             C.POINTER(u64)]
        L.atz_shard_assemble.argtypes = [C.c_void_p, C.c_void_p, u64, C.c_char_p, u64, u64, u64, C.c_void_p, u64,
                                         C.POINTER(u64)]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise AtzError("atz error %d: %s" % (rc, lib().atz_strerror(rc).decode()), rc)


class Context:
    """One libatz_accel context (one GPU).  Mirrors the reference's programOptions (ATZData.h:7-35)."""

    def __init__(self, recomp_tresh=128, sizediff_tresh=128, shortcut_len=512, mismatch_tol=2,
                 chunksize=524288, brute_window=False, device=-1, strategies=None, containers=None, stitch=None,
                 probe=None, deflaters=None, segments=None, nest=None):
        """strategies: names of zlib strategies ("filtered", "rle", "huffman") to try on the streams the
        reference walk leaves unrecorded (an extension, off by default; None reads ATZ_STRATEGIES, a
        comma-separated list, as the CLI does).
        containers: "zip", "gzip": also look for the raw deflate bodies of ZIP entries and gzip members (an
        extension, off by default; None reads ATZ_CONTAINERS, a comma-separated list, as the CLI does).
        stitch: "png": also look for zlib streams split over the IDAT chunks of a PNG (an extension, off by
        default; None reads ATZ_STITCH, a comma-separated list, as the CLI does).
        probe: "deflate": also test every byte position for the start of a raw deflate stream that no header or
        container announces (an extension, off by default; None reads ATZ_PROBE, a comma-separated list, as the
        CLI does).
        deflaters: "gnu": the raw records' walk (containers, probe) also tries the deflater of GNU gzip and Info-ZIP's
        zip (an extension, off by default; None reads ATZ_DEFLATERS, a comma-separated list, as the CLI does).
        segments: "flush": a stream cut by full-flush points (Z_FULL_FLUSH, pigz -i) is recorded as one raw record per
        segment (an extension, off by default; None reads ATZ_SEGMENTS, a comma-separated list, as the CLI does).
        nest: a depth 1-4: precompress also runs the whole pipeline, that many levels down, on the payloads of the
        streams it recorded and writes a nested file, magic "ATN" 1 (an extension, off by default, 0; None reads ATZ_NEST,
        a decimal depth, as the CLI does)."""
        L = lib()
        self.o = Opts(recomp_tresh, sizediff_tresh, shortcut_len, mismatch_tol, chunksize, int(brute_window), device)
        if strategies is None:
            strategies = os.environ.get("ATZ_STRATEGIES", "")
        mask = strategy_mask(strategies)
        if containers is None:
            containers = os.environ.get("ATZ_CONTAINERS", "")
        cmask = container_mask(containers)
        if stitch is None:
            stitch = os.environ.get("ATZ_STITCH", "")
        smask = stitch_mask(stitch)
        if probe is None:
            probe = os.environ.get("ATZ_PROBE", "")
        pmask = probe_mask(probe)
        if deflaters is None:
            deflaters = os.environ.get("ATZ_DEFLATERS", "")
        dmask = deflater_mask(deflaters)
        if segments is None:
            segments = os.environ.get("ATZ_SEGMENTS", "")
        gmask = segments_mask(segments)
        if nest is None:
            nest = os.environ.get("ATZ_NEST", "")
        depth = nest_depth(nest)
        self.h = C.c_void_p()
        _check(L.atz_open(C.byref(self.h), C.byref(self.o)))
        if mask:
            _check(L.atz_set_strategies(self.h, mask))
        if cmask:
            _check(L.atz_set_containers(self.h, cmask))
        if smask:
            _check(L.atz_set_stitch(self.h, smask))
        if pmask:
            _check(L.atz_set_probe(self.h, pmask))
        if dmask:
            _check(L.atz_set_deflaters(self.h, dmask))
        if gmask:
            _check(L.atz_set_segments(self.h, gmask))
        if depth:
            _check(L.atz_set_nesting(self.h, depth))

    def close(self):
        if self.h:
            lib().atz_close(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def precompress(self, data):
        L = lib()
        p = u8p()
        n = u64(0)
        st = Stats()
        _check(L.atz_precompress(self.h, data, len(data), C.byref(p), C.byref(n), C.byref(st)))
        out = C.string_at(p, n.value)
        L.atz_free(p)
        return out, st.as_dict()

    def nest_stats(self, level):
        """The stats of nesting level `level` (0: this context's own) of the last precompress; AtzError (ATZ_E_ARG) if
        that level did not run."""
        st = Stats()
        _check(lib().atz_nest_stats(self.h, level, C.byref(st)))
        return st.as_dict()

    def precompress_device(self, d_ptr, host_data):
        """Input already resident in HBM (d_ptr: device pointer, e.g. torch tensor.data_ptr())."""
        L = lib()
        dp = C.c_void_p()
        n = u64(0)
        st = Stats()
        _check(L.atz_precompress_device(self.h, C.c_void_p(d_ptr), host_data, len(host_data), C.byref(dp),
                                        C.byref(n), C.byref(st)))
        return dp.value, n.value, st.as_dict()

    # ---- one file over several GPUs (antiz_amd.shard drives these with torch.distributed) ----
    def shard_scan(self, d_ptr, host_data, rank, world):
        L = lib()
        p = u8p()
        n = u64(0)
        _check(L.atz_shard_scan(self.h, C.c_void_p(d_ptr), host_data, len(host_data), rank, world, C.byref(p),
                                C.byref(n)))
        out = C.string_at(p, n.value)
        L.atz_free(p)
        return out

    def shard_sweep(self, d_ptr, host_data, blobs):
        """-> (piece_len, recomp flags (bytes, one per record of this rank), n_recomp, stats)"""
        L = lib()
        k = len(blobs)
        bp = (C.c_char_p * k)(*blobs)
        bl = (u64 * k)(*[len(b) for b in blobs])
        pl, nf, nr = u64(0), u64(0), u64(0)
        fp = u8p()
        st = Stats()
        _check(L.atz_shard_sweep(self.h, C.c_void_p(d_ptr), host_data, len(host_data), bp, bl, k, C.byref(pl),
                                 C.byref(fp), C.byref(nf), C.byref(nr), C.byref(st)))
        flags = C.string_at(fp, nf.value)
        L.atz_free(fp)
        return pl.value, flags, nr.value, st.as_dict()

    def shard_piece(self, d_dst):
        _check(lib().atz_shard_piece(self.h, C.c_void_p(d_dst)))

    def shard_assemble(self, d_ptr, file_len, flags, n_recomp, pieces_len, d_atz, cap):
        n = u64(0)
        _check(lib().atz_shard_assemble(self.h, C.c_void_p(d_ptr), file_len, flags, len(flags), n_recomp,
                                        pieces_len, C.c_void_p(d_atz), cap, C.byref(n)))
        return n.value

    def reconstruct(self, atz):
        L = lib()
        p = u8p()
        n = u64(0)
        _check(L.atz_reconstruct(self.h, atz, len(atz), C.byref(p), C.byref(n)))
        out = C.string_at(p, n.value)
        L.atz_free(p)
        return out

    def reconstruct_device(self, d_atz, host_atz):
        """ATZ1 bytes already in HBM (d_atz: device pointer); returns (device pointer, length) of the original."""
        dp = C.c_void_p()
        n = u64(0)
        _check(lib().atz_reconstruct_device(self.h, C.c_void_p(d_atz), host_atz, len(host_atz), C.byref(dp),
                                            C.byref(n)))
        return dp.value, n.value

    def scan(self, data):
        L = lib()
        p = C.POINTER(Cand)()
        n = u64(0)
        _check(L.atz_scan(self.h, data, len(data), C.byref(p), C.byref(n)))
        recs = [(p[i].offset, p[i].type, p[i].comp_len, p[i].infl_len, p[i].flags) for i in range(n.value)]
        self._cands = (p, n.value)
        return recs

    def sweep(self):
        L = lib()
        p, n = self._cands
        res = (Result * max(n, 1))()
        do = C.POINTER(u64)()
        dv = u8p()
        nd = u64(0)
        _check(L.atz_sweep(self.h, p, n, res, C.byref(do), C.byref(dv), C.byref(nd)))
        out = [{k: getattr(res[i], k) for k, _ in Result._fields_} for i in range(n)]
        diffs = ([do[i] for i in range(nd.value)], bytes(dv[i] for i in range(nd.value)))
        L.atz_free(do)
        L.atz_free(dv)
        L.atz_free(p)
        self._cands = None
        return out, diffs

    def container_anchors(self, data, mask):
        """The anchor kernel's list for `data` (parity/debug): [(position, kind)], kind 0 ZIP, 1 gzip."""
        L = lib()
        p = C.POINTER(u64)()
        n = u64(0)
        _check(L.atz_container_anchors(self.h, data, len(data), mask, C.byref(p), C.byref(n)))
        out = [(p[i] >> 5, p[i] & 31) for i in range(n.value)]
        L.atz_free(p)
        return out

    def stitch_anchors(self, data, mask=1):
        """The IDAT anchors of `data` (parity/debug): [(position of the chunk type field, 2)], ascending."""
        L = lib()
        p = C.POINTER(u64)()
        n = u64(0)
        _check(L.atz_stitch_anchors(self.h, data, len(data), mask, C.byref(p), C.byref(n)))
        out = [(p[i] >> 5, p[i] & 31) for i in range(n.value)]
        L.atz_free(p)
        return out

    def probe_positions(self, data):
        """The probe kernel's list for `data` (parity/debug): the surviving positions, ascending."""
        L = lib()
        p = C.POINTER(u64)()
        n = u64(0)
        _check(L.atz_probe_positions(self.h, data, len(data), C.byref(p), C.byref(n)))
        out = [p[i] for i in range(n.value)]
        L.atz_free(p)
        return out

    def flush_markers(self, data):
        """The marker kernel's list for `data` (parity/debug): every q with data[q:q+4] == 00 00 FF FF, ascending."""
        L = lib()
        p = C.POINTER(u64)()
        n = u64(0)
        _check(L.atz_flush_markers(self.h, data, len(data), C.byref(p), C.byref(n)))
        out = [p[i] for i in range(n.value)]
        L.atz_free(p)
        return out

    def stitch_pieces(self, record):
        """[(file offset, length)] of the pieces of stitched record `record` of the last scan ([]: not stitched)."""
        L = lib()
        po, pl = C.POINTER(u64)(), C.POINTER(u64)()
        k = u64(0)
        _check(L.atz_stitch_pieces(self.h, record, C.byref(po), C.byref(pl), C.byref(k)))
        out = [(po[i], pl[i]) for i in range(k.value)]
        L.atz_free(po)
        L.atz_free(pl)
        return out

    def deflate(self, data, clevel, window, memlevel, strategy=0, raw=False, deflater=None, flush=False):
        """deflater: None zlib 1.2.8's; "gnu" GNU gzip's and Info-ZIP's (raw, window 15, strategy 0, level 1-9 only;
        memlevel is ignored).  flush: the body ends as deflate(Z_FULL_FLUSH) ends it (raw, zlib's, strategy 0 only)."""
        if strategy or raw or deflater or flush:
            return self.deflate_batch(data, [(0, len(data), clevel, window, memlevel, strategy, raw, deflater, flush)])[0]
        L = lib()
        cap = L.atz_deflate_bound(len(data), 10, 1) + 1024
        out = C.create_string_buffer(cap)
        n = u64(0)
        _check(L.atz_deflate(self.h, data, len(data), clevel, window, memlevel, out, cap, C.byref(n)))
        return out.raw[:n.value]

    def deflate_batch(self, buf, items):
        """items: list of (offset, length, clevel, window, memlevel[, strategy[, raw[, deflater[, flush]]]]) over `buf`;
        returns list of bytes.  raw: the deflate body alone (no zlib header, no Adler-32 trailer).  deflater, flush: see
        deflate()."""
        L = lib()
        k = len(items)
        offs = (u64 * max(k, 1))(*[it[0] for it in items])
        lens = (u64 * max(k, 1))(*[it[1] for it in items])
        ex = any(any(it[5:9]) for it in items)
        prm = (C.c_uint32 * max(k, 1))(*[((1 << 30) if len(it) > 8 and it[8] else 0) |
                                         ((deflater_mask((it[7],)) << 29) if len(it) > 7 and it[7] else 0) |
                                         ((1 << 28) if len(it) > 6 and it[6] else 0) |
                                         ((it[5] << 24) if len(it) > 5 else 0) | (it[2] << 16) | (it[3] << 8) | it[4]
                                         for it in items])
        caps = [L.atz_deflate_bound(it[1], 10, 1) + 64 for it in items]
        oo, tot = [], 0
        for cp in caps:
            oo.append(tot)
            tot += cp
        out = C.create_string_buffer(max(tot, 1))
        ooff = (u64 * max(k, 1))(*oo)
        ocap = (u64 * max(k, 1))(*caps)
        olen = (u64 * max(k, 1))()
        fn = L.atz_deflate_batch_ex if ex else L.atz_deflate_batch
        _check(fn(self.h, buf, len(buf), offs, lens, prm, k, out, ooff, ocap, olen))
        raw = out.raw
        return [raw[oo[i]:oo[i] + olen[i]] for i in range(k)]

    def inflate_batch(self, buf, ranges):
        L = lib()
        k = len(ranges)
        offs = (u64 * max(k, 1))(*[a for a, _ in ranges])
        lens = (u64 * max(k, 1))(*[b for _, b in ranges])
        st = (C.c_uint32 * max(k, 1))()
        co = (u64 * max(k, 1))()
        pr = (u64 * max(k, 1))()
        _check(L.atz_inflate_batch(self.h, buf, len(buf), offs, lens, k, st, co, pr))
        return [(st[i], co[i], pr[i]) for i in range(k)]

    def inflate_segments(self, buf, ranges):
        """inflate_batch on raw deflate bodies with the segment decoder, which also ends (status 0) at a flush
        marker: [(status, consumed, produced, at_marker)]."""
        L = lib()
        k = len(ranges)
        offs = (u64 * max(k, 1))(*[a for a, _ in ranges])
        lens = (u64 * max(k, 1))(*[b for _, b in ranges])
        st = (C.c_uint32 * max(k, 1))()
        co = (u64 * max(k, 1))()
        pr = (u64 * max(k, 1))()
        am = (C.c_uint8 * max(k, 1))()
        _check(L.atz_inflate_segments(self.h, buf, len(buf), offs, lens, k, st, co, pr, am))
        return [(st[i], co[i], pr[i], bool(am[i])) for i in range(k)]
