/*
 * atz_accel.h -- C ABI of libatz_accel.so, the MI355X (gfx950) replacement for AntiZ's codec boundary.
 *
 * The reference talks to zlib directly (ZlibWrapper.h:25-100 for the scanner, raw zlib calls in
 * main.cpp for the sweep, the writer and the reconstructor).  Those calls are per stream and per
 * trial; this ABI is per FILE: one call runs a whole phase on the GPU.  Plain pointers and sizes,
 * no C++ or torch types, negative error codes, no exceptions.  Library-owned arrays are released
 * with atz_free().  One context per process and per GPU; not shared across threads.
 *
 * Reference interface each entry point replaces (file:line in /root/reference):
 *   atz_scan        ATZcreator::searchInfile + ZBuffSearcher + ZlibInflator   main.cpp:392-420, 149-249;
 *                   ZlibWrapper.h:58-82 (inflateReset/inflate(Z_SYNC_FLUSH)/continuePrev/refillInput)
 *   atz_sweep       findDeflateParams_ALL .. testDeflateParams + doInflate     main.cpp:421-763
 *                   (deflateInit2/deflateBound/deflate(Z_FINISH)x2/deflateEnd, inflate(Z_FINISH))
 *   atz_precompress Phase1 + Phase3 + Phase4 (writeATZfile, main.cpp:764-834)  main.cpp:1216-1221
 *   atz_reconstruct ATZreconstructor::reconstructATZ + doDeflate               main.cpp:869-1003
 *   atz_deflate     one deflateInit2/deflate(Z_FINISH)/deflateEnd              main.cpp:976-1003
 *   atz_shard_*     the precompress of one file split over several GPUs (new: the reference is
 *                   single-threaded)
 * Six opt-in extensions, each off by default and leaving every output as the reference's while off:
 *   atz_set_strategies  zlib strategy trials ("ATZ\2"), atz_set_containers  raw deflate in ZIP / gzip ("ATZ\3"),
 *   atz_set_stitch      zlib streams split over PNG IDAT chunks ("ATZ\4"),
 *   atz_set_probe       raw deflate streams that nothing announces ("ATZ\3"),
 *   atz_set_deflaters   raw bodies written by GNU gzip's and Info-ZIP's deflater, not zlib's ("ATZ\5"),
 *   atz_set_segments    streams cut by full-flush points, one raw record per segment ("ATZ\6")
 * and one that runs the whole pipeline again on what they recorded:
 *   atz_set_nesting     the streams inside the recorded streams' payloads, a nested file ("ATN\1")
 */
#ifndef ATZ_ACCEL_H
#define ATZ_ACCEL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct atz_ctx atz_ctx_t;

/* ATZdata::programOptions (ATZData.h:7-35).  The thresholds are uint_fast16_t in the reference,
 * i.e. 64-bit on x86-64 glibc; they are uint64_t here so the unsigned wrap of main.cpp:649 is kept. */
typedef struct {
    uint64_t recomp_tresh;    /* default 128 */
    uint64_t sizediff_tresh;  /* default 128 */
    uint64_t shortcut_len;    /* default 512 */
    uint64_t mismatch_tol;    /* default 2 */
    uint64_t chunksize;       /* default 524288 */
    int32_t  brute_window;    /* default 0 */
    int32_t  device;          /* HIP device ordinal (-1: current) */
} atz_opts_t;

/* ATZdata::streamOffset after Phase 1 (ATZData.h:46-58). */
typedef struct {
    uint64_t offset;
    uint64_t comp_len;   /* streamLength */
    uint64_t infl_len;   /* inflatedLength */
    int32_t  type;       /* offsetType 0..23; 24 + hint for a raw deflate body behind a ZIP or gzip header
                            (only with atz_set_containers; hint 0 none, 1 fast, 2 max): offset is the
                            body's first byte, comp_len the body's length; 24 also for a raw stream the probe
                            found (only with atz_set_probe) */
    uint32_t flags;      /* bit0: recorded through a chunk-boundary continuation; bit1: the first block is
                            dynamic and codes matches but none of length 3-5 (a Z_FILTERED-like stream: the
                            multi-GPU split's cost hint, not part of the reference's record); bits 2-5:
                            the memLevel (1-9) whose lit_bufsize - 1 symbols the first block holds when
                            more blocks follow, else 0 (a sweep hint, likewise not the reference's); bit 6: a
                            stitched record (only with atz_set_stitch): a zlib stream split over k >= 2 PNG IDAT
                            chunks -- offset is its first payload byte, comp_len its length in stream bytes, and
                            it occupies [offset, offset + comp_len + 12 (k - 1)) of the file (atz_stitch_pieces);
                            bit 7: a flush-terminated segment (only with atz_set_segments): a raw record (type
                            24-26) that ends with a full flush's empty stored block, not with a final block */
} atz_cand_t;

/* ATZdata::streamOffset after Phase 3. */
typedef struct {
    uint8_t  clevel, window, memlevel, recomp;
    uint32_t n_trials;       /* trials evaluated (diagnostic) */
    uint64_t ident;          /* identBytes */
    int64_t  first_diff;     /* firstDiffByte (-1: none) */
    uint64_t n_diff;         /* diffByteOffsets.size() (written only for recomp streams) */
    uint64_t diff_index;     /* first entry of this stream in the diff arrays */
} atz_result_t;

typedef struct {
    uint64_t file_bytes, n_streams, n_recomp, n_trials, n_trials_shortcut, n_rounds, atz_bytes;
    uint64_t n_candidates, n_continuations, n_hazard;
    double scan_ms, sweep_ms, write_ms, total_ms;       /* device-synchronised wall times */
    /* per-kernel device time (HIP events on the library's stream) and algorithmic bytes */
    double k_trial_ms, k_inflate_ms, k_chains_ms, k_other_ms;
    uint64_t k_trial_launches, k_inflate_launches, k_chains_launches;
    uint64_t k_trial_alg_bytes, k_inflate_alg_bytes, k_chains_alg_bytes;
    uint64_t trial_parsed_bytes;                         /* inflated bytes the trials actually parsed */
    double k_match_ms;                                   /* match-table kernel (longest_match per position) */
    uint64_t k_match_launches, k_match_positions;
    uint64_t n_trials_rerun;                             /* trials run again after extending their match table */
    uint64_t n_fast_fallbacks;                           /* fast-level steps that walked a chain in the parse */
    uint64_t trial_cyc_total, trial_cyc_tree, trial_cyc_emit, trial_blocks;  /* shader clocks summed over trials */
    uint64_t trial_cyc_heap, trial_cyc_fallback, trial_symbols;   /* heap: ATZ_STEP_CLOCKS builds only */
    uint64_t n_trials_speculative;                       /* trials run ahead of a stream's stop and discarded */
    uint64_t n_reinflated;                               /* recorded streams inflated again (scan output not kept) */
    uint64_t n_inflate_retries;                          /* inflates rerun with the 32 KiB history ring */
    uint64_t n_trials_replayed;                          /* trials that replayed a saved symbol sequence */
    uint64_t n_replay_checked;                           /* replays offered under a match-table check (passed or not) */
    uint64_t n_trials_duplicate;                         /* replays whose output equals their saver's: not launched */
    uint64_t n_fast_restarts;                            /* fast-level exact walks that changed the parse path */
    /* device memory the library held in this process (every context's buffers): the peak during the call,
       and what stays allocated after it (kept for the next call's reuse) */
    uint64_t dev_bytes_peak, dev_bytes_held;
    uint64_t n_trials_skipped;                           /* speculative trials ended by an earlier trial's stop */
} atz_stats_t;

enum {
    ATZ_OK = 0,
    ATZ_E_ARG = -1,          /* bad argument */
    ATZ_E_NODEV = -2,        /* no HIP device / kernels not loadable */
    ATZ_E_HIP = -3,          /* HIP runtime error */
    ATZ_E_NOMEM = -4,        /* device or host allocation failed */
    ATZ_E_REF_ABORT = -5,    /* the reference would abort() here (e.g. main.cpp:450-452, 663-665) */
    ATZ_E_REF_UB = -6,       /* the reference has undefined behaviour on this input (documented) */
    ATZ_E_FORMAT = -7,       /* invalid ATZ file (main.cpp:1018-1025) */
    ATZ_E_INTERNAL = -8
};

int  atz_open(atz_ctx_t **ctx, const atz_opts_t *opts);
void atz_close(atz_ctx_t *ctx);
const char *atz_strerror(int err);
void atz_free(void *p);
void atz_default_opts(atz_opts_t *opts);

/* Phase 1: the reference's chunked scan.  *out (atz_free) receives *n records in scan order. */
int atz_scan(atz_ctx_t *ctx, const uint8_t *file, uint64_t len, atz_cand_t **out, uint64_t *n);

/* Phase 3 on the streams of the LAST atz_scan of this context (cands must be that array).  Returns
 * ATZ_E_ARG unless atz_scan was the previous call on ctx (any other call replaces its records); the
 * scanned host buffer need not stay alive (atz_scan keeps what the sweep needs: the file on the
 * device, each stream's Adler-32 trailer).  One atz_sweep per atz_scan.
 * res[n] is caller-allocated.  *diff_off / *diff_val (atz_free) hold n_diffs delta-encoded entries. */
int atz_sweep(atz_ctx_t *ctx, const atz_cand_t *cands, uint64_t n, atz_result_t *res,
              uint64_t **diff_off, uint8_t **diff_val, uint64_t *n_diffs);

/* Whole precompress of a host buffer: *atz (atz_free) receives the ATZ1 bytes (a nested file's, "ATN\1", under
 * atz_set_nesting). */
int atz_precompress(atz_ctx_t *ctx, const uint8_t *file, uint64_t len, uint8_t **atz, uint64_t *atz_len,
                    atz_stats_t *stats);

/* Benchmark entry: the input is already resident in HBM (d_file, a device pointer allocated by the
 * caller with >= 4096 bytes of slack after len) and a host copy is given for host-side bookkeeping.
 * The ATZ1 bytes are assembled in device memory; *d_atz (device pointer, owned by ctx, valid until
 * the next call) and *atz_len receive them. */
int atz_precompress_device(atz_ctx_t *ctx, const uint8_t *d_file, const uint8_t *h_file, uint64_t len,
                           const uint8_t **d_atz, uint64_t *atz_len, atz_stats_t *stats);

/* -r: rebuild the original from ATZ1 bytes (or a nested file's, atz_set_nesting). *out (atz_free). */
int atz_reconstruct(atz_ctx_t *ctx, const uint8_t *atz, uint64_t len, uint8_t **out, uint64_t *out_len);

/* -r with the ATZ1 bytes resident in HBM (d_atz, >= 4096 bytes of slack; h_atz: host copy for the
 * descriptors): *d_out (device, owned by ctx, valid until the next call) receives *out_len bytes. */
int atz_reconstruct_device(atz_ctx_t *ctx, const uint8_t *d_atz, const uint8_t *h_atz, uint64_t len,
                           const uint8_t **d_out, uint64_t *out_len);

/* One zlib-1.2.8-exact deflate (level 0..9, windowBits 9..15, memLevel 1..9, default strategy). */
int atz_deflate(atz_ctx_t *ctx, const uint8_t *in, uint64_t in_len, int clevel, int window, int memlevel,
                uint8_t *out, uint64_t out_cap, uint64_t *out_len);

/* Batch of independent one-shot deflates of ranges of a host buffer; params[i] = (clevel<<16)|(window<<8)|memlevel.
 * Output i is written at out + out_offs[i] (capacity out_caps[i]); out_lens[i] receives its length. */
int atz_deflate_batch(atz_ctx_t *ctx, const uint8_t *buf, uint64_t len, const uint64_t *offs, const uint64_t *lens,
                      const uint32_t *params, uint64_t n, uint8_t *out, const uint64_t *out_offs,
                      const uint64_t *out_caps, uint64_t *out_lens);

/* atz_deflate_batch with zlib's strategy: params[i] = (strategy<<24)|(clevel<<16)|(window<<8)|memlevel,
 * strategy 0 default, 1 Z_FILTERED, 2 Z_HUFFMAN_ONLY, 3 Z_RLE (zlib's numbering; Z_FIXED is not supported).
 * Levels 0..9 for strategies 0-1 (levels 0-3 ignore Z_FILTERED, as zlib does), 1..9 for strategies 2-3. */
int atz_deflate_batch_ex(atz_ctx_t *ctx, const uint8_t *buf, uint64_t len, const uint64_t *offs, const uint64_t *lens,
                         const uint32_t *params, uint64_t n, uint8_t *out, const uint64_t *out_offs,
                         const uint64_t *out_caps, uint64_t *out_lens);

/* Opt-in strategy trials (an extension: the reference never sweeps the strategy).  mask bit k (k = 1..3)
 * names zlib strategy k; 0, the default, is off and leaves every output as the reference's.  With a mask,
 * the precompress and sweep calls give each stream the reference walk leaves unrecorded a second walk,
 * under the same rule, over the masked strategies that its header's FLEVEL allows.  A stream recorded so
 * reports clevel = strategy<<4 | level, and a file that holds one is written with the magic "ATZ\2" (same
 * layout; the reference cannot read it), else the file is the ATZ1 of a context without a mask.
 * atz_reconstruct* read both.  The atz_shard_* calls return ATZ_E_ARG on a context with a mask. */
int atz_set_strategies(atz_ctx_t *ctx, uint32_t mask);

/* Opt-in container anchors (an extension: the reference only knows the 24 zlib headers).  mask bit 0: ZIP
 * local file headers, bit 1: gzip members; 0, the default, is off and leaves every output as the
 * reference's.  With a mask, the scan also lists the raw deflate bodies behind such headers that decode to
 * their end, agree with the container's size fields and meet no reference record (atz_cand_t.type 24 +
 * hint), and the precompress and sweep calls walk each under the reference's rule over window 15,
 * memLevels 8, 9, 7..1 and levels 0..9 in the order the container's hint suggests.  A body recorded so
 * reports clevel = 1<<6 | level, and a file that holds one is written with the magic "ATZ\3" (same layout,
 * clevel = raw<<6 | strategy<<4 | level; the reference cannot read it), else the file is what a context
 * without this mask writes.  atz_reconstruct* read all three.  In atz_deflate_batch_ex, bit 28 of a params
 * word asks for raw output: no zlib header and no Adler-32 trailer.  The atz_shard_* calls return
 * ATZ_E_ARG on a context with a mask. */
int atz_set_containers(atz_ctx_t *ctx, uint32_t mask);

/* The anchor kernel's list for a host buffer (parity/debug): *out (atz_free) receives *n entries,
 * position << 5 | kind (0 ZIP, 1 gzip), ascending.  A ZIP anchor at p: bytes 50 4B 03 04, p + 30 <= len,
 * method 8, not encrypted.  A gzip anchor: bytes 1F 8B 08, no reserved FLG bit, p + 18 <= len. */
int atz_container_anchors(atz_ctx_t *ctx, const uint8_t *file, uint64_t len, uint32_t mask, uint64_t **out,
                          uint64_t *n);

/* Opt-in stitching (an extension: the reference only decodes contiguous streams).  mask bit 0: PNG IDAT
 * chains; 0, the default, is off and leaves every output as what a context without this mask writes.  A PNG
 * writer cuts its one zlib stream into IDAT chunks, so 12 framing bytes (CRC, length, "IDAT") interrupt it
 * every few KiB and the scan's decode fails there.  With the mask, the scan also links consecutive IDAT
 * chunks into chains, decodes each chain's concatenated payloads, and lists a stream that ends (Adler-32
 * checked), crosses a chunk boundary and whose hull meets no other record: atz_cand_t.type is its header's
 * 0..23, flags bit 6 is set.  The precompress and sweep calls walk it as any stream of its type (the
 * reference walk, then the strategy walk under atz_set_strategies).  A file that records one is written with
 * the magic "ATZ\4": clevel = stitched<<7 | raw<<6 | strategy<<4 | level (never both of bits 6 and 7), and a
 * stitched descriptor carries, after its inflated payload, u32 k and k x u32 piece lengths (little-endian;
 * piece i starts at offset + sum_{j<i} (len_j + 12); diff positions are stream positions; the framing bytes
 * are residue).  Else the file is what a context without this mask writes.  atz_reconstruct* read all four.
 * atz_sweep's clevel never carries bit 7.  The atz_shard_* calls return ATZ_E_ARG on a context with a mask. */
int atz_set_stitch(atz_ctx_t *ctx, uint32_t mask);

/* The IDAT anchors of a host buffer (parity/debug): *out (atz_free) receives *n entries, position << 5 | 2,
 * ascending.  An anchor at a: a >= 4, bytes 49 44 41 54 at a, the big-endian length L at a - 4 is below 2^31
 * and a + 8 + L <= len.  mask as in atz_set_stitch. */
int atz_stitch_anchors(atz_ctx_t *ctx, const uint8_t *file, uint64_t len, uint32_t mask, uint64_t **out,
                       uint64_t *n);

/* The pieces of record `record` of the last atz_scan (before its atz_sweep): *offs and *lens (atz_free both)
 * receive the file offset and the length of each of its *k pieces; *k = 0 for a record that is not stitched. */
int atz_stitch_pieces(atz_ctx_t *ctx, uint64_t record, uint64_t **offs, uint64_t **lens, uint64_t *k);

/* Opt-in probe (an extension: raw deflate streams that no zlib header and no container announces).  mask bit
 * 0: streams whose first block is dynamic; 0, the default, is off and leaves every output as what a context
 * without this mask writes.  With the mask, the scan tests every byte position p of the file, reading bits
 * LSB-first from byte p: bits 1-2 = 2 (BTYPE dynamic), HLIT (bits 3-7) <= 29, HDIST (bits 8-12) <= 29, with nc
 * = (bits 13-16) + 4 all 17 + 3 nc header bits inside the file, and the nc 3-bit code-length-code lengths l != 0
 * a complete code (sum of 2^(7 - l) = 128).  A surviving position outside every record made before (the
 * reference's, the container extension's, a stitched record's hull) is decoded as a raw stream to the end of
 * the file; one that ends with 256 <= output < 2^31 bytes, meets no such record and does not start inside the
 * probe record kept before it becomes a record of atz_cand_t.type 24 (raw, no hint), walked, reported and
 * written ("ATZ\3") exactly as a container's body is.  Streams whose first block is stored or fixed are not
 * looked for.  The atz_shard_* calls return ATZ_E_ARG on a context with a mask. */
int atz_set_probe(atz_ctx_t *ctx, uint32_t mask);

/* The probe kernel's list for a host buffer (parity/debug): *out (atz_free) receives the *n surviving
 * positions, ascending, as plain positions. */
int atz_probe_positions(atz_ctx_t *ctx, const uint8_t *file, uint64_t len, uint64_t **out, uint64_t *n);

/* Opt-in deflater families (an extension: the raw walk only knows zlib 1.2.8's deflater).  mask bit 0: "gnu",
 * the deflater of GNU gzip and of Info-ZIP's zip (one family: zlib's parse at memLevel 8 and zlib's trees, but
 * blocks of up to 32 767 symbols that, for levels above 2, may end at every 4 096th symbol); 0, the default, is
 * off and leaves every output as what a context without this mask writes.  The mask acts on raw records only
 * (atz_cand_t.type 24-26, from atz_set_containers and atz_set_probe; alone it changes nothing): their walk
 * gets nine more candidates, levels 1-9 in the hint's order, directly behind the memLevel-8 group (positions
 * 10-18 of 99).  A body recorded so reports clevel = 1<<6 | level, window 15 and memLevel 0, and a file that
 * holds one is written with the magic "ATZ\5" (version 4's layout; memLevel byte 0 only on such a descriptor),
 * else the file is what a context without this mask writes.  atz_reconstruct* read every version.  In
 * atz_deflate_batch_ex, bit 29 of a params word asks for this deflater: only with bit 28, window 15, strategy
 * 0 and level 1-9 (else ATZ_E_ARG); the memLevel field is ignored.  The atz_shard_* calls return ATZ_E_ARG on
 * a context with a mask. */
int atz_set_deflaters(atz_ctx_t *ctx, uint32_t mask);

/* Opt-in segments (an extension: a stream cut by full-flush points -- deflate(.., Z_FULL_FLUSH), pigz -i,
 * dictzip-style seekable gzip -- is recorded by no one-shot deflate).  mask bit 0: "flush"; 0, the default, is off
 * and leaves every output as what a context without this mask writes.  After a full flush zlib starts from a
 * fresh state, so such a stream is a chain of independent raw bodies, each the one-shot deflate of its bytes but
 * for its end: no block is final, an empty last block is absent, and three zero bits, padding to a byte and
 * 00 00 FF FF follow.  With the mask, the scan lists every position q with bytes q..q+3 = 00 00 FF FF; a record
 * is eligible if it is raw (type 24-26; body = the record) or a zlib record whose header says window 15 and that
 * is not stitched (body = the record without its 2 header and 4 trailer bytes), and holds a marker with
 * body_start <= q and q + 4 < body_end.  The body's start and every such q + 4 are decoded as raw streams that
 * also end at the first stored block with BFINAL = 0 and LEN = 0.  The chain s_0 = body_start, s_(i+1) = s_i +
 * consumed_i over decodes that ended at such a block with output completes when it reaches one that ended at a
 * final block exactly at body_end, after at least one marker, with the outputs summing to the record's infl_len.
 * Then the record is replaced, in file order, by its segments {s_i, consumed_i, produced_i} of type 24 + hint (a
 * raw parent's; a zlib parent's FLEVEL 0 and 1 give 25, 2 gives 24, 3 gives 26), every one but the last with
 * atz_cand_t.flags bit 7; a last segment without output makes no record; a zlib parent's header and trailer
 * become residue.  Any other record stays exactly as it is.  Segments are walked as raw records are (window 15,
 * the default strategy; a bit-7 segment's trials end as a full flush does, and it gets no GNU candidates).  A
 * recorded bit-7 segment reports clevel = 1<<6 | level and window 0x8F, and a file that holds one is written with
 * the magic "ATZ\6" (version 5's layout; window byte 0x8F only on such a descriptor), else the file is what a
 * context without this mask writes.  atz_reconstruct* read all six.  In atz_deflate_batch_ex, bit 30 of a params
 * word asks for a flush-terminated body: only with bit 28, without bit 29, strategy 0 and windows 9-15 (else
 * ATZ_E_ARG).  The atz_shard_* calls return ATZ_E_ARG on a context with a mask. */
int atz_set_segments(atz_ctx_t *ctx, uint32_t mask);

/* Opt-in nesting (an extension: the reference stops one level down -- a recorded stream's inflated payload goes
 * into the file as opaque bytes, so the streams inside a .tar.gz's tar, a JAR in a WAR entry or a PDF object stream
 * stay compressed).  depth 0, the default, is off: no code of the extension runs and every output is what a context
 * without it writes; depth 1-4 is accepted, anything else is ATZ_E_ARG.  With a depth d >= 1, atz_precompress* run
 * level 0 as ever; if it recorded a stream, P -- the recorded streams' payloads, concatenated in descriptor order with
 * no padding, gathered on the device and copied once to the host -- is precompressed as if it were a file, with the
 * same options, the same six masks and depth d - 1, in a child context on the same device that this context owns,
 * opens at the first need, keeps and closes with itself.  If the child recorded a stream, the output is a nested file:
 *   "ATN" 1 | u64 length (whole file) | u64 outer_len | outer (outer_len bytes) | inner (to the end)
 * outer: the ATZ file (version 1-6, its own length field = outer_len, at least one descriptor) without every
 * descriptor's infl_len payload bytes -- a stitched descriptor's piece list then directly follows its diff list or
 * fixed fields; inner: the child's file (ATZ 1-6 or ATN), whose length field is what is left of the file and whose
 * origlen is the sum of the outer's infl_len; payload j of the outer is bytes [sum_{i<j} il_i, + il_j) of the inner's
 * original.  If the child recorded none, or P is empty, or the child returned ATZ_E_REF_ABORT or ATZ_E_REF_UB (the
 * reference itself would have died on P), the output is byte for byte what depth 0 writes; any other error of the
 * child fails the call.  *stats is level 0's but for atz_bytes and total_ms, which cover the whole file and call.
 * atz_reconstruct* read a nested file on any context, whatever its depth (at most 8 levels: deeper is
 * ATZ_E_FORMAT): the child rebuilds the inner file's original in HBM and the outer's payloads are read from there.
 * atz_scan and atz_sweep are level 0 only and unchanged.  The atz_shard_* calls return ATZ_E_ARG on a context
 * with a depth. */
int atz_set_nesting(atz_ctx_t *ctx, int depth);

/* The stats of level `level` (0: this context's own, 1: its child's, ...) of the last atz_precompress* on ctx;
 * ATZ_E_ARG if that level did not run in it (no depth, no recorded stream or an empty P one level up, a failed child). */
int atz_nest_stats(atz_ctx_t *ctx, int level, atz_stats_t *stats);

/* The marker kernel's list for a host buffer (parity/debug): *out (atz_free) receives the *n positions q with
 * q + 4 <= len and bytes q..q+3 = 00 00 FF FF, ascending. */
int atz_flush_markers(atz_ctx_t *ctx, const uint8_t *file, uint64_t len, uint64_t **out, uint64_t *n);

/* atz_inflate_batch on raw deflate bodies (no zlib header, no trailer) with the segment decoder (parity/debug):
 * a job also ends, with status 0, at the first stored block with BFINAL = 0 and LEN = 0 -- consumed[i] is then
 * the byte after NLEN and at_marker[i] = 1; at a final block at_marker[i] = 0. */
int atz_inflate_segments(atz_ctx_t *ctx, const uint8_t *buf, uint64_t len, const uint64_t *offs,
                         const uint64_t *lens, uint64_t n, uint32_t *status, uint64_t *consumed,
                         uint64_t *produced, uint8_t *at_marker);

/* Batch of independent one-shot inflates of the given ranges of a host buffer (parity/debug):
 * status[i] in {0 end, 1 error, 2 need input}, consumed[i] = zlib total_in, produced[i] = total_out. */
int atz_inflate_batch(atz_ctx_t *ctx, const uint8_t *buf, uint64_t len, const uint64_t *offs,
                      const uint64_t *lens, uint64_t n, uint32_t *status, uint64_t *consumed, uint64_t *produced);

/* ---- Multi-GPU precompress of ONE file -----------------------------------------
 * One process, context and GPU per rank; every rank holds the whole file in HBM (d_file, >= 4096
 * bytes of slack) and a host copy.  Replaces the same Phase 1 + 3 + 4 as atz_precompress, split
 * where the ranks exchange data (the caller does the exchanges, e.g. torch.distributed over RCCL):
 *   1. atz_shard_scan: inflates the scan candidates of this rank's chunk range -> *blob (atz_free).
 *      Exchange: all-gather every rank's blob.
 *   2. atz_shard_sweep: replays the whole file's greedy scan (main.cpp:205-246) from all blobs, then
 *      sweeps (main.cpp:421-763) and writes the ATZ1 descriptors + payloads (writeStreamdesc,
 *      main.cpp:805-831) of the records its chunk range produced: *piece_len bytes, kept in the
 *      context.  *recomp_flags (atz_free) = one byte per such record.
 *      Exchange: all-gather piece lengths, recomp counts and flags; gather the pieces to rank 0.
 *   3. atz_shard_piece: device copy of this rank's piece to d_dst (rank 0: d_atz + 28 + the pieces
 *      of the ranks before it).
 *   4. rank 0, atz_shard_assemble: header + residue (writeATZfile, main.cpp:764-801) around the
 *      pieces in d_atz (capacity cap); flags = every rank's, in rank order.
 * The ATZ1 bytes are identical to atz_precompress of the same file on one GPU. */
int atz_shard_scan(atz_ctx_t *ctx, const uint8_t *d_file, const uint8_t *h_file, uint64_t len, int rank, int world,
                   uint8_t **blob, uint64_t *blob_len);
int atz_shard_sweep(atz_ctx_t *ctx, const uint8_t *d_file, const uint8_t *h_file, uint64_t len,
                    const uint8_t *const *blobs, const uint64_t *blob_lens, int world, uint64_t *piece_len,
                    uint8_t **recomp_flags, uint64_t *n_flags, uint64_t *n_recomp, atz_stats_t *stats);
int atz_shard_piece(atz_ctx_t *ctx, uint8_t *d_dst);
int atz_shard_assemble(atz_ctx_t *ctx, const uint8_t *d_file, uint64_t len, const uint8_t *recomp_flags,
                       uint64_t n_flags, uint64_t n_recomp, uint64_t pieces_len, uint8_t *d_atz, uint64_t cap,
                       uint64_t *atz_len);

/* zlib-1.2.8 deflate bound for the parameters (deflateBound, Z/deflate.c:566-621). */
uint64_t atz_deflate_bound(uint64_t n, int window, int memlevel);

#ifdef __cplusplus
}
#endif
#endif
