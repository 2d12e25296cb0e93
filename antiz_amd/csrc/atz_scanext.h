// atz_scanext.h -- the rules of the scan's four opt-in extensions: containers, stitching (s7.3),
// probe (s7.4) and flush segments (s7.6).  Host only, plain C++17, no HIP header; tests/scanext_check.cpp runs every
// function on the CPU under ASan/UBSan against the tests' Python models.
// Each extension is a job step and an accept step with no device call between them: the job step turns a list kernel's
// positions (and the host copy of the file) into k_inflate jobs, atz_accel.cpp launches them, and the accept step turns
// their results into records.  The records made before are complete, in file order and disjoint, and never change but
// where a step says so.
// The contract with the kernels.  The steps read the file's bytes at places the lists name, so what
// the list kernels and k_inflate promise is checked here before it is relied on, one comparison per list entry; on
// a violation a step returns ATZ_E_INTERNAL and makes no read through the entry:
//   k_anchors_ordered, k_probe_ordered, k_marker_ordered: positions ascending;
//   anchor_kind: a ZIP anchor p has p + 30 <= n, a gzip anchor p + 18 <= n; an IDAT anchor p >= 4, its big-endian
//     length L at p - 4 is below 2^31, and p + 8 + L <= n;
//   k_probe_ordered: a position p < F;  k_marker_ordered: a marker q with q + 4 <= F;
//   k_inflate: one result per job, and a decode that ended (INF_END) consumed no more than the job offered.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "atz_device.h"
#include "atz_format.h"

namespace atz {

static constexpr uint64_t ARENA_SLOT = 65536;   // arena slot per scan candidate (longer outputs are re-inflated)

struct Rec {
  uint64_t offset, comp_len, infl_len;
  int type;
  uint32_t flags;
  uint64_t arena_off = ~0ull;   // scan output kept in the arena (complete), else ~0
  bool noshort = false;         // k_inflate's INF_HINT_NOSHORT (the multi-GPU split's cost estimate)
  uint8_t mhint = 0;            // k_inflate's first-block memLevel (0: none; whole match tables for it)
  // a stitched record (the stitch extension): its comp_len stream bytes lie contiguous at
  // this offset of the context's stitch buffer and in the file as pieces [p0, p0 + pk) of st_off / st_len,
  // 12 framing bytes between two pieces; offset is the first piece's.  ~0: an ordinary record
  uint64_t stitch = ~0ull;
  uint32_t p0 = 0, pk = 0;
  // the file range the record occupies: a stitched one's hull includes the framing between its pieces
  uint64_t hull() const { return comp_len + (stitch != ~0ull ? 12ull * (pk - 1) : 0); }
};

inline int header_type_host(unsigned b0, unsigned b1) {
  static const uint16_t H[24] = {0x2815, 0x2853, 0x2891, 0x28cf, 0x3811, 0x384f, 0x388d, 0x38cb,
                                 0x480d, 0x484b, 0x4889, 0x48c7, 0x5809, 0x5847, 0x5885, 0x58c3,
                                 0x6805, 0x6843, 0x6881, 0x68de, 0x7801, 0x785e, 0x789c, 0x78da};
  unsigned h = (b0 << 8) | b1;
  for (int t = 0; t < 24; t++) if (H[t] == h) return t;
  return -1;
}

// (rd4le: atz_format.h)
inline uint32_t rd2le(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t rd4be(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// the last four bytes of record r's stream (its Adler-32 trailer, big-endian) from the host copy h: a
// stitched record's may straddle its pieces (st_off / st_len: the piece lists r.p0 points into)
inline uint32_t rec_trailer(const Rec& r, const uint8_t* h, const std::vector<uint64_t>& st_off,
                            const std::vector<uint64_t>& st_len) {
  if (r.stitch == ~0ull) return rd4be(h + r.offset + r.comp_len - 4);
  uint32_t t = 0;
  int got = 0;
  for (uint32_t q = r.p0 + r.pk; q > r.p0 && got < 4; q--)
    for (uint64_t b = st_len[q - 1]; b > 0 && got < 4; b--, got++) t |= (uint32_t)h[st_off[q - 1] + b - 1] << (8 * got);
  return t;
}

// ---------------------------------------------------------------------------------------------
// Shared steps
// A record of ref (in file order, disjoint) meets the file range [lo, hi): only the last one that starts below
// hi can.
inline bool meets_earlier(const std::vector<Rec>& ref, uint64_t lo, uint64_t hi) {
  const auto it = std::lower_bound(ref.begin(), ref.end(), hi, [](const Rec& x, uint64_t v) { return x.offset < v; });
  return it != ref.begin() && (it - 1)->offset + (it - 1)->hull() > lo;
}
// `merged` becomes the records; recs keeps its capacity (the sweep's tables are sized for it)
inline int put_records(std::vector<Rec>& recs, const std::vector<Rec>& merged) {
  if (merged.size() > recs.capacity()) return ATZ_E_INTERNAL;
  recs.assign(merged.begin(), merged.end());
  return 0;
}
// The new records (ascending offsets, disjoint, meeting no record of recs) take their places in recs.
inline int splice(std::vector<Rec>& recs, const std::vector<Rec>& add) {
  if (add.empty()) return 0;
  std::vector<Rec> merged;
  merged.reserve(recs.size() + add.size());
  size_t i = 0;
  for (const Rec& e : add) {
    while (i < recs.size() && recs[i].offset < e.offset) merged.push_back(recs[i++]);
    merged.push_back(e);
  }
  while (i < recs.size()) merged.push_back(recs[i++]);
  return put_records(recs, merged);
}
// k_inflate's promise for a job that offered `offered` bytes
inline bool res_sound(const InfRes& r, uint64_t offered) { return r.status != INF_END || r.consumed <= offered; }
// the decode ended with min_out <= produced < 2^31
inline bool ended_with(const InfRes& r, uint64_t min_out) {
  return r.status == INF_END && r.produced >= min_out && r.produced < (1ull << 31);
}
// The greedy pick over acc (ascending offsets, ordinary records): one that starts inside the one kept before it
// is dropped.
inline void pick_disjoint(const std::vector<Rec>& acc, std::vector<Rec>& kept) {
  kept.clear();
  uint64_t end = 0;
  for (const Rec& e : acc) {
    if (e.offset < end) continue;
    end = e.offset + e.comp_len;
    kept.push_back(e);
  }
}
// a list kernel's positions: strictly ascending, each with `room` bytes from it inside [0, n)
inline bool positions_ok(const std::vector<uint64_t>& pos, uint64_t room, uint64_t n) {
  for (size_t k = 0; k < pos.size(); k++)
    if ((k && pos[k] <= pos[k - 1]) || !inside(pos[k], room, n)) return false;
  return true;
}

// ---------------------------------------------------------------------------------------------
// Containers (atz_set_containers).  ZIP entries and gzip members hold raw deflate bodies, which
// no zlib header announces.  k_anchors_ordered lists the fixed headers of both containers in file order (position
// << 5 | kind); raw_candidates parses their variable parts; one raw k_inflate launch decodes the bodies; what the
// container's own size fields confirm becomes a record of type 24 + hint.
struct RawCand {
  uint64_t p, d, limit;   // anchor, first body byte, bytes offered to the decoder
  int kind, hint;         // 0 ZIP / 1 gzip; 0 none, 1 fast, 2 max
  bool know_c, know_u;    // ZIP: the header states the compressed / the uncompressed size
  uint64_t csize, usize;
};

// The variable part of each anchor's header, from the host copy h[0, n): where the body starts, how many bytes
// the decoder may read, the level hint the container carries.  An anchor whose header runs past the end
// of the file, or that leaves no byte for a body, is dropped.  (Reads: a ZIP header's 30 fixed bytes and a gzip
// header's first 10, which anchor_kind promises; every byte behind them after its own length test.)
inline int raw_candidates(const uint8_t* h, uint64_t n, const std::vector<uint64_t>& anchors, std::vector<RawCand>& out) {
  out.clear();
  uint64_t below = 0;   // the next anchor's position is at least this
  for (const uint64_t a : anchors) {
    RawCand r{};
    r.p = a >> 5; r.kind = (int)(a & 31);
    if (r.p < below) return ATZ_E_INTERNAL;
    below = r.p + 1;
    if (r.kind > 1) continue;   // an IDAT anchor of the same pass (the stitch extension)
    if (!inside(r.p, r.kind == 0 ? 30 : 18, n)) return ATZ_E_INTERNAL;
    const uint8_t* q = h + r.p;
    if (r.kind == 0) {
      const uint32_t flag = rd2le(q + 6);
      r.csize = rd4le(q + 18); r.usize = rd4le(q + 22);
      r.d = r.p + 30 + rd2le(q + 26) + rd2le(q + 28);
      if (r.d >= n) continue;
      const bool dd = flag & 8;   // sizes follow the body in a data descriptor
      r.know_c = !dd && r.csize != 0 && r.csize != 0xffffffffu;
      r.know_u = !dd && r.usize != 0xffffffffu;
      if (r.know_c && r.csize > n - r.d) continue;
      r.limit = r.know_c ? r.csize : n - r.d;
      const uint32_t lv = (flag >> 1) & 3;   // general purpose bits 2-1: 01 maximum, 10 fast, 11 super fast
      r.hint = lv == 1 ? 2 : lv >= 2 ? 1 : 0;
    } else {
      const uint32_t flg = q[3], xfl = q[8];
      uint64_t at = r.p + 10;
      bool ok = true;
      if (flg & 4) {   // FEXTRA
        if (at + 2 > n) continue;
        at += 2 + rd2le(h + at);
        ok = at <= n;
      }
      for (uint32_t bit = 8; ok && bit <= 16; bit <<= 1)   // FNAME, FCOMMENT: zero-terminated
        if (flg & bit) {
          while (at < n && h[at]) at++;
          ok = at < n;
          at++;
        }
      if (ok && (flg & 2)) { at += 2; ok = at <= n; }   // FHCRC
      if (!ok || at + 8 >= n) continue;   // (the trailer's 8 bytes follow the body)
      r.d = at;
      r.limit = n - at - 8;
      r.hint = xfl == 2 ? 2 : xfl == 4 ? 1 : 0;
    }
    out.push_back(r);
  }
  return 0;
}

// outputs in the scan's arena, behind the candidates' decoded before
inline void raw_jobs(const std::vector<RawCand>& cands, std::vector<InfJob>& jobs) {
  jobs.resize(cands.size());
  for (size_t k = 0; k < cands.size(); k++) jobs[k] = {cands[k].d, cands[k].limit, ARENA_OUT, ARENA_SLOT};
}

// kept: the candidates accepted by the container's own fields, dropped where they meet a record of recs, taken
// greedily in ascending offset (two with one body: the lower anchor's).  (A gzip member's ISIZE lies inside the
// file: its candidate's limit leaves the trailer's 8 bytes, and the decode consumed no more than the limit.)
inline int raw_accept(const uint8_t* h, const std::vector<RawCand>& cands, const std::vector<InfRes>& res,
                      const std::vector<Rec>& recs, std::vector<Rec>& kept) {
  if (res.size() != cands.size()) return ATZ_E_INTERNAL;
  std::vector<Rec> acc;
  for (size_t k = 0; k < cands.size(); k++) {
    const RawCand& a = cands[k];
    const InfRes& r = res[k];
    if (!res_sound(r, a.limit)) return ATZ_E_INTERNAL;
    if (!ended_with(r, 1)) continue;
    if (a.kind == 0) {
      if (a.know_c && r.consumed != a.csize) continue;
      if (a.know_u && r.produced != a.usize) continue;
    } else if (rd4le(h + a.d + r.consumed + 4) != (uint32_t)r.produced) {   // ISIZE
      continue;
    }
    if (meets_earlier(recs, a.d, a.d + r.consumed)) continue;
    acc.push_back(Rec{a.d, r.consumed, r.produced, 24 + a.hint, 0, r.arena_off});
  }
  // (the candidates are in anchor order: equal offsets stay so)
  std::stable_sort(acc.begin(), acc.end(), [](const Rec& x, const Rec& y) { return x.offset < y.offset; });
  pick_disjoint(acc, kept);
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Stitching (atz_set_stitch).  A PNG writer cuts one zlib stream into IDAT chunks: every few KiB of
// it are followed by 12 framing bytes (the chunk's CRC, the next chunk's length, "IDAT"), at which the scan's decode
// fails.  k_anchors_ordered (kind 2) lists the IDAT type fields in file order; stitch_candidates links consecutive
// chunks into chains; k_gather copies each chain's payloads into one contiguous run of the stitch buffer; one
// k_inflate launch decodes the runs; a stream that ends, crosses a chunk boundary and meets no record made before
// becomes a record whose original bytes are the stitched copy.
struct StitchCand {
  uint64_t at, total;   // the chain's run in the stitch buffer (256-byte aligned), its payload bytes
  uint32_t p0, pk;      // its pieces in StitchPlan::off / len (the first and the last are not empty)
  int type;             // header type 0..23 of the run's first two bytes
};
struct StitchPlan {
  std::vector<StitchCand> cands;
  std::vector<uint64_t> off, len;   // file offset and length of every candidate's payloads
  uint64_t bytes = 0;               // the stitch buffer's size (without its slack)
};

// Chains and candidates from the kernel's anchors (position << 5 | 2 among them, ascending) and the host copy
// h[0, n).  A cursor walks the file: an anchor below it belongs to no chain; from an anchor a at or past it the
// chain follows a' = a + L + 12 while a' is an anchor, and the cursor moves to the end of the last chunk's
// CRC.  So chains are disjoint and inside the file: the payload bytes gathered never exceed n.  A chain without its
// leading empty chunks is a candidate if two chunks or more remain and its payloads start with one of the 24 zlib
// headers (the two bytes may lie in two chunks).
inline int stitch_candidates(const uint8_t* h, uint64_t n, const std::vector<uint64_t>& anchors, StitchPlan& P) {
  P = StitchPlan{};
  std::vector<uint64_t> A, AL;   // the IDAT anchors and their chunks' lengths
  uint64_t below = 0;
  for (const uint64_t a : anchors) {
    const uint64_t p = a >> 5;
    if (p < below) return ATZ_E_INTERNAL;
    below = p + 1;
    if ((a & 31) != 2) continue;
    if (p < 4 || !inside(p, 8, n)) return ATZ_E_INTERNAL;
    const uint64_t L = rd4be(h + p - 4);
    if (L >= (1ull << 31) || L > n - p - 8) return ATZ_E_INTERNAL;
    A.push_back(p); AL.push_back(L);
  }
  uint64_t cursor = 0;
  std::vector<std::pair<uint64_t, uint64_t>> ch;   // (payload offset, length)
  for (size_t i = 0; i < A.size(); i++) {
    if (A[i] < cursor) continue;
    ch.clear();
    size_t j = i;
    for (;;) {
      const uint64_t a = A[j], L = AL[j];
      ch.push_back({a + 4, L});
      cursor = a + 8 + L;
      j = (size_t)(std::lower_bound(A.begin() + j + 1, A.end(), a + L + 12) - A.begin());
      if (j == A.size() || A[j] != a + L + 12) break;
    }
    size_t q = 0;
    while (q < ch.size() && ch[q].second == 0) q++;
    if (ch.size() - q < 2) continue;
    unsigned hb[2] = {0, 0};
    uint64_t total = 0;
    for (size_t k = q; k < ch.size(); k++) {
      for (uint64_t b = 0; b < ch[k].second && total + b < 2; b++) hb[total + b] = h[ch[k].first + b];
      total += ch[k].second;
    }
    const int type = total >= 2 ? header_type_host(hb[0], hb[1]) : -1;
    if (type < 0) continue;
    StitchCand cd{P.bytes, total, (uint32_t)P.off.size(), (uint32_t)(ch.size() - q), type};
    for (size_t k = q; k < ch.size(); k++) { P.off.push_back(ch[k].first); P.len.push_back(ch[k].second); }
    P.cands.push_back(cd);
    P.bytes += (total + 255) & ~255ull;
  }
  return 0;
}

// k_gather's segments (file -> the stitch buffer) and one job per run (input base: the stitch buffer).  With each
// run rounded up to 256 bytes the buffer is at most n + 256 * candidates bytes.
inline void stitch_jobs(const StitchPlan& P, std::vector<Seg>& segs, std::vector<InfJob>& jobs) {
  segs.clear();
  jobs.resize(P.cands.size());
  for (size_t k = 0; k < P.cands.size(); k++) {
    const StitchCand& a = P.cands[k];
    uint64_t at = a.at;
    for (uint32_t q = a.p0; q < a.p0 + a.pk; q++) {
      if (P.len[q]) segs.push_back({SEG_FILE, 0, P.off[q], at, P.len[q]});
      at += P.len[q];
    }
    jobs[k] = {a.at, a.total, ARENA_OUT, ARENA_SLOT};
  }
}

// kept: the candidates (in file order and disjoint, as their chains are) whose stream ended behind its first chunk
// and whose hull meets no record of recs; their pieces are appended to st_off / st_len.  Only these records take
// noshort and mhint from InfRes.err: the stitched copy is all the sweep has of them.
inline int stitch_accept(const StitchPlan& P, const std::vector<InfRes>& res, const std::vector<Rec>& recs,
                         std::vector<uint64_t>& st_off, std::vector<uint64_t>& st_len, std::vector<Rec>& kept) {
  kept.clear();
  if (res.size() != P.cands.size()) return ATZ_E_INTERNAL;
  for (size_t k = 0; k < P.cands.size(); k++) {
    const StitchCand& a = P.cands[k];
    const InfRes& r = res[k];
    if (!res_sound(r, a.total)) return ATZ_E_INTERNAL;   // (so the pieces below hold the whole stream)
    if (!ended_with(r, 1)) continue;
    if (r.consumed <= P.len[a.p0]) continue;   // ends inside the first chunk: the reference scan's business
    Rec rec{P.off[a.p0], r.consumed, r.produced, a.type, 0, r.arena_off};
    rec.noshort = (r.err & INF_HINT_NOSHORT) != 0;
    rec.mhint = (uint8_t)((r.err >> INF_HINT_MLEV_SHIFT) & 15u);
    rec.stitch = a.at;
    rec.p0 = (uint32_t)st_off.size();
    // the pieces the stream touches: the last one ends where the stream does
    uint64_t sum = 0;
    for (uint32_t q = a.p0; q < a.p0 + a.pk && sum < r.consumed; q++) {
      const uint64_t take = std::min<uint64_t>(P.len[q], r.consumed - sum);
      st_off.push_back(P.off[q]); st_len.push_back(take);
      sum += take;
      rec.pk++;
    }
    if (meets_earlier(recs, rec.offset, rec.offset + rec.hull())) {
      st_off.resize(rec.p0); st_len.resize(rec.p0);
      continue;
    }
    kept.push_back(rec);
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Probe (atz_set_probe).  A raw deflate stream that no zlib header and no container announces:
// k_probe_ordered tests every byte position of the file for a plausible dynamic-block start, one raw k_inflate launch
// decodes the survivors that lie in no record made before, and one that decodes to its end with PROBE_MIN_OUT bytes
// or more and meets no such record becomes a record of type 24 (raw, no hint).
static constexpr uint64_t PROBE_MIN_OUT = 256;   // a dynamic header alone is 40-80 bytes: smaller bodies gain nothing

// Survivors inside a record's hull are not decoded (every byte-aligned block start of a known stream would be
// one); the rest are decoded to the end of the file.
inline int probe_jobs(const std::vector<uint64_t>& pos, uint64_t F, const std::vector<Rec>& recs, std::vector<InfJob>& jobs) {
  jobs.clear();
  if (!positions_ok(pos, 1, F)) return ATZ_E_INTERNAL;
  size_t i = 0;
  for (const uint64_t p : pos) {
    while (i < recs.size() && recs[i].offset + recs[i].hull() <= p) i++;
    if (i < recs.size() && recs[i].offset <= p) continue;
    jobs.push_back({p, F - p, ARENA_OUT, ARENA_SLOT});
  }
  return 0;
}

// accepted: by status and output size; kept: those of them that meet no record of recs, greedily in ascending offset
inline int probe_accept(const std::vector<InfJob>& jobs, const std::vector<InfRes>& res, const std::vector<Rec>& recs,
                        std::vector<Rec>& kept, size_t& accepted) {
  accepted = 0;
  if (res.size() != jobs.size()) return ATZ_E_INTERNAL;
  std::vector<Rec> acc;
  for (size_t k = 0; k < jobs.size(); k++) {
    const InfRes& r = res[k];
    if (!res_sound(r, jobs[k].in_len)) return ATZ_E_INTERNAL;
    if (!ended_with(r, PROBE_MIN_OUT)) continue;
    accepted++;
    const uint64_t lo = jobs[k].in_off;
    if (meets_earlier(recs, lo, lo + r.consumed)) continue;
    acc.push_back(Rec{lo, r.consumed, r.produced, 24 /* raw, hint none */, 0, r.arena_off});
  }
  pick_disjoint(acc, kept);
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Segments (atz_set_segments).  deflate(Z_FULL_FLUSH) ends a segment with an empty stored block
// (its byte-aligned tail is 00 00 FF FF) and starts the next one from a fresh state, so a stream cut by full flushes
// is a chain of independent raw bodies, each exactly what a one-shot deflate of its bytes writes, but for its end.
// k_marker_ordered lists the markers of the file; every segment start of the eligible records is decoded in one
// launch of k_inflate's SEG variant; a record whose chain completes is replaced by its segments.
struct SegElig { size_t rec; uint64_t b0, b1; size_t j0, j1; };   // record, its body [b0, b1), its jobs [j0, j1)

// Eligible: a raw record (type 24-26; its body is the record), or a zlib record whose header says window 15 and
// that is not stitched (its body lies between the 2 header bytes and the 4 trailer bytes), with a marker q,
// body_start <= q and q + 4 < body_end.  Jobs: body_start and every such q + 4, each offered the bytes up to
// body_end, without output (the record's whole decode lies in the arena, or is inflated again).  (A record that
// reaches past the file's F bytes, which the reference's scan can make and the sweep refuses, is not eligible.)
inline int seg_jobs(const uint8_t* h, uint64_t F, const std::vector<Rec>& recs, const std::vector<uint64_t>& markers,
                    std::vector<SegElig>& el, std::vector<InfJob>& jobs) {
  el.clear(); jobs.clear();
  if (!positions_ok(markers, 4, F)) return ATZ_E_INTERNAL;
  for (size_t i = 0; i < recs.size() && !markers.empty(); i++) {
    const Rec& r = recs[i];
    if (!inside(r.offset, r.comp_len, F)) continue;
    uint64_t b0 = r.offset, b1 = r.offset + r.comp_len;
    if (r.type < 24) {
      if (r.stitch != ~0ull || r.comp_len < 7 || (h[r.offset] >> 4) != 7) continue;
      b0 += 2; b1 -= 4;
    } else if (r.type > 26) continue;
    auto it = std::lower_bound(markers.begin(), markers.end(), b0);
    if (it == markers.end() || *it + 4 >= b1) continue;
    SegElig e{i, b0, b1, jobs.size(), 0};
    jobs.push_back({b0, b1 - b0, NO_OUT, 0});
    for (; it != markers.end() && *it + 4 < b1; ++it) jobs.push_back({*it + 4, b1 - (*it + 4), NO_OUT, 0});
    e.j1 = jobs.size();
    el.push_back(e);
  }
  return 0;
}

// The chain s_0 = body_start, s_{i+1} = s_i + consumed_i over jobs that ended at a marker with output completes when
// it reaches a job that ended at a final block exactly at body_end, after at least one marker, with the outputs
// summing to the record's; then the record is replaced, in place, by Rec{s_i, consumed_i, produced_i, 24 + hint}
// (a raw parent's hint; a zlib parent's FLEVEL 0, 1 -> fast, 2 -> none, 3 -> max), flags bit 7 on all but the last,
// and a last segment without output makes no record.  All or nothing.  merged: the records after every replacement
// (chains of them, `made` segments in all); the caller puts them in place when chains != 0.
inline int seg_accept(const uint8_t* h, const std::vector<Rec>& recs, const std::vector<SegElig>& el,
                      const std::vector<InfJob>& jobs, const std::vector<InfRes>& res, std::vector<Rec>& merged,
                      size_t& chains, size_t& made) {
  merged.clear();
  chains = made = 0;
  if (res.size() != jobs.size()) return ATZ_E_INTERNAL;
  for (size_t k = 0; k < jobs.size(); k++)
    if (!res_sound(res[k], jobs[k].in_len)) return ATZ_E_INTERNAL;
  merged.reserve(recs.size() + jobs.size());
  size_t i = 0;
  for (const SegElig& e : el) {
    const Rec& par = recs[e.rec];
    std::vector<Rec> segs;
    const int type = par.type >= 24 ? par.type : (h[par.offset + 1] >> 6) == 2 ? 24 : (h[par.offset + 1] >> 6) == 3 ? 26 : 25;
    uint64_t s = e.b0, sum = 0;
    size_t k = 0;
    bool ok = false;
    for (size_t j = e.j0; j < e.j1;) {
      const InfRes& r = res[j];
      if (r.status != INF_END) break;
      const uint64_t ao = par.arena_off != ~0ull ? par.arena_off + sum : ~0ull;
      k++;
      if (r.err & INF_AT_MARKER) {
        if (r.produced < 1) break;
        segs.push_back(Rec{s, r.consumed, r.produced, type, 128u, ao});
        s += r.consumed; sum += r.produced;
        // the job that starts at s (none: the marker's end is body_end, so no final block follows)
        j = (size_t)(std::lower_bound(jobs.begin() + j + 1, jobs.begin() + e.j1, s,
                                      [](const InfJob& x, uint64_t v) { return x.in_off < v; }) - jobs.begin());
        if (j < e.j1 && jobs[j].in_off != s) break;
        continue;
      }
      if (s + r.consumed != e.b1) break;
      if (r.produced) segs.push_back(Rec{s, r.consumed, r.produced, type, 0u, ao});
      sum += r.produced;
      ok = k >= 2 && sum == par.infl_len;
      break;
    }
    if (!ok) continue;
    while (i < e.rec) merged.push_back(recs[i++]);
    i++;   // the parent leaves
    merged.insert(merged.end(), segs.begin(), segs.end());
    chains++; made += segs.size();
  }
  while (i < recs.size()) merged.push_back(recs[i++]);
  return 0;
}

}  // namespace atz
