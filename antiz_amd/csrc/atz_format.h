// atz_format.h -- the ATZ container: its reader, the reconstruct plan and its writer (host only, plain C++17, no
// HIP header; tests/format_check.cpp executes the plans on the CPU under ASan/UBSan).
// The file (the reference's writer main.cpp:764-834, its reader main.cpp:1011-1063):
//   "ATZ" version | u64 length | u64 origlen | u64 nstreams | descriptors | residue
//   descriptor: u64 offset, comp_len, infl_len | clevel, window, memLevel | u64 ndiff
//               [ u64 first_diff | ndiff x u64 delta | ndiff x u8 value ] | infl_len payload bytes
//               [ u32 k | k x u32 piece length ]      (a stitched descriptor: bit 7 of clevel, version >= 4)
// A nested file wraps two of them:
//   "ATN" 1 | u64 length | u64 outer_len | outer (outer_len bytes) | inner (to the end)
// outer: an ATZ file without its descriptors' payload bytes ("stripped"); inner: the ATZ or ATN file of P, the outer's
// payloads concatenated in descriptor order.
// Both plans are lists of k_gather segments (Seg) plus, for reconstruct, k_patch's (address, value) pairs.  The
// kernels execute them with raw device addresses, so every bound they rely on is checked here: a plan function
// that would emit a range outside its buffer returns ATZ_E_INTERNAL instead (one comparison per stream or segment).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/atz_accel.h"
#include "atz_params.h"

namespace atz {

enum : uint32_t { SEG_META = 0, SEG_ADDR = 1, SEG_FILE = 2, SEG_ZERO = 3 };
struct Seg {           // k_gather segment: len bytes from src_off of the source to dst_off of the destination
  uint32_t src;        // SEG_META: the metadata buffer, SEG_ADDR: an absolute address, SEG_FILE: the file, SEG_ZERO
  uint32_t pad;
  uint64_t src_off, dst_off, len;
};

inline uint64_t rd8(const uint8_t* p) { uint64_t v; std::memcpy(&v, p, 8); return v; }
inline uint32_t rd4le(const uint8_t* p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
inline void put8(std::vector<uint8_t>& m, uint64_t v) { uint8_t b[8]; std::memcpy(b, &v, 8); m.insert(m.end(), b, b + 8); }
inline void put4(std::vector<uint8_t>& m, uint32_t v) { uint8_t b[4]; std::memcpy(b, &v, 4); m.insert(m.end(), b, b + 4); }
// [off, off + len) lies inside [0, cap) (subtraction only: no sum can wrap)
inline bool inside(uint64_t off, uint64_t len, uint64_t cap) { return off <= cap && len <= cap - off; }

// ---------------------------------------------------------------------------------------------
// Reader
// (dpos: the deltas, their values behind them; ipos: the payload; k, ppos: a stitched descriptor's piece count and
// the position of its k u32 piece lengths; k = 0: not stitched)
// (in a stripped file ipos is the payload's offset in P)
struct AtzDesc {
  uint64_t off, cl, il, nd, fd, dpos, ipos; uint8_t c, w, m;
  uint64_t k = 0, ppos = 0;
  uint64_t hull() const { return cl + (k ? 12 * (k - 1) : 0); }
};
// stream range [a, b) of a stitched descriptor, cut at its pieces: fn(stream position, file position, length)
template <class F>
inline void stitched_ranges(const uint8_t* atz, const AtzDesc& x, uint64_t a, uint64_t b, F fn) {
  uint64_t sp = 0, fp = x.off;   // the piece's first byte in the stream and in the file
  for (uint64_t i = 0; i < x.k && sp < b; i++) {
    const uint64_t len = rd4le(atz + x.ppos + 4 * i);
    const uint64_t lo = std::max(a, sp), hi = std::min(b, sp + len);
    if (lo < hi) fn(lo, fp + (lo - sp), hi - lo);
    sp += len; fp += len + 12;
  }
}

// ATZ parse with the reference's checks (main.cpp:1011-1063); every size field is bounded by the
// bytes actually left before anything is sized from it (subtraction-only checks: no sum can wrap).
// stripped: the outer file of a nested one -- no payload bytes follow a descriptor's fixed fields and diff list, and
// payload j is bytes [sum of the infl_len before it, + infl_len) of P, whose plen bytes bound them.
inline int parse_atz(const uint8_t* atz, uint64_t n, std::vector<AtzDesc>& d, uint64_t& origlen, uint64_t& residue,
                     bool stripped = false, uint64_t plen = 0) {
  // (the versions and what their descriptors may carry: atz_params.h)
  if (n < 28 || std::memcmp(atz, "ATZ", 3) != 0 || atz[3] < 1 || atz[3] > DeflSpec::MAX_VERSION) return ATZ_E_FORMAT;   // main.cpp:1018-1021
  const int version = atz[3];
  if (rd8(atz + 4) != n) return ATZ_E_FORMAT;                              // main.cpp:1022-1025
  origlen = rd8(atz + 12);
  const uint64_t nstrms = rd8(atz + 20);
  d.clear();
  if (nstrms == 0) {
    if (origlen > n - 28) return ATZ_E_FORMAT;
    residue = 28;
    return 0;
  }
  if (nstrms > (n - 28) / 35) return ATZ_E_FORMAT;                       // each descriptor is >= 35 bytes
  d.resize(nstrms);
  uint64_t lastos = 28;                                                    // main.cpp:1031-1063
  uint64_t pat = 0;                                                        // stripped: the next payload's place in P
  for (uint64_t j = 0; j < nstrms; j++) {
    if (n - lastos < 35) return ATZ_E_FORMAT;
    AtzDesc& x = d[j];
    x.off = rd8(atz + lastos); x.cl = rd8(atz + lastos + 8); x.il = rd8(atz + lastos + 16);
    x.c = atz[lastos + 24]; x.w = atz[lastos + 25]; x.m = atz[lastos + 26];
    x.nd = rd8(atz + lastos + 27);
    if (x.nd) {
      if (n - lastos < 43) return ATZ_E_FORMAT;
      const uint64_t room = n - lastos - 43;
      if (x.nd > room / 9) return ATZ_E_FORMAT;
      if (!stripped && x.il > room - x.nd * 9) return ATZ_E_FORMAT;
      x.fd = rd8(atz + lastos + 35); x.dpos = lastos + 43; x.ipos = lastos + 43 + x.nd * 9;
    } else {
      if (!stripped && x.il > n - lastos - 35) return ATZ_E_FORMAT;
      x.fd = 0; x.dpos = 0; x.ipos = lastos + 35;
    }
    if (!stripped) {
      lastos = x.ipos + x.il;
    } else {
      if (x.il > plen - pat) return ATZ_E_FORMAT;   // (pat <= plen)
      lastos = x.ipos; x.ipos = pat;
      pat += x.il;
    }
    // a refusal of the parameters: the clevel byte's before the piece list is read, the other bytes' after it
    const bool ok = valid_desc(version, x.c, x.w, x.m);
    if (!ok && !valid_desc(version, x.c, 15, 8)) return ATZ_E_REF_ABORT;
    bool stitched = false;
    DeflSpec::from_desc(x.c, x.w, x.m, &stitched);
    if (stitched) {   // k >= 2 pieces, the first and the last not empty, their lengths summing to comp_len
      if (n - lastos < 4) return ATZ_E_FORMAT;
      x.k = rd4le(atz + lastos);
      if (x.k < 2 || x.k > (n - lastos - 4) / 4) return ATZ_E_FORMAT;
      x.ppos = lastos + 4;
      lastos = x.ppos + 4 * x.k;
      uint64_t sum = 0;
      for (uint64_t i = 0; i < x.k; i++) sum += rd4le(atz + x.ppos + 4 * i);
      if (sum != x.cl || rd4le(atz + x.ppos) < 1 || rd4le(atz + x.ppos + 4 * (x.k - 1)) < 1) return ATZ_E_FORMAT;
    }
    if (!ok) return ATZ_E_REF_ABORT;
  }
  // streams in file order, inside the original (the writer emits them so; a crafted file with
  // overlapping or out-of-range streams is rejected before any buffer is sized)
  uint64_t end = 0;
  for (uint64_t j = 0; j < nstrms; j++) {
    if (d[j].off < end || d[j].off > origlen || d[j].cl > origlen - d[j].off) return ATZ_E_FORMAT;
    if (d[j].k && (d[j].k - 1 > (origlen - d[j].off - d[j].cl) / 12)) return ATZ_E_FORMAT;   // the hull inside the original
    end = d[j].off + d[j].hull();
  }
  residue = lastos;
  // the residue must hold every gap and the tail
  uint64_t gaps = origlen;
  for (const AtzDesc& x : d) gaps -= x.cl;
  if (gaps > n - residue) return ATZ_E_FORMAT;
  return 0;
}

// A nested file's levels, outermost first: every one but the last is a stripped outer, the last a complete ATZ file;
// level k's payloads are level k + 1's original.  pos, len: the level's bytes in the file.
struct NestLevel {
  uint64_t pos = 0, len = 0;
  std::vector<AtzDesc> d;   // positions relative to pos (a stripped level's ipos: in P)
  uint64_t origlen = 0, residue = 0;
};
enum : uint64_t { NEST_HEADER = 20, NEST_MAX_DEPTH = 8 };
inline bool is_nest(const uint8_t* a, uint64_t n) { return n >= 4 && std::memcmp(a, "ATN", 3) == 0; }
// ATN parse: the wrappers first (every size by subtraction from the bytes left), then each level with parse_atz,
// innermost first, since a stripped level's payloads are bounded by the original of the level inside it.
inline int parse_nest(const uint8_t* a, uint64_t n, std::vector<NestLevel>& lv) {
  lv.clear();
  uint64_t at = 0, left = n;
  while (left >= 4 && std::memcmp(a + at, "ATN", 3) == 0) {
    if (lv.size() == NEST_MAX_DEPTH) return ATZ_E_FORMAT;
    if (left < NEST_HEADER + 28 + 28 || a[at + 3] != 1 || rd8(a + at + 4) != left) return ATZ_E_FORMAT;
    const uint64_t outer = rd8(a + at + 12);
    if (outer < 28 || outer > left - NEST_HEADER - 28) return ATZ_E_FORMAT;   // the inner file: a header at least
    NestLevel L;
    L.pos = at + NEST_HEADER; L.len = outer;
    lv.push_back(std::move(L));
    at += NEST_HEADER + outer; left -= NEST_HEADER + outer;
  }
  if (lv.empty()) return ATZ_E_FORMAT;
  NestLevel last;
  last.pos = at; last.len = left;
  lv.push_back(std::move(last));
  for (size_t k = lv.size(); k-- > 0;) {
    NestLevel& L = lv[k];
    const bool stripped = k + 1 < lv.size();
    if (int r = parse_atz(a + L.pos, L.len, L.d, L.origlen, L.residue, stripped, stripped ? lv[k + 1].origlen : 0)) return r;
    if (!stripped) continue;
    if (L.d.empty()) return ATZ_E_FORMAT;
    uint64_t sum = 0;   // (no wrap: every term was bounded by what P had left)
    for (const AtzDesc& x : L.d) sum += x.il;
    if (sum != lv[k + 1].origlen) return ATZ_E_FORMAT;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Reconstruct plan (ATZreconstructor::reconstructATZ, main.cpp:869-950), in two steps.
// Layout, once per file: the original is the residue's gaps and tail (plain copies from the ATZ bytes) around the
// streams; each stream is deflated again from its payload, which the trial kernels read 256-byte aligned from a slab.
struct RecLayout {
  std::vector<Seg> gaps;           // ATZ bytes -> the original: residue gaps and the tail
  std::vector<uint64_t> rec_off;   // stream j's first byte in the original
  std::vector<Seg> payloads;       // ATZ bytes -> the slab
  std::vector<uint64_t> loc;       // payload j's offset in the slab
  uint64_t slab = 0;               // the slab's size
  std::vector<DeflSpec> params;    // stream j's deflate, window 8 read as 9 (as zlib's deflateInit2 does)
};
// Where the payloads lie: in the file at each descriptor's ipos, or (a stripped file's) in P, plen bytes at absolute
// address pbase
struct PayloadSrc { bool stripped = false; uint64_t pbase = 0, plen = 0; };
enum : uint64_t { SEG_SPLIT = 1ull << 20 };   // k_gather gives one wave per segment: long copies are cut to this
inline void push_split(std::vector<Seg>& segs, Seg g) {
  while (g.len > SEG_SPLIT) {
    segs.push_back({g.src, 0, g.src_off, g.dst_off, SEG_SPLIT});
    g.src_off += SEG_SPLIT; g.dst_off += SEG_SPLIT; g.len -= SEG_SPLIT;
  }
  segs.push_back(g);
}
// atz[0, n) and (d, origlen, residue) as parse_atz accepted them
inline int plan_layout(const uint8_t* atz, uint64_t n, const std::vector<AtzDesc>& d, uint64_t origlen,
                       uint64_t residue, RecLayout& L, const PayloadSrc& P = PayloadSrc{}) {
  const size_t ns = d.size();
  L = RecLayout{};
  L.rec_off.resize(ns); L.loc.resize(ns); L.params.resize(ns);
  if (residue > n) return ATZ_E_INTERNAL;
  uint64_t gapsum = 0, lo = 0, ll = 0, out = 0;
  bool ok = true;
  // (a source range inside the residue [residue, n), a destination inside the original)
  auto gap = [&](uint64_t g) {
    ok = ok && inside(gapsum, g, n - residue) && inside(out, g, origlen);
    L.gaps.push_back({SEG_FILE, 0, residue + gapsum, out, g});
    gapsum += g; out += g;
  };
  // (a stitched stream's pieces each take their place: the 12 framing bytes between two are a gap)
  auto place = [&](uint64_t off, uint64_t len) {
    ok = ok && off >= lo + ll;   // offsets ascending
    if (lo + ll != off) gap(off - (lo + ll));
    ok = ok && inside(out, len, origlen);
    out += len;
    lo = off; ll = len;
  };
  for (size_t j = 0; j < ns && ok; j++) {
    if (!d[j].k) { place(d[j].off, d[j].cl); L.rec_off[j] = out - d[j].cl; continue; }
    L.rec_off[j] = d[j].off;   // (out == off at a stream's first byte: gaps and streams fill the original in order)
    uint64_t fp = d[j].off;
    for (uint64_t i = 0; i < d[j].k; i++) {
      const uint64_t len = rd4le(atz + d[j].ppos + 4 * i);
      place(fp, len);
      fp += len + 12;
    }
  }
  if (ok && lo + ll < origlen) gap(origlen - (lo + ll));
  if (!ok) return ATZ_E_INTERNAL;
  if (out != origlen) return ATZ_E_FORMAT;
  for (size_t j = 0; j < ns; j++) {
    if (!inside(d[j].ipos, d[j].il, P.stripped ? P.plen : n)) return ATZ_E_INTERNAL;
    L.loc[j] = L.slab; L.slab += (d[j].il + 255) & ~255ull;
    if (d[j].il && !P.stripped) L.payloads.push_back({SEG_FILE, 0, d[j].ipos, L.loc[j], d[j].il});
    if (d[j].il && P.stripped) push_split(L.payloads, {SEG_ADDR, 0, P.pbase + d[j].ipos, L.loc[j], d[j].il});
    L.params[j] = DeflSpec::from_desc(d[j].c, d[j].w, d[j].m);
    if (L.params[j].window == 8) L.params[j].window = 9;
  }
  return 0;
}

// Batch: streams [s0, s1) have been deflated, stream j's output is ol[j - s0] bytes at absolute address oa[j - s0],
// and the original is being rebuilt at absolute address rec_base.  Their first comp_len output bytes go to their
// places (zero-extended, as the reference's buffer is), then the diff bytes are patched (main.cpp:916-926).
struct RecBatch {
  std::vector<Seg> segs;       // outputs (SEG_ADDR) and zero extensions (SEG_ZERO) -> the original
  std::vector<uint64_t> pat;   // k_patch: absolute addresses, strictly ascending per stream, and
  std::vector<uint8_t> pval;   //          the byte each takes
};
inline int plan_batch(const uint8_t* atz, const std::vector<AtzDesc>& d, const RecLayout& L, uint64_t origlen,
                      size_t s0, size_t s1, const std::vector<uint64_t>& oa, const std::vector<uint64_t>& ol,
                      uint64_t rec_base, RecBatch& B) {
  B = RecBatch{};
  std::vector<Seg>& sg = B.segs;
  std::vector<uint64_t>& pat = B.pat;
  std::vector<uint8_t>& pval = B.pval;
  if (s1 > d.size() || s0 > s1 || oa.size() < s1 - s0 || ol.size() < s1 - s0) return ATZ_E_INTERNAL;
  for (size_t j = s0; j < s1; j++) {
    const uint64_t out_at = oa[j - s0], out_len = ol[j - s0], cl = d[j].cl, rec_off = L.rec_off[j];
    if (out_len > cl + 65535) return ATZ_E_REF_ABORT;   // deflate() != Z_STREAM_END in a cl+65535 buffer
    // every segment and patch of the stream lands in its hull, and the hull inside the original
    if (!inside(rec_off, d[j].hull(), origlen)) return ATZ_E_INTERNAL;
    const uint64_t k = out_len < cl ? out_len : cl;
    if (d[j].k) {
      // a stitched stream: its bytes go straight to their pieces' file positions -- the output ranges, the
      // zero extension and (below) each diff position are mapped through the piece prefix sums
      stitched_ranges(atz, d[j], 0, k, [&](uint64_t sp, uint64_t fp, uint64_t len) { sg.push_back({SEG_ADDR, 0, out_at + sp, fp, len}); });
      stitched_ranges(atz, d[j], k, cl, [&](uint64_t, uint64_t fp, uint64_t len) { sg.push_back({SEG_ZERO, 0, 0, fp, len}); });
    } else {
      if (k) sg.push_back({SEG_ADDR, 0, out_at, rec_off, k});
      if (cl > k) sg.push_back({SEG_ZERO, 0, 0, rec_off + k, cl - k});   // zero-extended buffer
    }
    // diff bytes: positions first_diff + prefix sums of the deltas; only those < cl reach the output
    if (!d[j].nd) continue;
    const size_t p0 = pat.size();
    std::vector<uint64_t> pre;   // a stitched stream's pieces: the stream position each starts at
    for (uint64_t i = 0, sp = 0; i < d[j].k; i++) { pre.push_back(sp); sp += rd4le(atz + d[j].ppos + 4 * i); }
    uint64_t sum = 0;
    bool increasing = true;
    for (uint64_t i = 0; i < d[j].nd; i++) {
      const uint64_t delta = rd8(atz + d[j].dpos + 8 * i);
      const uint64_t at = d[j].fd + delta + sum;
      sum += delta;
      if (at < cl) {
        uint64_t to = rec_off + at;
        if (d[j].k)   // behind i pieces' framing: i = the last piece that starts at or before `at`
          to += 12 * (uint64_t)(std::upper_bound(pre.begin(), pre.end(), at) - pre.begin() - 1);
        if (pat.size() > p0 && rec_base + to <= pat.back()) increasing = false;
        pat.push_back(rec_base + to);
        pval.push_back(atz[d[j].dpos + 8 * d[j].nd + i]);
      }
    }
    if (!increasing) {   // crafted deltas (wrap / zero): the last write to a position wins
      std::vector<std::pair<uint64_t, size_t>> o;
      for (size_t q = p0; q < pat.size(); q++) o.push_back({pat[q], q});
      std::stable_sort(o.begin(), o.end(), [](const std::pair<uint64_t, size_t>& a, const std::pair<uint64_t, size_t>& b) { return a.first < b.first; });
      std::vector<uint64_t> pa;
      std::vector<uint8_t> pv;
      for (size_t q = 0; q < o.size(); q++)
        if (q + 1 == o.size() || o[q + 1].first != o[q].first) { pa.push_back(o[q].first); pv.push_back(pval[o[q].second]); }
      pat.resize(p0); pval.resize(p0);
      pat.insert(pat.end(), pa.begin(), pa.end());
      pval.insert(pval.end(), pv.begin(), pv.end());
    }
    // (ascending: the first and the last bound them all)
    if (pat.size() > p0 && (pat[p0] < rec_base + rec_off || pat.back() - rec_base - rec_off >= d[j].hull())) return ATZ_E_INTERNAL;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Writer (main.cpp:764-834)
struct WriteRec {   // one record of the file; the parameters, diffs and payload only where recomp
  uint64_t off = 0, comp_len = 0, infl_len = 0;
  bool recomp = false;
  uint8_t c = 0, w = 0, m = 0;      // the descriptor bytes, c without its bit 7
  int64_t first_diff = -1;
  uint64_t nd = 0;                  // diffs: ascending positions in the stream and the bytes there
  const uint32_t* pos = nullptr;
  const uint8_t* val = nullptr;
  uint64_t payload = 0;             // the inflated bytes' absolute address
  // a stitched record's k pieces in the file (12 framing bytes between two; off is the first one's); k = 0: none
  uint32_t k = 0;
  const uint64_t* piece_off = nullptr;
  const uint64_t* piece_len = nullptr;
};

// The writers below take the file's n records as rec(s) -> WriteRec, s in file order (called more than once per
// record, so that no table of them is built).

// The header, as its own segment at the file's start; -> the bytes written so far.
inline uint64_t write_header(std::vector<uint8_t>& meta, std::vector<Seg>& segs, uint64_t F, uint64_t nrec, uint8_t version) {
  const uint8_t h[4] = {'A', 'T', 'Z', version};
  meta.insert(meta.end(), h, h + 4);
  put8(meta, 0); put8(meta, F); put8(meta, nrec);   // length back-patched (main.cpp:776, 797-800)
  segs.push_back({SEG_META, 0, 0, 0, meta.size()});
  return meta.size();
}
inline void write_length(std::vector<uint8_t>& meta, uint64_t out) { std::memcpy(meta.data() + 4, &out, 8); }

// Stream descriptors + inflated payloads of the recompressed streams, in record order
// (writeStreamdesc, main.cpp:805-831): metadata bytes into `meta`, copy segments into `segs`.
// stripped: without the payload bytes (a nested file's outer)
template <class Get>
inline void write_descriptors(size_t n, Get rec, std::vector<uint8_t>& meta, std::vector<Seg>& segs, uint64_t& out,
                              bool stripped = false) {
  segs.reserve(segs.size() + 2 * n + 8);
  for (size_t s = 0; s < n; s++) {
    const WriteRec r = rec(s);
    if (!r.recomp) continue;
    const size_t m0 = meta.size();   // the stream descriptor goes straight into meta
    put8(meta, r.off); put8(meta, r.comp_len); put8(meta, r.infl_len);
    // (version 4: bit 7 of the clevel byte marks a stitched descriptor, whose piece list follows its payload)
    meta.push_back((uint8_t)(r.c | (r.k ? DeflSpec::DESC_STITCHED : 0))); meta.push_back(r.w); meta.push_back(r.m);
    put8(meta, r.nd);
    if (r.nd) {
      put8(meta, (uint64_t)r.first_diff);
      for (uint64_t q = 0; q < r.nd; q++) put8(meta, q == 0 ? 0 : (uint64_t)r.pos[q] - r.pos[q - 1]);
      meta.insert(meta.end(), r.val, r.val + r.nd);
    }
    segs.push_back({SEG_META, 0, m0, out, meta.size() - m0});
    out += meta.size() - m0;
    if (!stripped) {
      segs.push_back({SEG_ADDR, 0, r.payload, out, r.infl_len});
      out += r.infl_len;
    }
    if (r.k) {   // u32 k, k x u32 piece lengths (piece i starts at offset + sum_{j<i} (len_j + 12))
      const size_t m1 = meta.size();
      put4(meta, r.k);
      for (uint32_t q = 0; q < r.k; q++) put4(meta, (uint32_t)r.piece_len[q]);
      segs.push_back({SEG_META, 0, m1, out, meta.size() - m1});
      out += meta.size() - m1;
    }
  }
}

// The residue (main.cpp:784-796): every file byte outside the recompressed streams, in order.
// rec[k] = (offset, comp_len) of every record of the file, recomp[k] its decision.
inline int write_residue(const std::vector<std::pair<uint64_t, uint64_t>>& rec, const uint8_t* recomp, uint64_t F,
                         std::vector<Seg>& segs, uint64_t& out) {
  uint64_t lastos = 0, lastlen = 0;
  auto copy = [&](uint64_t off, uint64_t len) {   // (inside the file)
    segs.push_back({SEG_FILE, 0, off, out, len});
    out += len;
    return inside(off, len, F);
  };
  for (size_t s = 0; s < rec.size(); s++) {
    const uint64_t off = rec[s].first, len = rec[s].second;
    if (lastos + lastlen != off) {
      if (off < lastos + lastlen) return ATZ_E_REF_UB;   // copyto() with a wrapped length
      if (!copy(lastos + lastlen, off - (lastos + lastlen))) return ATZ_E_INTERNAL;
    }
    if (!recomp[s] && !copy(off, len)) return ATZ_E_INTERNAL;
    lastos = off; lastlen = len;
  }
  if (lastos + lastlen < F && !copy(lastos + lastlen, F - (lastos + lastlen))) return ATZ_E_INTERNAL;
  return 0;
}

// The whole file of the F-byte original's records: header, descriptors, residue (a stitched record occupies one range
// per piece: the framing between them is residue); out: the ATZ's length.  The version is the lowest whose reader
// accepts every recorded stream: ATZ1 unless one needs more.
template <class Get>
inline int write_file(size_t n, Get rec, uint64_t F, std::vector<uint8_t>& meta, std::vector<Seg>& segs, uint64_t& out,
                      bool stripped = false) {
  uint64_t nrec = 0;
  size_t npieces = 0;
  uint8_t version = 1;
  std::vector<std::pair<uint64_t, uint64_t>> range;
  std::vector<uint8_t> rc;
  for (int pass = 0; pass < 2; pass++) {   // count, then fill
    range.reserve(npieces); rc.reserve(npieces);
    for (size_t s = 0; s < n; s++) {
      const WriteRec r = rec(s);
      if (!pass) {
        nrec += r.recomp; npieces += r.k ? r.k : 1;
        if (r.recomp) version = std::max(version, DeflSpec::from_desc(r.c, r.w, r.m).min_version(r.k != 0));
      } else if (!r.k) {
        range.push_back({r.off, r.comp_len}); rc.push_back(r.recomp);
      } else {
        for (uint32_t q = 0; q < r.k; q++) { range.push_back({r.piece_off[q], r.piece_len[q]}); rc.push_back(r.recomp); }
      }
    }
  }
  meta.reserve(28 + nrec * 43 + 64);
  out = write_header(meta, segs, F, nrec, version);
  write_descriptors(n, rec, meta, segs, out, stripped);
  if (int r = write_residue(range, rc.data(), F, segs, out)) return r;
  write_length(meta, out);
  return 0;
}

// P of the records: the recorded streams' payloads, concatenated in descriptor order with no padding; segs gather
// them (absolute addresses) to offsets of P, plen its length; -> the number of recorded streams
template <class Get>
inline uint64_t plan_payloads(size_t n, Get rec, std::vector<Seg>& segs, uint64_t& plen) {
  uint64_t nrec = 0;
  plen = 0;
  for (size_t s = 0; s < n; s++) {
    const WriteRec r = rec(s);
    if (!r.recomp) continue;
    nrec++;
    if (r.infl_len) push_split(segs, {SEG_ADDR, 0, r.payload, plen, r.infl_len});
    plen += r.infl_len;
  }
  return nrec;
}

// The nested file of a stripped outer (meta, segs and outer_len as write_file left them) and the inner file, inner_len
// bytes at absolute address inner: the outer's segments move behind the 20 header bytes, the inner file follows them.
inline int write_nest(std::vector<uint8_t>& meta, std::vector<Seg>& segs, uint64_t outer_len, uint64_t inner,
                      uint64_t inner_len, uint64_t& out) {
  const uint64_t top = ~0ull - NEST_HEADER;
  if (outer_len > top || inner_len > top - outer_len) return ATZ_E_INTERNAL;
  for (Seg& g : segs) {
    if (!inside(g.dst_off, g.len, outer_len)) return ATZ_E_INTERNAL;
    g.dst_off += NEST_HEADER;
  }
  out = NEST_HEADER + outer_len + inner_len;
  const size_t m0 = meta.size();
  const uint8_t h[4] = {'A', 'T', 'N', 1};
  meta.insert(meta.end(), h, h + 4);
  put8(meta, out); put8(meta, outer_len);
  segs.push_back({SEG_META, 0, m0, 0, NEST_HEADER});
  if (inner_len) push_split(segs, {SEG_ADDR, 0, inner, NEST_HEADER + outer_len, inner_len});
  return 0;
}

}  // namespace atz
