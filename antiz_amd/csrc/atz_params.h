// atz_params.h -- the parameters of one deflate and their encodings (host only, plain C++17, no HIP header).
// The only place that knows the bit positions; DESIGN.md s7.7 tabulates the encodings.
//   word : flush<<30 | gnu<<29 | raw<<28 | strategy<<24 | level<<16 | window<<8 | memLevel: atz_deflate_batch_ex's
//          params and the candidate lists' entries (which mark GNU by memLevel 0, the ABI by bit 29)
//   desc : the bytes clevel = stitched<<7 | raw<<6 | strategy<<4 | level, window (0x8F: a flush-terminated body of
//          window 15) and memLevel (0: a GNU-family body) of an ATZ descriptor, StreamState and atz_result_t.
//          Stitching belongs to the record, not to the parameters: bit 7 goes in and out beside the DeflSpec.
// ATZ versions, by what a descriptor may carry:
//   1  level 0-9, window 8-15, memLevel 1-9: the reference's file
//   2  the strategy extension's: clevel = strategy << 4 | level (same layout)
//   3  the container extension's: clevel = raw << 6 | strategy << 4 | level
//   4  the stitch extension's: bit 7 of clevel, never with bit 6; a stitched descriptor's piece list follows its
//      payload (u32 k, k x u32 lengths)
//   5  the deflater extension's: a raw, unstitched descriptor with the default strategy, level 1-9, window 15 and
//      memLevel byte 0 is a GNU-family body
//   6  the segment extension's: a raw, unstitched descriptor with the default strategy, memLevel 1-9 and window
//      byte 0x8F is a flush-terminated body of window 15
#pragma once
#include <array>
#include <cstdint>
#include <vector>

namespace atz {

struct DeflSpec {
  int level = 0, window = 15;
  int memlevel = 8;    // zlib's memLevel; 8 for a GNU-family deflate, whose parse is zlib's at memLevel 8
  uint32_t strategy = 0;   // zlib's number: 0 default, 1 Z_FILTERED, 2 Z_HUFFMAN_ONLY, 3 Z_RLE
  bool raw = false;    // no zlib header, no Adler-32 trailer
  bool gnu = false;    // GNU gzip's and Info-ZIP's deflater (raw, window 15, level 1-9, default strategy)
  bool flush = false;  // the body ends as a full flush ends it (raw, zlib's deflater, default strategy)

  static constexpr uint8_t DESC_STITCHED = 0x80;   // bit 7 of a descriptor's clevel byte

  static DeflSpec from_word(uint32_t p) {
    DeflSpec s;
    s.level = (int)((p >> 16) & 0xff); s.window = (int)((p >> 8) & 0xff);
    s.strategy = (p >> 24) & 3u;
    s.raw = (p >> 28) & 1u; s.flush = (p >> 30) & 1u;
    s.gnu = ((p >> 29) & 1u) || !(p & 0xff);
    s.memlevel = s.gnu ? 8 : (int)(p & 0xff);
    return s;
  }
  // from_word reads both forms.  word() writes the ABI form with a memLevel field of 0, which either reading takes
  // for GNU; the list form is still read because raw_list keeps its entries as the tests' models pin them.
  uint32_t word() const {
    return ((uint32_t)flush << 30) | ((uint32_t)gnu << 29) | ((uint32_t)raw << 28) | (strategy << 24) |
           ((uint32_t)level << 16) | ((uint32_t)window << 8) | (gnu ? 0u : (uint32_t)memlevel);
  }
  static DeflSpec from_desc(uint8_t c, uint8_t w, uint8_t m, bool* stitched = nullptr) {
    DeflSpec s;
    s.level = c & 15; s.strategy = (c >> 4) & 3u; s.raw = (c >> 6) & 1u;
    s.window = w & 0x7f; s.flush = (w >> 7) & 1u;
    s.gnu = m == 0; s.memlevel = s.gnu ? 8 : m;
    if (stitched) *stitched = (c & DESC_STITCHED) != 0;
    return s;
  }
  std::array<uint8_t, 3> desc(bool stitched = false) const {   // {clevel, window, memLevel}
    return {(uint8_t)((stitched ? DESC_STITCHED : 0) | ((int)raw << 6) | (int)(strategy << 4) | level),
            (uint8_t)(window | ((int)flush << 7)), (uint8_t)(gnu ? 0 : memlevel)};
  }

  int table_memlevel() const { return memlevel; }   // whose bucket and match tables the trial reads (GNU: 8)
  bool needs_tables() const { return level > 0 && strategy < 2; }   // Z_RLE, Z_HUFFMAN_ONLY and level 0 read none
  uint8_t mode() const { return (uint8_t)((raw ? 2 : 0) | (flush ? 64 : 0)); }   // TM_RAW | TM_FLUSH (atz_device.h)
  // the lowest ATZ version whose reader accepts this descriptor
  uint8_t min_version(bool stitched) const {
    return flush ? 6 : gnu ? 5 : stitched ? 4 : raw ? 3 : strategy ? 2 : 1;
  }
  static constexpr uint8_t MAX_VERSION = 6;   // the highest version a reader accepts (and min_version returns)
};

// A reader of `version` (1-6) accepts the descriptor bytes (c with its bit 7).  parse_atz's size and layout
// checks are not made here.
inline bool valid_desc(int version, uint8_t c, uint8_t w, uint8_t m) {
  const int level = c & 15, sg = (c >> 4) & 3;
  if (version >= 3) {
    if ((c & 0x80) && (version < 4 || (c & 0x40))) return false;
  } else if ((c >> 4) > (version == 2 ? 3 : 0)) return false;
  if (level > 9 || (sg >= 2 && level < 1)) return false;   // Z_HUFFMAN_ONLY and Z_RLE have no level 0
  const bool plain_raw = (c & 0xf0) == 0x40;   // raw, not stitched, default strategy
  if (version >= 5 && m == 0) return plain_raw && level >= 1 && w == 15;
  if (version >= 6 && (w & 0x80)) return w == 0x8f && plain_raw && m <= 9;
  return w >= 8 && w <= 15 && m >= 1 && m <= 9;
}

// atz_deflate_batch{,_ex} accept the params word p; *out: its parameters, window 8 raised to 9 as zlib does.
// Without ex, bits 16-31 are the level (so any extension bit is a level past 9).
inline bool valid_api(uint32_t p, bool ex, DeflSpec* out) {
  DeflSpec s;
  s.raw = ex && ((p >> 28) & 1u); s.gnu = ex && ((p >> 29) & 1u); s.flush = ex && ((p >> 30) & 1u);
  const uint32_t sg = ex ? (p >> 24) & 0x8fu : 0u;   // Z_FIXED (4) and up, and bit 31, are refused
  const uint32_t cl = ex ? (p >> 16) & 0xff : p >> 16, w = (p >> 8) & 0xff, m = p & 0xff;
  if (s.gnu ? (!s.raw || sg != 0 || w != 15 || cl < 1) : (m < 1 || m > 9)) return false;   // (GNU: memLevel ignored)
  if (s.flush && (!s.raw || s.gnu || sg != 0 || w < 9)) return false;
  if (cl > 9 || w < 8 || w > 15 || sg > 3 || (sg >= 2 && cl < 1)) return false;
  s.level = (int)cl; s.window = w == 8 ? 9 : (int)w; s.memlevel = s.gnu ? 8 : (int)m; s.strategy = sg;
  *out = s;
  return true;
}

// The candidate lists.  Entries are words in the list form.
inline uint32_t pk(int c, int w, int m) { return ((uint32_t)c << 16) | ((uint32_t)w << 8) | (uint32_t)m; }

inline void prange(std::vector<uint32_t>& l, int cmin, int cmax, int wmin, int wmax, int mmin, int mmax) {
  for (int w = wmax; w >= wmin; w--)
    for (int m = mmax; m >= mmin; m--)
      for (int c = cmax; c >= cmin; c--) l.push_back(pk(c, w, m));
}
// tryParamsFastest/Fast/Default/Best (main.cpp:487-560)
inline void list_a(std::vector<uint32_t>& l, int type) {
  if (type >= 24) return;   // a raw record (the container extension): the reference walk leaves it alone
  int w = 10 + type / 4;
  switch (type % 4) {
    case 0: l.push_back(pk(0, w, 8)); l.push_back(pk(1, w, 8)); l.push_back(pk(1, w, 9));
            prange(l, 1, 1, w, w, 1, 7); prange(l, 2, 9, w, w, 1, 9); break;
    case 1: prange(l, 2, 5, w, w, 8, 8); prange(l, 2, 5, w, w, 1, 7); prange(l, 2, 5, w, w, 9, 9);
            prange(l, 1, 1, w, w, 1, 9); prange(l, 6, 9, w, w, 1, 9); break;
    case 2: l.push_back(pk(6, w, 8)); l.push_back(pk(6, w, 9)); prange(l, 6, 6, w, w, 1, 7);
            prange(l, 1, 5, w, w, 1, 9); prange(l, 7, 9, w, w, 1, 9); break;
    default: prange(l, 7, 9, w, w, 8, 8); prange(l, 7, 9, w, w, 1, 7); prange(l, 7, 9, w, w, 9, 9);
             prange(l, 1, 6, w, w, 1, 9); break;
  }
}
// brute-window continuation (main.cpp:590-601)
inline void list_b(std::vector<uint32_t>& l, int type) {
  if (type >= 24) return;
  int w = 10 + type / 4;
  if (w == 10) prange(l, 1, 9, 11, 15, 1, 9);
  else if (w == 15) prange(l, 1, 9, 10, 14, 1, 9);
  else { prange(l, 1, 9, 10, w - 1, 1, 9); prange(l, 1, 9, w + 1, 15, 1, 9); }
}

// The trial lists depend only on the header type (24) and the phase: built once, shared by streams.
inline const std::vector<uint32_t>& trial_list(int type, bool brute) {
  static const std::array<std::array<std::vector<uint32_t>, 27>, 2> L = [] {   // 24..26: raw records, empty
    std::array<std::array<std::vector<uint32_t>, 27>, 2> t;
    for (int ty = 0; ty < 27; ty++) { list_a(t[0][ty], ty); list_b(t[1][ty], ty); }
    return t;
  }();
  return L[brute ? 1 : 0][type];
}

// Opt-in strategy trials (atz_set_strategies): the streams the reference walk left with
// recomp == 0 get a second walk under the same rule (main.cpp:616-700, restarted with identBytes = 0) over
// the candidates their header's FLEVEL allows -- zlib writes FLEVEL from level and strategy
// (Z/deflate.c:738-750): 0 for strategy >= Z_HUFFMAN_ONLY, else by level -- at the header's window,
// memLevels 8, 9, 7..1, levels descending within a memLevel.  Entries: (strategy<<24)|(c<<16)|(w<<8)|m.
inline void strategy_list(std::vector<uint32_t>& l, int type, uint32_t mask) {
  if (type >= 24) return;   // raw records take no strategy trials
  const int w = 10 + type / 4;
  static const int mo[9] = {8, 9, 7, 6, 5, 4, 3, 2, 1};
  auto add = [&](uint32_t strat, int chi, int clo) {
    if (!((mask >> strat) & 1u)) return;
    for (int m : mo)
      for (int cl = chi; cl >= clo; cl--) l.push_back((strat << 24) | pk(cl, w, m));
  };
  switch (type % 4) {
    case 0: add(3, 6, 6); add(2, 6, 6); break;   // the parse ignores the level: recorded as 6
    case 1: add(1, 5, 4); break;                 // (levels 1-3 ignore Z_FILTERED: the default list's)
    case 2: add(1, 6, 6); break;
    default: add(1, 9, 7); break;
  }
}

// The raw walk (the container extension): a record of type 24 + hint is a raw deflate body
// of C = comp_len bytes behind a ZIP or gzip header.  Its candidates: window 15 (what ZIP and gzip writers
// use; --brute-window does not widen it), the default strategy, memLevels 8, 9, 7..1, and inside a
// memLevel the levels in the order its container's hint suggests -- 90 entries, raw << 28 | c << 16 |
// 15 << 8 | m.  The rule is strategy_pass's, on the body: a recorded one gets clevel = 1 << 6 | level.
// defl_mask bit 0 (atz_set_deflaters): GNU gzip's and Info-ZIP's deflater, levels 1-9 in the
// hint's order, marked with memLevel 0, directly behind the memLevel-8 group (their parse is zlib's at
// memLevel 8, so they share its tables) -- 99 entries.
// flush (a record with flags bit 7, the segment extension's): every entry carries bit 30, which
// makes its trial TM_FLUSH, and no GNU candidate is added (gzip has no full flush) -- 90 entries.
inline void raw_list(std::vector<uint32_t>& l, int type, uint32_t defl_mask, bool flush) {
  if (type < 24 || type > 26) return;
  if (flush) defl_mask = 0;
  const uint32_t fb = flush ? 1u << 30 : 0u;
  static const int mo[9] = {8, 9, 7, 6, 5, 4, 3, 2, 1};
  static const int lo[3][10] = {{6, 9, 1, 5, 7, 8, 4, 3, 2, 0},    // no hint
                                {1, 2, 3, 4, 5, 6, 7, 8, 9, 0},    // fast
                                {9, 8, 7, 6, 5, 4, 3, 2, 1, 0}};   // max
  for (int m : mo) {
    for (int cl : lo[type - 24]) l.push_back(fb | (1u << 28) | pk(cl, 15, m));
    if (m == 8 && (defl_mask & 1u))
      for (int cl : lo[type - 24])
        if (cl) l.push_back((1u << 28) | pk(cl, 15, 0));
  }
}

}  // namespace atz
