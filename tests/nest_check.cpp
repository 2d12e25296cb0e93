// nest_check -- format_check's twin for nested files ("ATN" 1): a host executor of
// antiz_amd/csrc/atz_format.h for tests/test_nest_cpu.py (stand-alone: it includes only that header; built with
// -fsanitize=address,undefined).  What k_gather and k_patch do with a plan's segments and patches on the GPU is done
// here with memcpy, after every range has been checked against the buffer its source names.  The buffers live at fake
// base addresses far apart, so a wrong address cannot alias a right one.
//   nest_check parse ATN...                   N rc levels, then per level (outermost first) L pos len version origlen
//                                             nstreams stripped and per descriptor D off cl il c w m nd fd k ipos
//   nest_check rebuild (ATN OUTS REBUILT)...  the parse lines, then R rc; OUTS: the "deflate outputs" of every level's
//                                             streams, innermost level first, per stream u64 length + that many bytes;
//                                             REBUILT is written where rc is 0.  A flat ATZ file is one level.
//   nest_check write TABLE ORIG INNER OUT     W rc length plen; TABLE as format_check's; the stripped outer of the
//                                             table's records joined with the file INNER (placed at a fake address)
//                                             goes to OUT, and P of the records (plan_payloads) to OUT.p
// A range outside its buffer, overlapping destinations, a byte of the result left unwritten or patch addresses out
// of order: a message on stderr and exit status 3.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>

#include "atz_format.h"

using namespace atz;
using Bytes = std::vector<uint8_t>;

static const uint64_t SLAB = 1ull << 40, OUTS = 2ull << 40, INNER = 3ull << 40, ORIG = 8ull << 40;
static const size_t BATCH = 3;   // streams per plan_batch call
static uint64_t orig_base(size_t level) { return ORIG + ((uint64_t)level << 40); }

[[noreturn]] static void die(int code, const std::string& why) {
  std::fprintf(stderr, "nest_check: %s\n", why.c_str());
  std::exit(code);
}
static void require(bool ok, const char* what) { if (!ok) die(3, what); }

static Bytes slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) die(2, std::string("cannot read ") + path);
  return Bytes(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static void spill(const std::string& path, const Bytes& b) {
  std::ofstream f(path, std::ios::binary);
  f.write((const char*)b.data(), (std::streamsize)b.size());
  if (!f) die(2, std::string("cannot write ") + path);
}

struct Region { uint64_t base, len; const uint8_t* p; };   // readable bytes at a fake absolute address

// One gather into dst: every source range inside the buffer its src names (file: [file_lo, file_n) of `file`; meta;
// for an absolute address, one of `abs`), every destination inside dst, then the copies.  `cover` collects the
// destinations for the caller's check that the gathers into one buffer tile it.
static void gather(const std::vector<Seg>& segs, const uint8_t* file, uint64_t file_lo, uint64_t file_n, const Bytes& meta,
                   const std::vector<Region>& abs, Bytes& dst, std::vector<std::pair<uint64_t, uint64_t>>& cover) {
  for (const Seg& g : segs) {
    require(g.src <= SEG_ZERO, "segment source unknown");
    require(inside(g.dst_off, g.len, dst.size()), "segment destination outside its buffer");
    cover.push_back({g.dst_off, g.len});
    const uint8_t* from = nullptr;
    if (g.src == SEG_FILE) {
      require(g.src_off >= file_lo && inside(g.src_off, g.len, file_n), "file segment outside the file");
      from = file + g.src_off;
    } else if (g.src == SEG_META) {
      require(inside(g.src_off, g.len, meta.size()), "metadata segment outside the metadata");
      from = meta.data() + g.src_off;
    } else if (g.src == SEG_ADDR) {
      for (const Region& r : abs)
        if (g.src_off >= r.base && inside(g.src_off - r.base, g.len, r.len)) from = r.p + (g.src_off - r.base);
      require(from != nullptr || g.len == 0, "address segment outside every buffer");
    }
    if (!g.len) continue;
    if (g.src == SEG_ZERO) std::memset(dst.data() + g.dst_off, 0, g.len);
    else std::memcpy(dst.data() + g.dst_off, from, g.len);
  }
}
// the destinations are disjoint and, where `whole`, tile [0, size)
static void check_cover(std::vector<std::pair<uint64_t, uint64_t>> cover, uint64_t size, bool whole) {
  std::sort(cover.begin(), cover.end());
  uint64_t at = 0;
  for (const auto& c : cover) {
    if (!c.second) continue;
    require(c.first >= at, "segment destinations overlap");
    require(!whole || c.first == at, "bytes of the result left unwritten");
    at = c.first + c.second;
  }
  require(!whole || at == size, "the result's end left unwritten");
}

// a flat ATZ file as the one level parse_nest would make of it
static int parse_any(const Bytes& a, std::vector<NestLevel>& lv) {
  if (is_nest(a.data(), a.size())) return parse_nest(a.data(), a.size(), lv);
  lv.assign(1, NestLevel{});
  lv[0].pos = 0; lv[0].len = a.size();
  const int rc = parse_atz(a.data(), a.size(), lv[0].d, lv[0].origlen, lv[0].residue);
  if (rc) lv.clear();
  return rc;
}

static int parse_and_print(const Bytes& a, std::vector<NestLevel>& lv) {
  const int rc = parse_any(a, lv);
  std::printf("N %d %zu\n", rc, rc ? (size_t)0 : lv.size());
  if (rc) return rc;
  for (size_t k = 0; k < lv.size(); k++) {
    const NestLevel& L = lv[k];
    require(inside(L.pos, L.len, a.size()) && L.len >= 28, "level outside the file");
    std::printf("L %llu %llu %d %llu %zu %d\n", (unsigned long long)L.pos, (unsigned long long)L.len, a[L.pos + 3],
                (unsigned long long)L.origlen, L.d.size(), (int)(k + 1 < lv.size()));
    for (const AtzDesc& x : L.d)
      std::printf("D %llu %llu %llu %u %u %u %llu %llu %llu %llu\n", (unsigned long long)x.off, (unsigned long long)x.cl,
                  (unsigned long long)x.il, x.c, x.w, x.m, (unsigned long long)x.nd, (unsigned long long)x.fd,
                  (unsigned long long)x.k, (unsigned long long)x.ipos);
  }
  return 0;
}

// One level: its original from its bytes a[0, n), its streams' outputs (outs, from `at` on) and, for a stripped
// level, P (the level inside it, already rebuilt) at fake address pbase
static int rebuild_level(const uint8_t* a, uint64_t n, const NestLevel& V, bool stripped, const Bytes* P, uint64_t pbase,
                         const Bytes& outs, size_t& at, uint64_t rec_base, Bytes& orig) {
  const std::vector<AtzDesc>& d = V.d;
  const uint64_t origlen = V.origlen, residue = V.residue;
  PayloadSrc src;
  std::vector<Region> pregion;
  if (stripped) {
    src.stripped = true; src.pbase = pbase; src.plen = P->size();
    pregion.push_back({pbase, P->size(), P->data()});
  }
  RecLayout L;
  if (int rc = plan_layout(a, n, d, origlen, residue, L, src)) return rc;
  const size_t ns = d.size();
  if (origlen > (1ull << 30) || L.slab > (1ull << 30)) die(2, "a file this large is not for this program");
  orig.assign(origlen, 0xEE);
  std::vector<std::pair<uint64_t, uint64_t>> cover, slab_cover;
  gather(L.gaps, a, residue, n, {}, {}, orig, cover);
  Bytes slab(L.slab, 0xEE);
  // (a stripped level copies no payload from its file, a flat one none from an address)
  gather(L.payloads, a, stripped ? n : 28, n, {}, pregion, slab, slab_cover);
  check_cover(slab_cover, slab.size(), false);
  require(L.rec_off.size() == ns && L.loc.size() == ns && L.params.size() == ns, "layout tables of another size");
  for (size_t j = 0; j < ns; j++) {
    require(L.loc[j] % 256 == 0 && inside(L.loc[j], d[j].il, slab.size()), "payload outside the slab");
    const uint8_t* want = stripped ? P->data() + d[j].ipos : a + d[j].ipos;
    require(inside(d[j].ipos, d[j].il, stripped ? P->size() : n), "payload outside its source");
    require(!d[j].il || !std::memcmp(slab.data() + L.loc[j], want, d[j].il), "payload bytes differ");
  }
  for (size_t s0 = 0; s0 < ns; s0 += BATCH) {
    const size_t s1 = std::min(ns, s0 + BATCH);
    std::vector<uint64_t> oa, ol;
    std::vector<Region> regions;
    uint64_t off = 0;
    for (size_t j = s0; j < s1; j++) {
      if (outs.size() - at < 8) die(2, "outputs file too short");
      const uint64_t len = rd8(outs.data() + at);
      at += 8;
      if (len > outs.size() - at) die(2, "outputs file too short");
      oa.push_back(OUTS + off); ol.push_back(len);
      regions.push_back({OUTS + off, len, outs.data() + at});
      at += len; off += (len + 255 + 256) & ~255ull;   // (a hole between two outputs)
    }
    RecBatch B;
    if (int rc = plan_batch(a, d, L, origlen, s0, s1, oa, ol, rec_base, B)) return rc;
    gather(B.segs, a, n, n, {}, regions, orig, cover);   // (a batch copies nothing from the file)
    require(B.pat.size() == B.pval.size(), "patch lists of two sizes");
    for (size_t q = 0; q < B.pat.size(); q++) {
      require(B.pat[q] >= rec_base && B.pat[q] - rec_base < origlen, "patch outside the original");
      require(!q || B.pat[q] > B.pat[q - 1], "patch addresses not strictly ascending");
    }
    for (size_t q = 0; q < B.pat.size(); q++) orig[B.pat[q] - rec_base] = B.pval[q];
  }
  check_cover(cover, origlen, true);
  return 0;
}

static int rebuild(const Bytes& a, const Bytes& outs, Bytes& orig) {
  std::vector<NestLevel> lv;
  if (int rc = parse_and_print(a, lv)) return rc;
  size_t at = 0;
  Bytes inner;   // the level inside the current one, rebuilt: its P
  for (size_t k = lv.size(); k-- > 0;) {
    const bool stripped = k + 1 < lv.size();
    Bytes out;
    if (int rc = rebuild_level(a.data() + lv[k].pos, lv[k].len, lv[k], stripped, &inner, orig_base(k + 1), outs, at,
                               orig_base(k), out))
      return rc;
    inner.swap(out);
  }
  orig.swap(inner);
  return 0;
}

static Bytes unhex(const std::string& s) {
  Bytes b;
  if (s == "-") return b;
  for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return b;
}

static int write_mode(const char* table, const char* orig_path, const char* inner_path, const char* out_path) {
  std::ifstream t(table);
  if (!t) die(2, std::string("cannot read ") + table);
  const Bytes file = slurp(orig_path), inner = slurp(inner_path);
  size_t n = 0;
  t >> n;
  std::vector<WriteRec> recs(n);
  std::vector<std::vector<uint32_t>> pos(n);
  std::vector<Bytes> val(n), payload(n);
  std::vector<std::vector<uint64_t>> poff(n), plen(n);
  std::vector<Region> regions;
  uint64_t at = 0;
  for (size_t s = 0; s < n; s++) {
    WriteRec& r = recs[s];
    unsigned c, w, m, recomp;
    std::string hex;
    t >> r.off >> r.comp_len >> r.infl_len >> recomp >> c >> w >> m >> r.first_diff >> r.nd >> r.k;
    r.recomp = recomp != 0; r.c = (uint8_t)c; r.w = (uint8_t)w; r.m = (uint8_t)m;
    pos[s].resize(r.nd); poff[s].resize(r.k); plen[s].resize(r.k);
    for (uint32_t& p : pos[s]) t >> p;
    t >> hex; val[s] = unhex(hex);
    for (uint64_t& p : poff[s]) t >> p;
    for (uint64_t& p : plen[s]) t >> p;
    t >> hex; payload[s] = unhex(hex);
    if (!t || val[s].size() != r.nd || (r.recomp && payload[s].size() != r.infl_len)) die(2, "bad table");
    r.pos = pos[s].data(); r.val = val[s].data(); r.piece_off = poff[s].data(); r.piece_len = plen[s].data();
    r.payload = SLAB + at;
    regions.push_back({SLAB + at, payload[s].size(), payload[s].data()});
    at += (payload[s].size() + 255 + 256) & ~255ull;
  }
  auto rec = [&](size_t s) { return recs[s]; };
  // P, gathered from the payloads where they lie
  std::vector<Seg> psegs;
  uint64_t pl = 0;
  plan_payloads(n, rec, psegs, pl);
  Bytes P(pl, 0xEE);
  std::vector<std::pair<uint64_t, uint64_t>> pcover;
  for (const Seg& g : psegs) require(g.len <= SEG_SPLIT, "a payload segment longer than the split size");
  gather(psegs, nullptr, 0, 0, {}, regions, P, pcover);
  check_cover(pcover, pl, true);
  // the stripped outer never reads a payload: only the inner file is addressable
  Bytes meta;
  std::vector<Seg> segs;
  uint64_t outer = 0, out = 0;
  int rc = write_file(n, rec, file.size(), meta, segs, outer, true);
  if (!rc) rc = write_nest(meta, segs, outer, INNER, inner.size(), out);
  std::printf("W %d %llu %llu\n", rc, (unsigned long long)(rc ? 0 : out), (unsigned long long)pl);
  if (rc) return rc;
  for (const Seg& g : segs) require(g.len <= SEG_SPLIT || g.src != SEG_ADDR, "an inner segment longer than the split size");
  Bytes atn(out, 0xEE);
  std::vector<std::pair<uint64_t, uint64_t>> cover;
  gather(segs, file.data(), 0, file.size(), meta, {{INNER, inner.size(), inner.data()}}, atn, cover);
  check_cover(cover, out, true);
  spill(out_path, atn);
  spill(std::string(out_path) + ".p", P);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "parse") {
    for (int i = 2; i < argc; i++) {
      std::vector<NestLevel> lv;
      parse_and_print(slurp(argv[i]), lv);
    }
  } else if (mode == "rebuild" && argc % 3 == 2) {
    for (int i = 2; i < argc; i += 3) {
      Bytes orig;
      const int rc = rebuild(slurp(argv[i]), slurp(argv[i + 1]), orig);
      std::printf("R %d\n", rc);
      if (!rc) spill(argv[i + 2], orig);
    }
  } else if (mode == "write" && argc == 6) {
    write_mode(argv[2], argv[3], argv[4], argv[5]);
  } else {
    die(2, "usage: nest_check parse ATN... | rebuild (ATN OUTS REBUILT)... | write TABLE ORIG INNER OUT");
  }
  return 0;
}
