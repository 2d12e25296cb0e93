// format_check -- a host executor of antiz_amd/csrc/atz_format.h for tests/test_format_cpu.py (stand-alone: it
// includes only that header; built with -fsanitize=address,undefined).  What k_gather and k_patch do with a plan's
// segments and patches on the GPU is done here with memcpy, after every range has been checked against the buffer
// its source names.  The buffers live at fake base addresses far apart, so a wrong address cannot alias a right one.
//   format_check parse ATZ...                   P rc version origlen nstreams, then per descriptor
//                                               D off cl il c w m nd fd k ipos
//   format_check rebuild (ATZ OUTS REBUILT)...  the parse lines, per stream S level window memlevel strategy raw gnu
//                                               flush loc, then R rc; OUTS: per stream u64 length + that many bytes,
//                                               the "deflate outputs"; REBUILT is written where rc is 0
//   format_check write TABLE ORIG ATZ           W rc length; TABLE: the record count, then per record
//                                               off comp_len infl_len recomp c w m first_diff nd k, nd positions,
//                                               the values in hex (or -), k piece offsets, k piece lengths, the
//                                               payload in hex (or -)
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

static const uint64_t SLAB = 1ull << 40, OUTS = 2ull << 40, ORIG = 3ull << 40;
static const size_t BATCH = 3;   // streams per plan_batch call

[[noreturn]] static void die(int code, const std::string& why) {
  std::fprintf(stderr, "format_check: %s\n", why.c_str());
  std::exit(code);
}
static void require(bool ok, const char* what) { if (!ok) die(3, what); }

static Bytes slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) die(2, std::string("cannot read ") + path);
  return Bytes(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static void spill(const char* path, const Bytes& b) {
  std::ofstream f(path, std::ios::binary);
  f.write((const char*)b.data(), (std::streamsize)b.size());
  if (!f) die(2, std::string("cannot write ") + path);
}

struct Region { uint64_t base, len; const uint8_t* p; };   // readable bytes at a fake absolute address

// One gather into dst: every source range inside the buffer its src names (file; meta; for an absolute address, one
// of `abs`), every destination inside dst and disjoint from the others', then the copies.  `cover` collects the
// destinations for the caller's check that the gathers into one buffer tile it.
static void gather(const std::vector<Seg>& segs, const Bytes& file, uint64_t file_lo, const Bytes& meta,
                   const std::vector<Region>& abs, Bytes& dst, std::vector<std::pair<uint64_t, uint64_t>>& cover) {
  for (const Seg& g : segs) {
    require(g.src <= SEG_ZERO, "segment source unknown");
    require(inside(g.dst_off, g.len, dst.size()), "segment destination outside its buffer");
    cover.push_back({g.dst_off, g.len});
    const uint8_t* from = nullptr;
    if (g.src == SEG_FILE) {
      require(g.src_off >= file_lo && inside(g.src_off, g.len, file.size()), "file segment outside the file");
      from = file.data() + g.src_off;
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

static int parse_and_print(const Bytes& a, std::vector<AtzDesc>& d, uint64_t& origlen, uint64_t& residue) {
  origlen = residue = 0;
  const int rc = parse_atz(a.data(), a.size(), d, origlen, residue);
  std::printf("P %d %d %llu %zu\n", rc, a.size() > 3 ? a[3] : 0, (unsigned long long)origlen, rc ? (size_t)0 : d.size());
  if (rc) return rc;
  for (const AtzDesc& x : d)
    std::printf("D %llu %llu %llu %u %u %u %llu %llu %llu %llu\n", (unsigned long long)x.off, (unsigned long long)x.cl,
                (unsigned long long)x.il, x.c, x.w, x.m, (unsigned long long)x.nd, (unsigned long long)x.fd,
                (unsigned long long)x.k, (unsigned long long)x.ipos);
  return 0;
}

static int rebuild(const Bytes& a, const Bytes& outs, Bytes& orig) {
  std::vector<AtzDesc> d;
  uint64_t origlen, residue;
  if (int rc = parse_and_print(a, d, origlen, residue)) return rc;
  RecLayout L;
  if (int rc = plan_layout(a.data(), a.size(), d, origlen, residue, L)) return rc;
  const size_t ns = d.size();
  if (origlen > (1ull << 30) || L.slab > (1ull << 30)) die(2, "a file this large is not for this program");
  orig.assign(origlen, 0xEE);
  std::vector<std::pair<uint64_t, uint64_t>> cover, slab_cover;
  gather(L.gaps, a, residue, {}, {}, orig, cover);
  Bytes slab(L.slab, 0xEE);
  gather(L.payloads, a, 28, {}, {}, slab, slab_cover);
  check_cover(slab_cover, slab.size(), false);
  require(L.rec_off.size() == ns && L.loc.size() == ns && L.params.size() == ns, "layout tables of another size");
  for (size_t j = 0; j < ns; j++) {
    require(L.loc[j] % 256 == 0 && inside(L.loc[j], d[j].il, slab.size()), "payload outside the slab");
    require(!d[j].il || !std::memcmp(slab.data() + L.loc[j], a.data() + d[j].ipos, d[j].il), "payload bytes differ");
    const DeflSpec& s = L.params[j];
    std::printf("S %d %d %d %u %d %d %d %llu\n", s.level, s.window, s.memlevel, s.strategy, (int)s.raw, (int)s.gnu,
                (int)s.flush, (unsigned long long)(SLAB + L.loc[j]));
  }
  // the deflate outputs, in batches whose buffers are valid for their batch only
  size_t at = 0;
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
    if (int rc = plan_batch(a.data(), d, L, origlen, s0, s1, oa, ol, ORIG, B)) return rc;
    gather(B.segs, a, a.size(), {}, regions, orig, cover);   // (a batch copies nothing from the file)
    require(B.pat.size() == B.pval.size(), "patch lists of two sizes");
    for (size_t q = 0; q < B.pat.size(); q++) {
      require(B.pat[q] >= ORIG && B.pat[q] - ORIG < origlen, "patch outside the original");
      require(!q || B.pat[q] > B.pat[q - 1], "patch addresses not strictly ascending");
    }
    for (size_t q = 0; q < B.pat.size(); q++) orig[B.pat[q] - ORIG] = B.pval[q];
  }
  check_cover(cover, origlen, true);
  return 0;
}

static Bytes unhex(const std::string& s) {
  Bytes b;
  if (s == "-") return b;
  for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return b;
}

static int write_mode(const char* table, const char* orig_path, const char* out_path) {
  std::ifstream t(table);
  if (!t) die(2, std::string("cannot read ") + table);
  const Bytes file = slurp(orig_path);
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
  Bytes meta;
  std::vector<Seg> segs;
  uint64_t out = 0;
  const int rc = write_file(n, [&](size_t s) { return recs[s]; }, file.size(), meta, segs, out);
  std::printf("W %d %llu\n", rc, (unsigned long long)(rc ? 0 : out));
  if (rc) return rc;
  Bytes atz(out, 0xEE);
  std::vector<std::pair<uint64_t, uint64_t>> cover;
  gather(segs, file, 0, meta, regions, atz, cover);
  check_cover(cover, out, true);
  spill(out_path, atz);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "parse") {
    for (int i = 2; i < argc; i++) {
      std::vector<AtzDesc> d;
      uint64_t origlen, residue;
      parse_and_print(slurp(argv[i]), d, origlen, residue);
    }
  } else if (mode == "rebuild" && argc % 3 == 2) {
    for (int i = 2; i < argc; i += 3) {
      Bytes orig;
      const int rc = rebuild(slurp(argv[i]), slurp(argv[i + 1]), orig);
      std::printf("R %d\n", rc);
      if (!rc) spill(argv[i + 2], orig);
    }
  } else if (mode == "write" && argc == 5) {
    write_mode(argv[2], argv[3], argv[4]);
  } else {
    die(2, "usage: format_check parse ATZ... | rebuild (ATZ OUTS REBUILT)... | write TABLE ORIG ATZ");
  }
  return 0;
}
