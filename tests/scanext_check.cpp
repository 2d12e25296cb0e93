// scanext_check -- a host driver of antiz_amd/csrc/atz_scanext.h for tests/test_scanext_cpu.py (stand-alone: it
// includes only that header; built with -fsanitize=address,undefined).  The file lies in a heap buffer of exactly its
// length, so a read past its end is ASan's to report.
//   scanext_check raw|stitch|probe|seg jobs|accept FILE INPUT
// INPUT (text): cap C | pos N, N positions | recs N, N x (offset comp_len infl_len type flags arena_off stitch pk) |
//               res N, N x (status err consumed produced)
// pos: the list kernel's output (raw, stitch: position << 5 | kind); recs: the records made before (-1: ~0); cap: the
// record vector's capacity (-1: the records and one per position); res (accept): one result per job, which gets
// arena_off = 65536 x its index.
// Output: "rc R" (the step's return code; nothing follows one that is not 0), then
//   jobs:   raw C p d limit kind hint know_c know_u csize usize | stitch C at total p0 pk type, P off len, B bytes,
//           G src src_off dst_off len | seg E rec b0 b1 j0 j1 | all J in_off in_len out_off out_cap
//   accept: K the records the step keeps (seg: none), R the records after it, T off len the piece lists,
//           N accepted kept (probe) / N chains made (seg); a record: offset comp_len infl_len type flags arena_off
//           noshort mhint stitch p0 pk
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <sstream>
#include <string>

#include "atz_scanext.h"

using namespace atz;

[[noreturn]] static void die(const std::string& why) {
  std::fprintf(stderr, "scanext_check: %s\n", why.c_str());
  std::exit(2);
}
static long long ll(uint64_t v) { return (long long)v; }
static void print_jobs(const std::vector<InfJob>& jobs) {
  for (const InfJob& j : jobs) std::printf("J %lld %lld %lld %lld\n", ll(j.in_off), ll(j.in_len), ll(j.out_off), ll(j.out_cap));
}
static void print_recs(char tag, const std::vector<Rec>& recs) {
  for (const Rec& r : recs)
    std::printf("%c %lld %lld %lld %d %u %lld %d %d %lld %u %u\n", tag, ll(r.offset), ll(r.comp_len), ll(r.infl_len), r.type,
                r.flags, ll(r.arena_off), (int)r.noshort, (int)r.mhint, ll(r.stitch), r.p0, r.pk);
}
static int fail(int rc) { std::printf("rc %d\n", rc); return 0; }

int main(int argc, char** argv) {
  if (argc != 5) die("usage: scanext_check raw|stitch|probe|seg jobs|accept FILE INPUT");
  const std::string ext = argv[1], cmd = argv[2];
  const bool accept = cmd == "accept";
  if (!accept && cmd != "jobs") die("unknown command " + cmd);

  std::ifstream f(argv[3], std::ios::binary);
  if (!f) die(std::string("cannot read ") + argv[3]);
  const std::string bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const uint64_t n = bytes.size();
  std::unique_ptr<uint8_t[]> file(new uint8_t[n]);
  std::copy(bytes.begin(), bytes.end(), file.get());
  const uint8_t* h = file.get();

  std::ifstream in(argv[4]);
  if (!in) die(std::string("cannot read ") + argv[4]);
  long long cap = -1;
  std::vector<uint64_t> pos;
  std::vector<Rec> prior;
  std::vector<InfRes> res;
  std::string key;
  while (in >> key) {
    long long cnt = 0, v[8];
    in >> cnt;
    if (key == "cap") { cap = cnt; continue; }
    for (long long k = 0; k < cnt; k++) {
      const int nf = key == "pos" ? 1 : key == "recs" ? 8 : key == "res" ? 4 : 0;
      if (!nf) die("unknown key " + key);
      for (int q = 0; q < nf; q++) in >> v[q];
      if (key == "pos") pos.push_back((uint64_t)v[0]);
      if (key == "recs") {
        Rec r{(uint64_t)v[0], (uint64_t)v[1], (uint64_t)v[2], (int)v[3], (uint32_t)v[4], (uint64_t)v[5]};
        r.stitch = (uint64_t)v[6]; r.pk = (uint32_t)v[7];
        prior.push_back(r);
      }
      if (key == "res") res.push_back(InfRes{(uint32_t)v[0], (uint32_t)v[1], (uint64_t)v[2], (uint64_t)v[3], 65536ull * (uint64_t)k});
    }
  }
  if (!in.eof()) die("malformed input");
  std::vector<Rec> recs;
  recs.reserve(cap >= 0 ? (size_t)cap : prior.size() + pos.size());
  recs.assign(prior.begin(), prior.end());

  std::vector<InfJob> jobs;
  std::vector<Rec> kept;
  std::vector<uint64_t> st_off, st_len;
  size_t accepted = 0;
  if (ext == "raw") {
    std::vector<RawCand> cands;
    if (int r = raw_candidates(h, n, pos, cands)) return fail(r);
    raw_jobs(cands, jobs);
    if (!accept) {
      std::printf("rc 0\n");
      for (const RawCand& c : cands)
        std::printf("C %lld %lld %lld %d %d %d %d %lld %lld\n", ll(c.p), ll(c.d), ll(c.limit), c.kind, c.hint, (int)c.know_c,
                    (int)c.know_u, ll(c.csize), ll(c.usize));
      print_jobs(jobs);
      return 0;
    }
    if (int r = raw_accept(h, cands, res, recs, kept)) return fail(r);
  } else if (ext == "stitch") {
    StitchPlan P;
    std::vector<Seg> segs;
    if (int r = stitch_candidates(h, n, pos, P)) return fail(r);
    stitch_jobs(P, segs, jobs);
    if (!accept) {
      std::printf("rc 0\n");
      for (const StitchCand& c : P.cands) std::printf("C %lld %lld %u %u %d\n", ll(c.at), ll(c.total), c.p0, c.pk, c.type);
      for (size_t q = 0; q < P.off.size(); q++) std::printf("P %lld %lld\n", ll(P.off[q]), ll(P.len[q]));
      std::printf("B %lld\n", ll(P.bytes));
      for (const Seg& g : segs) std::printf("G %u %lld %lld %lld\n", g.src, ll(g.src_off), ll(g.dst_off), ll(g.len));
      print_jobs(jobs);
      return 0;
    }
    if (int r = stitch_accept(P, res, recs, st_off, st_len, kept)) return fail(r);
  } else if (ext == "probe") {
    if (int r = probe_jobs(pos, n, recs, jobs)) return fail(r);
    if (!accept) {
      std::printf("rc 0\n");
      print_jobs(jobs);
      return 0;
    }
    if (int r = probe_accept(jobs, res, recs, kept, accepted)) return fail(r);
  } else if (ext == "seg") {
    std::vector<SegElig> el;
    if (int r = seg_jobs(h, n, recs, pos, el, jobs)) return fail(r);
    if (!accept) {
      std::printf("rc 0\n");
      for (const SegElig& e : el) std::printf("E %zu %lld %lld %zu %zu\n", e.rec, ll(e.b0), ll(e.b1), e.j0, e.j1);
      print_jobs(jobs);
      return 0;
    }
    std::vector<Rec> merged;
    size_t chains = 0, made = 0;
    if (int r = seg_accept(h, recs, el, jobs, res, merged, chains, made)) return fail(r);
    if (chains)
      if (int r = put_records(recs, merged)) return fail(r);
    std::printf("rc 0\nN %zu %zu\n", chains, made);
    print_recs('R', recs);
    return 0;
  } else {
    die("unknown extension " + ext);
  }
  if (int r = splice(recs, kept)) return fail(r);
  std::printf("rc 0\n");
  if (ext == "probe") std::printf("N %zu %zu\n", accepted, kept.size());
  print_recs('K', kept);
  print_recs('R', recs);
  for (size_t q = 0; q < st_off.size(); q++) std::printf("T %lld %lld\n", ll(st_off[q]), ll(st_len[q]));
  return 0;
}
