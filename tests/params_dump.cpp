// Prints what antiz_amd/csrc/atz_params.h computes, for tests/test_params_cpu.py to compare with its models.
// Stand-alone: includes that header only, built with -fsanitize=address,undefined and run directly.
#include <cstdio>

#include "atz_params.h"

using namespace atz;

static void fields(const DeflSpec& s) {
  std::printf(" %d %d %d %u %d %d %d %d %d %d", s.level, s.window, s.memlevel, s.strategy, (int)s.raw, (int)s.gnu,
              (int)s.flush, s.table_memlevel(), (int)s.needs_tables(), (int)s.mode());
}

static void list(const char* tag, int a, unsigned b, int c, const std::vector<uint32_t>& l) {
  std::printf("%s %d %u %d :", tag, a, b, c);
  for (uint32_t e : l) std::printf(" %x", e);
  std::printf("\n");
  for (uint32_t e : l) {   // every entry: its parameters, and the word they write
    const DeflSpec s = DeflSpec::from_word(e);
    std::printf("E %x", e);
    fields(s);
    std::printf(" %x\n", s.word());
  }
}

int main() {
  for (int type = 0; type < 24; type++)
    for (unsigned mask = 0; mask < 16; mask += 2) {
      std::vector<uint32_t> l;
      strategy_list(l, type, mask);
      list("S", type, mask, 0, l);
    }
  for (int type = 24; type < 27; type++)
    for (unsigned dm = 0; dm < 2; dm++)
      for (int flush = 0; flush < 2; flush++) {
        std::vector<uint32_t> l;
        raw_list(l, type, dm, flush != 0);
        list("R", type, dm, flush, l);
      }
  // valid_desc: one line per (version, c), one character per (w, m)
  static const int W[21] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 0x80, 0x8E, 0x8F, 0xFF};
  for (int v = 1; v <= 6; v++)
    for (int c = 0; c < 256; c++) {
      std::printf("D %d %d ", v, c);
      for (int w : W)
        for (int m = 0; m <= 10; m++) std::putchar(valid_desc(v, (uint8_t)c, (uint8_t)w, (uint8_t)m) ? '1' : '0');
      std::printf("\n");
    }
  // every triple some version accepts: desc -> spec -> desc, spec -> word -> spec -> desc, the lowest version
  for (int c = 0; c < 256; c++)
    for (int w : W)
      for (int m = 0; m <= 10; m++) {
        if (!valid_desc(6, (uint8_t)c, (uint8_t)w, (uint8_t)m)) continue;
        bool st = false;
        const DeflSpec s = DeflSpec::from_desc((uint8_t)c, (uint8_t)w, (uint8_t)m, &st);
        const auto d = s.desc(st), d2 = DeflSpec::from_word(s.word()).desc(st);
        std::printf("X %d %d %d", c, w, m);
        fields(s);
        std::printf(" %d %d %d %d %d %d %d %x %d\n", (int)st, d[0], d[1], d[2], d2[0], d2[1], d2[2], s.word(), s.min_version(st));
      }
  // valid_api: every field in and just outside its range, every value of bits 24-31
  static const unsigned L[5] = {0, 1, 9, 10, 255}, WW[6] = {7, 8, 9, 14, 15, 16}, M[5] = {0, 1, 8, 9, 10};
  for (int ex = 0; ex < 2; ex++)
    for (unsigned hi = 0; hi < 256; hi++)
      for (unsigned l : L)
        for (unsigned w : WW)
          for (unsigned m : M) {
            const uint32_t p = (hi << 24) | (l << 16) | (w << 8) | m;
            DeflSpec s;
            if (!valid_api(p, ex != 0, &s)) { std::printf("A %d %x 0\n", ex, p); continue; }
            const auto d = s.desc();
            std::printf("A %d %x 1", ex, p);
            fields(s);   // then: its word, that word read and written again, its descriptor
            std::printf(" %x %x %d %d %d\n", s.word(), DeflSpec::from_word(s.word()).word(), d[0], d[1], d[2]);
          }
  return 0;
}
