// atz_accel.cpp -- libatz_accel.so: host orchestration + C ABI (include/atz_accel.h) for the
// MI355X zlib-stream precompressor.  Unity build: the HIP kernels are compiled into this TU.
//
// Phase 1 (scan)  : k_find_headers over the whole file in HBM, one k_inflate launch over every
//                   candidate of every chunk, the reference's greedy per-chunk selection
//                   (ZBuffSearcher::operator(), main.cpp:205-246) replayed on the host from the
//                   results, boundary continuations (main.cpp:207-217) batched speculatively,
//                   then one k_inflate launch that writes every recorded stream's inflated bytes
//                   into a packed HBM buffer (the reference re-inflates each stream in Phase 3
//                   and again in Phase 4; here they stay resident).
// Phase 3 (sweep) : rounds; round r evaluates the r-th trial of every stream that has not stopped
//                   (one wavefront per trial, k_trial_{stored,fast,slow}), so the reference's
//                   ordered first-improving-within-tolerance rule (main.cpp:685-700, 746-754) is
//                   applied exactly, per stream, between rounds.  Chain links per (stream,memLevel)
//                   are built on demand by k_chains and cached in HBM.
// Phase 4 (write) : ATZ1 (main.cpp:764-834) assembled in HBM by k_gather from the resident
//                   inflated payloads and the original file.
#include "k_inflate.hip"
#include "k_deflate.hip"

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <memory>
#include <new>
#include <stdexcept>
#include <atomic>
#include <thread>
#include <condition_variable>
#include <mutex>
#include <functional>
#include <unordered_map>
#include <vector>
#include <dlfcn.h>
#include <signal.h>
#include <sys/time.h>
#include <ucontext.h>

#include "../../include/atz_accel.h"
#include "atz_params.h"
#include "atz_format.h"
#include "atz_scanext.h"

using namespace atz;

namespace {

// (Seg, the k_gather segment: atz_format.h)
__global__ __launch_bounds__(256) void k_gather(const uint8_t* __restrict__ meta, const uint8_t* __restrict__ infl,
                                               const uint8_t* __restrict__ file, uint8_t* __restrict__ dst,
                                               const Seg* __restrict__ segs, uint32_t nseg) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (uint32_t s = blockIdx.x * 4 + wave; s < nseg; s += gridDim.x * 4) {
    const Seg g = segs[s];
    uint8_t* d = dst + g.dst_off;
    if (g.src == SEG_ZERO) {
      for (uint64_t k = lane; k < g.len; k += 64) d[k] = 0;
      continue;
    }
    const uint8_t* src = (g.src == SEG_META ? meta : g.src == SEG_ADDR ? infl : file) + g.src_off;
    // head bytes up to a 4-byte aligned destination, then aligned dword stores whose 4 source bytes
    // come from two aligned dword loads joined with v_alignbyte (any source alignment), 4 per lane in
    // flight, then the tail bytes.  Reads stay inside the source's 4-byte words that hold segment bytes.
    const uint64_t head = ((4 - ((uintptr_t)d & 3)) & 3) < g.len ? ((4 - ((uintptr_t)d & 3)) & 3) : g.len;
    if (lane < head) d[lane] = src[lane];
    const uint64_t nw = (g.len - head) >> 2;
    const uint8_t* sb = src + head;
    uint32_t* dw = (uint32_t*)(d + head);
    const uint32_t sh = (uint32_t)((uintptr_t)sb & 3);
    const uint32_t* sw = (const uint32_t*)(sb - sh);
    if (sh == 0) {
      uint64_t k = lane;
      for (; k + 192 < nw; k += 256) {
        const uint32_t a0 = sw[k], a1 = sw[k + 64], a2 = sw[k + 128], a3 = sw[k + 192];
        dw[k] = a0; dw[k + 64] = a1; dw[k + 128] = a2; dw[k + 192] = a3;
      }
      for (; k < nw; k += 64) dw[k] = sw[k];
    } else {
      // word k takes source bytes [4k, 4k + 4): aligned words k and k + 1 (the last of which holds a
      // segment byte whenever it is read: 4k + 3 < 4 nw <= len - head)
      uint64_t k = lane;
      for (; k + 192 < nw; k += 256) {
        uint32_t lo[4], hi[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { lo[u] = sw[k + 64 * u]; hi[u] = sw[k + 64 * u + 1]; }
#pragma unroll
        for (int u = 0; u < 4; u++) dw[k + 64 * u] = __builtin_amdgcn_alignbyte(hi[u], lo[u], sh);
      }
      for (; k < nw; k += 64) dw[k] = __builtin_amdgcn_alignbyte(sw[k + 1], sw[k], sh);
    }
    const uint64_t t0 = head + 4 * nw;
    if (t0 + lane < g.len) d[t0 + lane] = src[t0 + lane];
  }
}

// Adler-32 (Z/adler32.c:65) of each stream at absolute address addr[j]: lane l sums its contiguous
// share, the shares are joined in order with adler32_combine's arithmetic (Z/adler32.c:139-167).
__global__ __launch_bounds__(64) void k_adler32(const uint64_t* __restrict__ addr, const uint64_t* __restrict__ len,
                                               uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t j = blockIdx.x;
  if (j >= n) return;
  const uint32_t lane = threadIdx.x;
  constexpr uint32_t BASE = 65521;
  const uint8_t* p = (const uint8_t*)(uintptr_t)addr[j];
  const uint64_t L = len[j], share = (L + 63) / 64;
  const uint64_t b0 = share * lane < L ? share * lane : L, b1 = b0 + share < L ? b0 + share : L;
  uint32_t a = 1, b = 0;
  for (uint64_t i = b0; i < b1;) {
    const uint64_t e = b1 - i < 5552 ? b1 : i + 5552;   // NMAX: no overflow before the reduction
    for (; i < e; i++) { a += p[i]; b += a; }
    a %= BASE; b %= BASE;
  }
  // join the 64 shares in lane order: adler(x||y) from adler(x), adler(y), len(y)
  uint32_t acc = 1;   // adler of the empty prefix
  for (int l = 0; l < 64; l++) {
    const uint32_t ad2 = (uint32_t)__shfl((int)((b << 16) | a), l, 64);
    const uint64_t ln2 = (uint64_t)__shfl((int)(uint32_t)(b1 - b0), l, 64);
    const uint32_t rem = (uint32_t)(ln2 % BASE);
    uint32_t sum1 = acc & 0xffff;
    uint32_t sum2 = (uint32_t)(((uint64_t)rem * sum1) % BASE);
    sum1 += (ad2 & 0xffff) + BASE - 1;
    sum2 += ((acc >> 16) & 0xffff) + ((ad2 >> 16) & 0xffff) + BASE - rem;
    if (sum1 >= BASE) sum1 -= BASE;
    if (sum1 >= BASE) sum1 -= BASE;
    if (sum2 >= ((uint32_t)BASE << 1)) sum2 -= ((uint32_t)BASE << 1);
    if (sum2 >= BASE) sum2 -= BASE;
    acc = sum1 | (sum2 << 16);
  }
  if (lane == 0) out[j] = acc;
}

// diff bytes of reconstructed streams (main.cpp:916-926): one byte per thread, distinct addresses
__global__ __launch_bounds__(256) void k_patch(const uint64_t* __restrict__ at, const uint8_t* __restrict__ val, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) *(uint8_t*)(uintptr_t)at[i] = val[i];
}

// Mismatch list of a winning trial (main.cpp:699-714): positions i < min(L, C_s) with out[i] != orig[i],
// then L..C_s-1 if the recompressed stream is shorter.
struct DiffJob {
  uint64_t out_off, out_len, orig_off, comp_len, dst;  // dst: index into pos/val arrays
  uint64_t cap;                                       // entries reserved
};
__global__ __launch_bounds__(64) void k_diffs(const uint8_t* __restrict__ out, const uint8_t* __restrict__ file,
                                             const DiffJob* __restrict__ jobs, uint32_t* __restrict__ pos,
                                             uint8_t* __restrict__ val, uint64_t* __restrict__ count, uint32_t n) {
  const uint32_t j = blockIdx.x;
  if (j >= n) return;
  const int lane = threadIdx.x;
  const DiffJob d = jobs[j];
  const uint8_t* o = out + d.out_off;
  const uint8_t* f = file + d.orig_off;
  uint64_t sm = d.out_len < d.comp_len ? d.out_len : d.comp_len;
  uint64_t k = 0;
  uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (uint64_t b = 0; b < d.comp_len; b += 64) {
    uint64_t i = b + lane;
    bool m = false;
    uint8_t v = 0;
    if (i < d.comp_len) {
      v = f[i];
      m = i < sm ? o[i] != v : true;
    }
    uint64_t bal = __ballot(m);
    if (m) {
      uint64_t at = k + __popcll(bal & lt);
      if (at < d.cap) { pos[d.dst + at] = (uint32_t)i; val[d.dst + at] = v; }
    }
    k += __popcll(bal);
  }
  if (lane == 0) count[j] = k;
}

#define HIPCHK(x)                                                     \
  do {                                                                \
    hipError_t e_ = (x);                                              \
    if (e_ != hipSuccess) {                                           \
      std::fprintf(stderr, "atz: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      return ATZ_E_HIP;                                               \
    }                                                                 \
  } while (0)

// Device bytes the library holds in this process (every DBuf: the contexts' buffers, their pipes' scratch,
// the arenas' chunks), and the peak since the last dev_mark_call(): atz_stats_t dev_bytes_*.
struct DevAcct {
  std::atomic<uint64_t> cur{0}, peak{0};
  void add(uint64_t n) {
    const uint64_t v = cur.fetch_add(n) + n;
    uint64_t p = peak.load();
    while (v > p && !peak.compare_exchange_weak(p, v)) {}
  }
  void sub(uint64_t n) { cur.fetch_sub(n); }
  // diagnostics (ATZ_TIMING): allocations / frees and the host time they took (a hipFree waits for the device)
  std::atomic<uint64_t> n_alloc{0}, n_free{0}, alloc_us{0};
};
DevAcct g_dev;
void dev_mark_call() { g_dev.peak.store(g_dev.cur.load()); }

// ATZ_HOSTPROF=<file> (diagnostics): wall-clock sampling of the call's host threads (the caller's and
// the sweep's pipe threads register themselves): a sampler thread signals each one every 100 us and the
// handler records the interrupted instruction (a blocked thread's is its system call).  Appended to
// <file> as "count thread object offset symbol" lines (tools/hostprof.py resolves them).
struct HostProf {
  static constexpr size_t MAXS = 1u << 22;
  static constexpr int MAXT = 64;
  static std::atomic<size_t>& n() { static std::atomic<size_t> v{0}; return v; }
  static uint64_t* pcs() { static uint64_t* b = new uint64_t[MAXS]; return b; }
  static std::atomic<int>& nthr() { static std::atomic<int> v{0}; return v; }
  static pthread_t* thr() { static pthread_t t[MAXT]; return t; }
  static std::atomic<bool>& on() { static std::atomic<bool> v{false}; return v; }
  static int& my_slot() { thread_local int s = -1; return s; }
  static std::mutex& mu() { static std::mutex m; return m; }   // held while signalling: leave() waits for it
  static bool* alive() { static bool a[MAXT]; return a; }
  static void on_sig(int, siginfo_t*, void* uc) {
    const int slot = my_slot();
    if (slot < 0) return;
    const size_t i = n().fetch_add(1, std::memory_order_relaxed);
    if (i < MAXS) pcs()[i] = (uint64_t)((ucontext_t*)uc)->uc_mcontext.gregs[REG_RIP] | ((uint64_t)slot << 56);
  }
  static void enroll() {   // the calling thread is sampled while a profile runs (until leave())
    if (!on().load() || my_slot() >= 0) return;
    std::lock_guard<std::mutex> lk(mu());
    const int k = nthr().load();
    if (k >= MAXT) return;
    thr()[k] = pthread_self();
    alive()[k] = true;
    my_slot() = k;
    nthr().store(k + 1);
  }
  static void leave() {
    if (my_slot() < 0) return;
    std::lock_guard<std::mutex> lk(mu());
    alive()[my_slot()] = false;
    my_slot() = -1;
  }
  struct Enroll { Enroll() { enroll(); } ~Enroll() { leave(); } };
  const char* path = nullptr;
  std::thread sampler;
  std::atomic<bool> stop{false};
  HostProf() {
    path = std::getenv("ATZ_HOSTPROF");
    if (!path || !*path) { path = nullptr; return; }
    pcs();
    n().store(0);
    struct sigaction sa{};
    sa.sa_sigaction = on_sig;
    sa.sa_flags = SA_SIGINFO | SA_RESTART;
    sigemptyset(&sa.sa_mask);
    sigaction(SIGPROF, &sa, nullptr);
    {
      std::lock_guard<std::mutex> lk(mu());
      nthr().store(0);
    }
    on().store(true);
    enroll();
    sampler = std::thread([this] {
      while (!stop.load()) {
        {
          std::lock_guard<std::mutex> lk(mu());
          const int k = std::min(nthr().load(), MAXT);
          for (int i = 0; i < k; i++)
            if (alive()[i]) pthread_kill(thr()[i], SIGPROF);
        }
        std::this_thread::sleep_for(std::chrono::microseconds(100));
      }
    });
  }
  ~HostProf() {
    if (!path) return;
    stop.store(true);
    sampler.join();
    on().store(false);
    const size_t cnt = std::min(n().load(), MAXS);
    std::unordered_map<uint64_t, uint64_t> hist;
    for (size_t i = 0; i < cnt; i++) hist[pcs()[i]]++;
    FILE* f = std::fopen(path, "a");
    if (f) {
      std::fprintf(f, "# call: %zu samples, %d threads\n", cnt, nthr().load());
      for (const auto& kv : hist) {
        const uint64_t pc = kv.first & ((1ull << 56) - 1);
        Dl_info di{};
        if (dladdr((void*)(uintptr_t)pc, &di) && di.dli_fname)
          std::fprintf(f, "%llu %d %s 0x%llx %s\n", (unsigned long long)kv.second, (int)(kv.first >> 56), di.dli_fname,
                       (unsigned long long)(pc - (uint64_t)(uintptr_t)di.dli_fbase), di.dli_sname ? di.dli_sname : "?");
        else
          std::fprintf(f, "%llu %d ? 0x%llx ?\n", (unsigned long long)kv.second, (int)(kv.first >> 56), (unsigned long long)pc);
      }
      std::fclose(f);
    }
    leave();
    std::lock_guard<std::mutex> lk(mu());
    nthr().store(0);
  }
};

struct DBuf {              // device buffer, freed with its owner (atz_close deletes the context)
  void* p = nullptr;
  size_t n = 0;
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  ~DBuf() { release(); }
  int reserve(size_t need) {
    if (need <= n) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    release();
    size_t cap = need + need / 4 + 65536;
    const hipError_t e = hipMalloc(&p, cap);
    g_dev.n_alloc++;
    g_dev.alloc_us += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    if (e != hipSuccess) { p = nullptr; return ATZ_E_NOMEM; }
    n = cap;
    g_dev.add(n);
    return 0;
  }
  void release() {
    if (p) { hipFree(p); g_dev.sub(n); g_dev.n_free++; }
    p = nullptr;
    n = 0;
  }
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct PinBuf {            // pinned host buffer that kernels write directly
  void* p = nullptr;
  size_t n = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { if (p) (void)hipHostFree(p); }
  int reserve(size_t need) {
    if (need <= n) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    if (p) { (void)hipHostFree(p); g_dev.n_free++; }
    p = nullptr;
    n = 0;
    const hipError_t e = hipHostMalloc(&p, need, hipHostMallocDefault);
    g_dev.n_alloc++;
    g_dev.alloc_us += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    if (e != hipSuccess) return ATZ_E_NOMEM;
    n = need;
    return 0;
  }
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// (Rec, a record of the scan: atz_scanext.h)
struct StreamState {
  // sweep
  const std::vector<uint32_t>* list = nullptr;   // packed (c<<16)|(w<<8)|m: the header type's shared list
  uint32_t idx = 0;
  uint32_t phase = 0;             // 0 = list A, 1 = list B, 2 = done
  uint8_t c = 9, w = 15, m = 9;   // streamOffset ctor defaults (ATZData.h:51-53)
  uint64_t ident = 0;
  int64_t first_diff = -1;
  std::vector<uint32_t> rawdiff;  // raw positions of the current best
  std::vector<uint8_t> diffval;
  uint32_t trials = 0;
  int32_t rp = -1;                // symbol-replay entries (levels 1-9) in the context's rp_pool
  // their states at a glance (bit L: level L's entry is saved / has its saver in flight; rp_win[L]: that
  // sequence's window), so that planning reads rp_pool only where an entry is used
  uint16_t rp_saved = 0, rp_busy = 0;
  uint8_t rp_win[10] = {};
  bool recomp = false;
  // levels 7-9 already run budget-free at (window, memLevel): level, longest PL a lazy read improved,
  // longest length read (cross-level duplicates, see level_dups)
  std::vector<std::array<uint16_t, 5>> xl;   // {window, memLevel, level, imp, len}
};


uint64_t bound(uint64_t n, int w, int m) {  // deflateBound (Z/deflate.c:566-621), zlib wrapper
  uint64_t complen = n + ((n + 7) >> 3) + ((n + 63) >> 6) + 5;
  if (w != 15 || m + 7 != 15) return complen + 6;
  return n + (n >> 12) + (n >> 14) + (n >> 25) + 13 - 6 + 6;
}

double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// trees.c tr_static_init (Z/trees.c:232-330)
void make_tables(DeflTables& T) {
  static const int xlb[29] = {0,0,0,0,0,0,0,0,1,1,1,1,2,2,2,2,3,3,3,3,4,4,4,4,5,5,5,5,0};
  static const int xdb[30] = {0,0,0,0,1,1,2,2,3,3,4,4,5,5,6,6,7,7,8,8,9,9,10,10,11,11,12,12,13,13};
  std::memset(&T, 0, sizeof(T));
  int len = 0, code;
  for (code = 0; code < 28; code++) {
    T.lbase[code] = (uint16_t)len;
    for (int k = 0; k < (1 << xlb[code]); k++) T.lcode[len++] = (uint8_t)code;
  }
  T.lbase[28] = 0;
  T.lcode[255] = 28;
  int dist = 0;
  for (code = 0; code < 16; code++) {
    T.dbase[code] = (uint16_t)dist;
    for (int k = 0; k < (1 << xdb[code]); k++) T.dcode[dist++] = (uint8_t)code;
  }
  dist >>= 7;
  for (; code < 30; code++) {
    T.dbase[code] = (uint16_t)(dist << 7);
    for (int k = 0; k < (1 << (xdb[code] - 7)); k++) T.dcode[256 + dist++] = (uint8_t)code;
  }
  uint16_t blc[16] = {0};
  for (int n = 0; n < 288; n++) {
    T.st_llen[n] = n < 144 ? 8 : n < 256 ? 9 : n < 280 ? 7 : 8;
    blc[T.st_llen[n]]++;
  }
  uint16_t next[16];
  uint32_t c = 0;
  for (int b = 1; b <= 15; b++) { c = (c + blc[b - 1]) << 1; next[b] = (uint16_t)c; }
  auto rev = [](uint32_t v, int l) { uint32_t r = 0; for (int i = 0; i < l; i++) { r = (r << 1) | (v & 1); v >>= 1; } return r; };
  for (int n = 0; n < 288; n++) T.st_lcode[n] = (uint16_t)rev(next[T.st_llen[n]]++, T.st_llen[n]);
  for (int n = 0; n < 30; n++) { T.st_dlen[n] = 5; T.st_dcode[n] = (uint16_t)rev((uint32_t)n, 5); }
}

// Stream bytes are addressed by absolute device addresses (infl_off / StreamDev.infl_off /
// ChainJob.infl_off / MatchJob.infl_off), so every kernel takes a null inflated-buffer base: the
// records of one file may live in several allocations (one per scan piece).
const uint8_t* const INFL_BASE = nullptr;
// Hash-bucket tables likewise: chain_off fields hold a table's absolute address / 4 (DevArena / a pipe's
// round-local d_chains), so the kernels take a null base.
uint32_t* const CHAIN_BASE = nullptr;

}  // namespace

struct KTimer {   // HIP events bracketing kernel launches on the library stream
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  std::vector<int> kind;
  std::vector<hipEvent_t> pool;
  double gnu_ms = 0;   // kind 5: the GNU-family trial kernels' share of k_trial_ms (ATZ_TIMING's raw pass line)
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
  }
};

// A saved symbol sequence of (stream, level): the first trial at that level whose chain walks cannot
// reach their budget saves it; later ones at that level replay it (see plan_replay, trial_body).
struct RpEntry {
  uint32_t reads_max = 0;   // the saver's TrialRes::reads_max (its whole parse)
  uint64_t addr = 0;      // device address of the arena slot (n + 64 symbols, then n table entries for slow levels)
  uint64_t tab = 0;       // its match-table part (0: none)
  uint32_t nsym = 0, flags = 0;
  uint8_t state = 0;      // 0 free (addr may hold a reusable slot), 1 a saving trial in flight, 2 saved
  uint8_t window = 0;
  uint8_t memlevel = 0;   // the saver's
};
// Device memory in 1 GiB chunks (allocated on demand, kept across sweeps), handed out by a bump
// pointer that each sweep resets: the context's hash-bucket cache and its saved symbol sequences.
// Shared by the sweep's pipes (a stream's tables, built by whichever pipe ran its step, are read by
// the next one), hence the lock; addresses are absolute.  Sizes are rounded to 4 KiB classes, and a
// released block (a finished stream's bucket tables: release_tables) serves the next request of its class.
struct DevArena {
  static constexpr uint64_t CHUNK = 1ull << 30;
  std::mutex mu;
  std::vector<std::unique_ptr<DBuf>> chunks;
  std::vector<std::pair<uint64_t, uint64_t>> span;   // [lo, hi) of each chunk (holds() without the lock's allocator state)
  std::unordered_map<uint64_t, std::vector<uint64_t>> freel;   // size class -> released addresses
  size_t cur = 0;
  uint64_t used = 0, total = 0, cap = 0;   // bytes in chunks[cur]; bytes handed out this sweep; limit
  uint64_t reused = 0;                     // bytes served from released blocks this sweep
  static uint64_t cls(uint64_t bytes) { return (bytes + 4095) & ~4095ull; }
  void reset(uint64_t cap_) {
    std::lock_guard<std::mutex> lk(mu);
    cur = 0; used = 0; total = 0; cap = cap_; reused = 0;
    freel.clear();
  }
  void release(uint64_t a, uint64_t bytes) {
    std::lock_guard<std::mutex> lk(mu);
    freel[cls(bytes)].push_back(a);
  }
  uint64_t alloc(uint64_t bytes) {   // device address (256-byte aligned), 0: none (cap reached, no memory)
    bytes = cls(bytes);
    std::lock_guard<std::mutex> lk(mu);
    auto it = freel.find(bytes);
    if (it != freel.end() && !it->second.empty()) {
      const uint64_t a = it->second.back();
      it->second.pop_back();
      reused += bytes;
      return a;
    }
    if (total + bytes > cap) return 0;
    while (cur < chunks.size() && used + bytes > chunks[cur]->n) { cur++; used = 0; }
    if (cur == chunks.size()) {
      auto b = std::make_unique<DBuf>();
      if (b->reserve(std::max(CHUNK, bytes)) != 0) { (void)hipGetLastError(); return 0; }
      span.push_back({(uint64_t)(uintptr_t)b->p, (uint64_t)(uintptr_t)b->p + b->n});
      chunks.push_back(std::move(b));
      used = 0;
    }
    const uint64_t a = (uint64_t)(uintptr_t)chunks[cur]->p + used;
    used += bytes;
    total += bytes;
    return a;
  }
  bool holds(uint64_t a, uint64_t len) {   // [a, a + len) inside one chunk
    std::lock_guard<std::mutex> lk(mu);
    for (const auto& s : span)
      if (a >= s.first && a + len <= s.second) return true;
    return false;
  }
};
struct ChainBufs {   // bucket-build job lists and scratch (one set per HIP stream that builds)
  DBuf d_cjobs, d_cjobs2, d_cjobs3, d_heads, d_heads2;
};
// One HIP stream of sweep work with its own buffers, kernel timers and counters.  The sweep runs
// several pipes at once (one host thread each, taking batches of streams from the sweep's queues), so
// one pipe's launch tails, host gaps and small launches overlap another's work.
struct Pipe {
  hipStream_t st = nullptr;
  KTimer kt;
  atz_stats_t stats{};
  DBuf d_trials, d_tres, d_out, d_syms, d_R, d_mjobs, d_diffjobs, d_diffpos, d_diffval, d_diffcnt, d_djobs;
  // speculative rounds: per stream, the lowest place in the round of a trial that stops it
  // (SweepArgs::stopj); stopj_cur is the round's (null: no flag)
  DBuf d_stopj;
  uint32_t* stopj_cur = nullptr;
  uint32_t mw_cap = 2;   // multi-wave trials up to this memLevel (mw_cap_for, set per round)
  // round-local bucket tables (the context's cache is full): one buffer per ensure_chains call of the
  // round (a later call must not move an earlier call's tables), kept for the next rounds' reuse
  std::vector<std::unique_ptr<DBuf>> d_chains;
  size_t chains_next = 0;
  ChainBufs cb;
  // pinned staging for the pipe's uploads (a pageable hipMemcpyAsync returns only once the stream has
  // reached it, which would hold the host thread behind every kernel enqueued before it): a bump
  // allocator that pipe_sync resets, every copy from it being complete then
  PinBuf stage;
  size_t stage_used = 0;
  // match tables of the round: d_R regions handed out in order (Round::plan reserves the round's bound)
  uint64_t r_next = 0;
  hipEvent_t ev_built = nullptr;   // after a round's direct bucket builds (their depths: Round::plan)

  // a second stream that stays idle: it only shifts how the process's GPU_MAX_HW_QUEUES (4) hardware
  // queues are shared by the pipes' streams (two pipes then share a queue, which measured faster
  // than every pipe on its own queue: DESIGN.md s3.6)
  hipStream_t pst = nullptr;
  // (stream, memLevel) pairs whose tables this round built in d_chains because the context's bucket
  // cache was full: forgotten at the round's end
  std::vector<std::pair<uint32_t, int>> tmp_chains;
  // diagnostics (ATZ_TIMING): bucket builds, and per stream the memLevels a table-reading trial used
  uint64_t diag_builds = 0;
  std::vector<std::pair<uint32_t, uint32_t>> diag_rt;   // ATZ_TIMING >= 3: every launched trial's realtime span
  std::vector<uint64_t> diag_path;   // ATZ_TIMING >= 3: per stream, its trials' summed realtime spans (10 ns)
  std::vector<uint32_t> diag_ntr;    //   and their number
  std::vector<uint16_t> diag_need;
  std::vector<uint32_t> slot;   // per stream of the current round: its index in the round's batch
  int id = 0;
  // diagnostics (ATZ_TIMING): host phase times, per trial kind x level counters; time in HIP copy calls
  // (host -> device uploads and result downloads) and in stream synchronisations
  double t_list = 0, t_chains = 0, t_trials = 0, t_apply = 0, t_copy = 0, t_sync = 0;
  uint64_t n_copy = 0, n_sync = 0;
  // host time per phase of a round (lap), and the part of it spent waiting in copies / synchronisations
  static constexpr int NPH = 13;
  double ph[NPH] = {}, ph_wait[NPH] = {};
  std::chrono::steady_clock::time_point lap_t;
  double lap_w = 0;
  void lap_start() { lap_t = std::chrono::steady_clock::now(); lap_w = t_copy + t_sync; }
  void lap(int i) {
    const auto n = std::chrono::steady_clock::now();
    ph[i] += std::chrono::duration<double, std::milli>(n - lap_t).count();
    ph_wait[i] += t_copy + t_sync - lap_w;
    lap_t = n;
    lap_w = t_copy + t_sync;
  }
  uint64_t kind[3][10][14] = {};
  ~Pipe() {
    if (ev_built) hipEventDestroy(ev_built);
    if (pst) { hipStreamSynchronize(pst); hipStreamDestroy(pst); }
    if (st) { hipStreamSynchronize(st); hipStreamDestroy(st); }
    for (hipEvent_t e : kt.pool) hipEventDestroy(e);
  }
};

// Trials of one launch group, kept between their first pass and their reruns: tr[k] (k = 0 stored,
// 1 fast, 2 slow levels) in launch order (LPT, see trials_order), perm[k][q] = the caller's index of
// tr[k][q], res[k] in launch order.  Match tables are built for a prefix of each trial's positions; a
// trial that parses past it stops with TR_NEED_R, and trials_rerun completes its table and runs it
// again.
struct TrialSet {
  std::vector<Trial> tr[3];
  std::vector<uint32_t> perm[3];
  std::vector<TrialRes> res[3];
  size_t base = 0;   // next free slot of d_trials / d_tres
};

struct ProbeList {   // the probe extension's survivors
  std::vector<uint64_t> pos;   // the surviving positions, ascending
  double kernel_ms = 0;        // k_probe_ordered, both passes
};

struct MarkerList {   // the segment extension's flush markers
  std::vector<uint64_t> pos;   // every q with bytes q..q+3 = 00 00 FF FF, ascending
  double kernel_ms = 0;        // k_marker_ordered, both passes
};

struct atz_ctx {
  KTimer kt;
  atz_opts_t o{};
  int dev = 0;
  hipStream_t st = nullptr;
  DBuf d_rec, d_atzin;   // reconstructed original / uploaded ATZ1 bytes (atz_reconstruct*)
  DBuf d_file, d_pos, d_cnt, d_hbase, d_jobs, d_res, d_virt, d_infl, d_chains, d_heads, d_streams, d_trials,
      d_tres, d_out, d_syms, d_adler, d_meta, d_segs, d_atz, d_diffjobs, d_diffpos, d_diffval, d_diffcnt,
      d_cjobs, d_cjobs2, d_cjobs3, d_heads2, d_tmp, d_R, d_mjobs, d_ins, d_arena, d_arena_used;
  // last scan
  std::vector<Rec> recs;
  std::vector<uint64_t> infl_off;   // per record offset in d_infl
  std::vector<uint32_t> adler;
  const uint8_t* hfile = nullptr;   // caller's host copy; valid only inside the call that set it
  uint64_t flen = 0;
  // atz_scan -> atz_sweep hand-off: set by a successful atz_scan, cleared by every call that
  // replaces recs / d_file (precompress, deflate, reconstruct, inflate_batch)
  bool scan_valid = false;
  // opt-in strategy trials (atz_set_strategies): bit k = zlib strategy k (1 Z_FILTERED, 2 Z_HUFFMAN_ONLY,
  // 3 Z_RLE) is tried on the streams the reference walk leaves unrecorded; 0: off
  uint32_t strat_mask = 0;
  // opt-in container anchors (atz_set_containers): bit 0 ZIP local file headers, bit 1 gzip members -- raw
  // deflate bodies behind them become records of type 24 + hint, which only raw_pass walks; 0: off
  uint32_t cont_mask = 0;
  // opt-in stitching (atz_set_stitch): bit 0 PNG IDAT chains -- a zlib stream split over consecutive IDAT
  // chunks is gathered into d_stitch, decoded and walked there; 0: off.  d_stitch lives until the next scan
  // (the sweep, the diff lists and the re-inflates read it); st_off / st_len: the pieces of the last scan's
  // stitched records, file offset and length each (Rec::p0, Rec::pk)
  uint32_t stitch_mask = 0;
  // opt-in probe (atz_set_probe): bit 0 raw deflate streams whose first block is dynamic, which no header or
  // container announces -- records of type 24 (raw, no hint), walked by raw_pass; 0: off
  uint32_t probe_mask = 0;
  // opt-in segments (atz_set_segments): bit 0 streams cut by full-flush points become one raw record per
  // segment (seg_merge), the flush-terminated ones with Rec::flags bit 7; 0: off
  uint32_t seg_mask = 0;
  // opt-in deflater families for the raw walk (atz_set_deflaters): bit 0 GNU gzip's and Info-ZIP's; 0: zlib's only
  uint32_t defl_mask = 0;
  DBuf d_stitch;
  std::vector<uint64_t> st_off, st_len;
  // atz_sweep reports every stream's best ident, c, w, m as the reference computes them; the precompress
  // paths only need what the ATZ1 holds, so they let trials stop once they cannot make their stream
  // recompressible (elig_floor)
  bool exact_idents = false;
  std::vector<uint32_t> scan_trailer;   // per record: the stream's Adler-32 trailer (big-endian word)
  bool file_on_device = false;      // d_file holds the current file
  const uint8_t* dev_file = nullptr;
  atz_stats_t stats{};
  // hash-bucket cache: per record and memLevel the tables' absolute device address / 4 (u32 units
  // from a null base; ~0: not built), in chain_arena
  std::vector<std::array<uint64_t, 10>> chain_off;
  DevArena chain_arena;
  // symbol replay: saved sequences and per-stream entries (StreamState::rp indexes rp_pool, reserved
  // for every stream of the sweep so that a pipe's push_back never moves another pipe's entries)
  DevArena rp_arena;
  std::vector<std::array<RpEntry, 9>> rp_pool;   // [stream's entry][level - 1]
  std::mutex rp_mu;
  // deepest bucket - 1 per (stream, memLevel) at [10 s + m], written by k_buckets_sort into pinned
  // host memory (~0: not built yet); read after the building stream has been synchronised
  PinBuf depth_pin;
  // The sweep's queues of streams waiting for their next step (see sched_take)
  struct Sched {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::deque<uint32_t>> q;  // one per pipe
    std::vector<size_t> unfinished;       // published streams not done, per pipe
    bool closed = false;                  // every stream is published
    bool abort = false;
    std::atomic<size_t> published{0};     // streams published to the sweep so far (round_target)
  } sched;
  std::vector<std::unique_ptr<Pipe>> pipes;
  std::vector<std::unique_ptr<DBuf>> slabs;   // inflated records, one allocation per scan piece
  size_t pipes_running = 1;
  size_t sweep_nmax = 0;   // the sweep's bound on its streams (sweep_begin)
  std::atomic<bool> sweep_abort{false};   // the pipes stop at their next round (a withdrawn speculative scan)
  // precompress_dev's large per-call state, kept so its capacity survives the calls
  std::shared_ptr<struct ScanState> scan_keep;
  // atz_precompress: called once the sweep has the speculative records, with an estimate of the ATZ1 size
  std::function<void(uint64_t)> on_records;
  std::vector<StreamState> ss_keep;
  std::vector<StreamDev> sd_keep;
  // multi-GPU precompress of one file (atz_shard_*): this rank's state between the calls
  struct Shard {
    std::shared_ptr<struct ScanState> S;
    int rank = -1, world = 0;
    uint32_t ja = 0, jb = 0;
    uint64_t F = 0;
    std::vector<std::pair<uint64_t, uint64_t>> all;   // every record of the file: (offset, comp_len)
    uint64_t piece_len = 0;
    int stage = 0;   // 1 scanned, 2 swept (piece in d_atz)
    std::chrono::steady_clock::time_point t0;
  } shard;
  // the probe extension's list for the current scan (kept here, not in precompress_dev's frame, whose
  // layout the sweep's threads share: with the mask off the call's stack is exactly what it was)
  ProbeList probe;
  MarkerList marks;   // the segment extension's, likewise
  // opt-in nesting (atz_set_nesting): with a depth d >= 1 a precompress runs the whole pipeline
  // again, at depth d - 1, on P -- the recorded streams' payloads, gathered into d_nestp and copied once to
  // h_nestp -- in a child context on the same device, opened at the first need and closed with this one.  A
  // reconstruct of a nested file uses the child too, whatever the depth: the inner file's original stays in the
  // child's d_rec.  nest_ran: the child's precompress completed in this context's last precompress.
  int nest_depth = 0;
  atz_ctx* nest_child = nullptr;
  bool nest_ran = false;
  DBuf d_nestp;
  std::vector<uint8_t> h_nestp;
};

// kind: 0 trial, 1 inflate, 2 chains, 3 other, 4 match tables, 5 GNU-family trial (counted as a trial too)
template <class C>
static void kbeg(C* c, int kind, hipStream_t st = nullptr) {
  hipEvent_t a = c->kt.get(), b = c->kt.get();
  (void)hipEventRecord(a, st ? st : c->st);
  c->kt.pending.push_back({a, b});
  c->kt.kind.push_back(kind);
}
template <class C>
static void kend(C* c, hipStream_t st = nullptr) { (void)hipEventRecord(c->kt.pending.back().second, st ? st : c->st); }
// after a stream synchronisation: fold elapsed times into the stats
template <class C>
static void kcollect(C* c) {
  for (size_t i = 0; i < c->kt.pending.size(); i++) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, c->kt.pending[i].first, c->kt.pending[i].second);
    switch (c->kt.kind[i]) {
      case 5: c->kt.gnu_ms += ms; [[fallthrough]];
      case 0: c->stats.k_trial_ms += ms; c->stats.k_trial_launches++; break;
      case 1: c->stats.k_inflate_ms += ms; c->stats.k_inflate_launches++; break;
      case 2: c->stats.k_chains_ms += ms; c->stats.k_chains_launches++; break;
      case 4: c->stats.k_match_ms += ms; c->stats.k_match_launches++; break;
      default: c->stats.k_other_ms += ms; break;
    }
    c->kt.pool.push_back(c->kt.pending[i].first);
    c->kt.pool.push_back(c->kt.pending[i].second);
  }
  c->kt.pending.clear();
  c->kt.kind.clear();
}

// copy n host bytes into b (device capacity n + slack; the slack is never read from the host)
template <class C> static void copy_timed(C*, double) {}
template <> void copy_timed<Pipe>(Pipe* p, double ms) { p->t_copy += ms; p->n_copy++; }
// The source of a host -> device upload: a pipe's copies go through its pinned staging (ATZ_STAGE=0: not),
// the context's straight from the caller's memory.  (A full staging buffer falls back to the latter.)
static bool stage_on() {
  static const bool v = [] { const char* e = std::getenv("ATZ_STAGE"); return !e || std::atoi(e) != 0; }();
  return v;
}
static constexpr size_t STAGE_BYTES = 32u << 20;
template <class C> static const void* staged(C*, const void* h, size_t) { return h; }
template <> const void* staged<Pipe>(Pipe* p, const void* h, size_t n) {
  if (!stage_on() || !n) return h;
  if (!p->stage.p && p->stage.reserve(STAGE_BYTES)) return h;
  const size_t a = (p->stage_used + 255) & ~(size_t)255;
  if (a + n > p->stage.n) return h;
  std::memcpy(static_cast<uint8_t*>(p->stage.p) + a, h, n);
  p->stage_used = a + n;
  return static_cast<uint8_t*>(p->stage.p) + a;
}
// a pipe's stream synchronisation, timed (ATZ_TIMING)
static hipError_t pipe_sync(Pipe* p) {
  const auto t = std::chrono::steady_clock::now();
  const hipError_t e = hipStreamSynchronize(p->st);
  if (e == hipSuccess) p->stage_used = 0;   // every staged copy has run
  p->t_sync += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
  p->n_sync++;
  return e;
}
// a pipe's copy to or from the host, timed (ATZ_TIMING)
static hipError_t pipe_copy(Pipe* p, void* dst, const void* src, size_t n, hipMemcpyKind k) {
  const auto t = std::chrono::steady_clock::now();
  if (k == hipMemcpyHostToDevice) src = staged(p, src, n);
  const hipError_t e = hipMemcpyAsync(dst, src, n, k, p->st);
  copy_timed(p, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count());
  return e;
}
template <class C>
static int upload(C* c, DBuf& b, const void* h, size_t n, size_t slack = 4096) {
  if (int r = b.reserve(n + slack)) return r;
  const auto t = std::chrono::steady_clock::now();
  if (n) HIPCHK(hipMemcpyAsync(b.p, staged(c, h, n), n, hipMemcpyHostToDevice, c->st));
  copy_timed(c, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count());
  return 0;
}

static bool sync_debug() {
  static const int v = [] { const char* e = std::getenv("ATZ_SYNC_DEBUG"); return (int)(e && *e == '1'); }();
  return v == 1;
}
// ATZ_SYNC_DEBUG=1: synchronise after every launch and name the kernel that failed
#define KCHECK(name)                                                                            \
  do {                                                                                          \
    hipError_t e_ = hipGetLastError();                                                          \
    if (e_ == hipSuccess && sync_debug()) e_ = hipStreamSynchronize(c->st);                     \
    if (e_ != hipSuccess) {                                                                     \
      std::fprintf(stderr, "atz: kernel %s failed: %s (%s:%d)\n", name, hipGetErrorString(e_), \
                   __FILE__, __LINE__);                                                         \
      return ATZ_E_HIP;                                                                         \
    }                                                                                           \
  } while (0)

// ---------------------------------------------------------------------------------------------
// Phase 1
struct Chunk {
  uint64_t co;    // chunkOffset (file position of buffer[1] minus 1)
  uint64_t len;   // buffer length
  uint8_t b0;     // buffer[0]
  bool b0_file;   // buffer[0] == file[co] (buffer is contiguous file data)
};

static int timing_level() {   // ATZ_TIMING=1: phase timings, 2: + per-round sweep timeline
  static const int v = [] { const char* e = std::getenv("ATZ_TIMING"); return (int)(e ? std::atoi(e) : 0); }();
  return v;
}
static bool timing_on() { return timing_level() >= 1; }

static constexpr int INF_SEG = 2;   // run_inflate_jobs' raw argument: k_inflate's SEG variant
static int run_inflate_jobs(atz_ctx* c, const uint8_t* d_in, uint8_t* d_out, const std::vector<InfJob>& jobs,
                            std::vector<InfRes>& res, uint64_t arena_cap = 0, bool full_ring = false,
                            bool arena_reset = true, int raw = 0) {
  res.resize(jobs.size());
  if (jobs.empty()) return 0;
  auto ti0 = std::chrono::steady_clock::now();
  if (int r = upload(c, c->d_jobs, jobs.data(), jobs.size() * sizeof(InfJob))) return r;
  if (int r = c->d_res.reserve(jobs.size() * sizeof(InfRes))) return r;
  if (int r = c->d_arena_used.reserve(64)) return r;
  if (arena_cap && arena_reset) {
    if (int r = c->d_arena.reserve(arena_cap)) return r;
    HIPCHK(hipMemsetAsync(c->d_arena_used.p, 0, 8, c->st));
  }
  uint32_t n = (uint32_t)jobs.size();
  // The small-ring decoder needs an HBM copy of its output for matches beyond the ring: every job
  // writes to a destination or an arena slot.  Jobs without output use the 32 KiB ring.
  bool small = !full_ring;
  for (const InfJob& jb : jobs) small = small && jb.out_off != NO_OUT;
  kbeg(c, 1);
  // raw 1: deflate bodies without the zlib wrapper (the container extension's candidates and records);
  // raw 2 (INF_SEG): such bodies that also end at a flush marker (the segment extension)
  auto kern = small ? (raw == INF_SEG ? k_inflate<INF_RING_SMALL, true, true>
                       : raw          ? k_inflate<INF_RING_SMALL, true> : k_inflate<INF_RING_SMALL>)
                    : (raw == INF_SEG ? k_inflate<INF_RING_FULL, true, true>
                       : raw          ? k_inflate<INF_RING_FULL, true> : k_inflate<INF_RING_FULL>);
  hipLaunchKernelGGL(kern, dim3(n), dim3(64), 0, c->st, d_in, d_out, c->d_jobs.as<InfJob>(), c->d_res.as<InfRes>(), n,
                     c->d_arena.as<uint8_t>(), c->d_arena_used.as<unsigned long long>(), arena_cap);
  kend(c);
  KCHECK("k_inflate");
  const double ti_launch = ms_since(ti0);
  HIPCHK(hipMemcpyAsync(res.data(), c->d_res.p, n * sizeof(InfRes), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  const double ti_sync = ms_since(ti0);
  kcollect(c);
  if (timing_level() >= 2)
    std::fprintf(stderr, "atz: inflate jobs %u: launched at %.2f ms, synced at %.2f ms, collected at %.2f ms\n", n,
                 ti_launch, ti_sync, ms_since(ti0));
  if (small) {   // jobs whose far history was lost (arena full / slot overflowed): 32 KiB ring, no slot
    std::vector<InfJob> rj;
    std::vector<uint32_t> ri;
    for (uint32_t k = 0; k < n; k++)
      if (res[k].status == INF_RETRY) {
        InfJob jb = jobs[k];
        if (jb.out_off == ARENA_OUT) { jb.out_off = NO_OUT; jb.out_cap = 0; }
        rj.push_back(jb);
        ri.push_back(k);
      }
    if (!rj.empty()) {
      std::vector<InfRes> rr;
      if (int r = run_inflate_jobs(c, d_in, d_out, rj, rr, 0, true, true, raw)) return r;
      for (size_t q = 0; q < ri.size(); q++) res[ri[q]] = rr[q];
      c->stats.n_inflate_retries += rj.size();
    }
  }
  for (uint32_t k = 0; k < n; k++)   // bytes read + bytes written (when kept)
    c->stats.k_inflate_alg_bytes += res[k].consumed + (jobs[k].out_off == NO_OUT ? 0 : res[k].produced);
#if ATZ_INF_CLOCKS
  if (timing_on()) {   // diagnostics build: clocks per job / per symbol
    uint64_t cyc = 0, nl = 0, nm = 0, cmax = 0, outb = 0, cc = 0, cf = 0;
    for (uint32_t k = 0; k < n; k++) {
      cyc += res[k].cyc; nl += res[k].nlit; nm += res[k].nmatch; outb += res[k].produced;
      cc += res[k].cyc_copy; cf += res[k].cyc_flush;
      cmax = std::max<uint64_t>(cmax, res[k].cyc);
    }
    std::fprintf(stderr, "atz: k_inflate %u jobs: %.3f Gcyc, max %.2f Mcyc, lit %llu match %llu out %llu, "
                 "%.1f cyc/symbol (copy %.3f Gcyc, flush %.3f Gcyc)\n", n, cyc / 1e9, cmax / 1e6, (unsigned long long)nl,
                 (unsigned long long)nm, (unsigned long long)outb, (nl + nm) ? (double)cyc / (nl + nm) : 0.0, cc / 1e9, cf / 1e9);
    // where the cycles go: complete streams vs candidates that fail (false headers) by output size
    uint64_t ce = 0, ne = 0, cfl[4] = {}, nfl[4] = {}, nf = 0, cfar = 0;
    for (uint32_t k = 0; k < n; k++) nf += res[k].nfar, cfar += res[k].cyc_far;
    std::fprintf(stderr, "atz: k_inflate far matches (source beyond the LDS ring): %llu, %.3f Gcyc\n",
                 (unsigned long long)nf, cfar / 1e9);
    {
      uint64_t nb = 0, ch = 0, nlg = 0, nbs = 0, chs = 0;
      for (uint32_t k = 0; k < n; k++) {
        nb += res[k].nblk; ch += res[k].cyc_hdr; nlg += res[k].nlong;
        if (res[k].status == INF_END && res[k].consumed > 16) { nbs += res[k].nblk; chs += res[k].cyc_hdr; }
      }
      std::fprintf(stderr, "atz: k_inflate blocks %llu (streams: %llu), header+build %.3f Gcyc (streams: %.3f), "
                   "codes > 6 bits in the fast loop %llu\n", (unsigned long long)nb, (unsigned long long)nbs, ch / 1e9,
                   chs / 1e9, (unsigned long long)nlg);
    }
    for (uint32_t k = 0; k < n; k++) {
      if (res[k].status == INF_END && res[k].consumed > 16) { ce += res[k].cyc; ne++; continue; }
      const int b = res[k].produced < 64 ? 0 : res[k].produced < 1024 ? 1 : res[k].produced < 4096 ? 2 : 3;
      cfl[b] += res[k].cyc; nfl[b]++;
    }
    std::fprintf(stderr, "atz: k_inflate streams %llu: %.3f Gcyc; failing candidates by output <64/<1K/<4K/more: "
                 "%llu/%llu/%llu/%llu jobs, %.3f/%.3f/%.3f/%.3f Gcyc\n", (unsigned long long)ne, ce / 1e9,
                 (unsigned long long)nfl[0], (unsigned long long)nfl[1], (unsigned long long)nfl[2], (unsigned long long)nfl[3],
                 cfl[0] / 1e9, cfl[1] / 1e9, cfl[2] / 1e9, cfl[3] / 1e9);
  }
#endif
  return 0;
}

// inflate one materialized byte string (boundary continuations)
static int inflate_bytes(atz_ctx* c, const std::vector<uint8_t>& v, InfRes& out) {
  if (int r = upload(c, c->d_virt, v.data(), v.size())) return r;
  std::vector<InfJob> j(1);
  j[0].in_off = 0; j[0].in_len = v.size(); j[0].out_off = NO_OUT; j[0].out_cap = 0;
  std::vector<InfRes> rr;
  if (int r = run_inflate_jobs(c, c->d_virt.as<uint8_t>(), nullptr, j, rr)) return r;
  out = rr[0];
  return 0;
}

static void chunk_bytes(const uint8_t* f, const Chunk& ch, std::vector<uint8_t>& v) {
  v.push_back(ch.b0);
  v.insert(v.end(), f + ch.co + 1, f + ch.co + ch.len);
}

// ATZ_TIMING=1: host phase timings on stderr
#define TMARK(name)                                                                        \
  do {                                                                                     \
    if (timing_on()) std::fprintf(stderr, "atz: %-28s %9.2f ms\n", name, ms_since(tm_));   \
    tm_ = std::chrono::steady_clock::now();                                                \
  } while (0)

// Phase 1 is split into a plan (chunk layout, header list, candidates) and pieces: contiguous chunk
// ranges whose candidates are inflated and replayed in file order.  The replay state (a pending
// stream at a chunk end) carries from one piece into the next, so any split gives the reference's
// sequential result; precompress_dev hands each piece's records to the sweep while the next piece
// is scanned.
struct ScanCand { uint32_t chunk; int32_t type; uint64_t i; };
// pending stream: its bytes are chunk j0 from i0 plus the napp following chunk buffers (size
// bytes); they are materialized only for a second refill (rare)
struct ScanPend { uint64_t off; int type; int state; uint32_t j0, napp; uint64_t i0, size; uint64_t in, out; long spec_chunk; int refills; bool noshort; uint8_t mhint; };
struct ScanState {
  std::vector<Chunk> chunks;
  std::vector<ScanCand> cands;
  std::vector<size_t> cbeg;      // chunk j's candidates: cands[cbeg[j] .. cbeg[j + 1])
  std::vector<InfRes> cres;      // per candidate
  std::vector<long> pend0;       // per chunk: pending candidate of the selection from i = 0 (-1: none)
  std::vector<InfRes> cont0;     // per chunk: speculative first continuation of that candidate
  bool need_more = false;
  ScanPend pd{};
  uint64_t arena_cap = 0;
  // per-call scratch, kept with the context's ScanState so its capacity survives the calls (multi-MB
  // buffers would otherwise be mapped, faulted in and unmapped on every precompress)
  std::vector<uint64_t> pairs;
  std::vector<InfJob> fjobs;
  std::vector<size_t> fk;
  std::vector<InfRes> fr;
  std::vector<Rec> check;
  uint64_t max_records() const { return cands.size() + chunks.size() + 1; }
};

// ATZ_CAP_DIV=d (read once; tests): every device-memory cap of the library divided by d -- the scan's
// output arena, the bucket cache, the replay arena and the round / batch scratch budgets -- so that
// small inputs take the paths past the caps (re-inflates, per-round tables, unsaved replays, deferred
// streams, several reconstruct batches) that only inputs of tens of GB reach otherwise.
static uint64_t cap_bytes(uint64_t cap) {
  static const uint64_t d = [] {
    const char* e = std::getenv("ATZ_CAP_DIV");
    const long long v = e ? std::atoll(e) : 1;
    return (uint64_t)(v > 1 ? v : 1);
  }();
  return std::max<uint64_t>(cap / d, 4096);
}
static uint64_t arena_cap_for(uint64_t scanned) {
  return cap_bytes(std::min<uint64_t>(64ull << 30, std::max<uint64_t>(1ull << 30, 8 * scanned)));
}
static int scan_plan(atz_ctx* c, const uint8_t* h, const uint8_t* d_file, uint64_t F, ScanState& S) {
  auto tm_ = std::chrono::steady_clock::now();
  const uint64_t cs = c->o.chunksize;
  if (cs < 2) return ATZ_E_REF_UB;      // main.cpp:410-415 never reaches eof with chunksize 1
  if (F == 0) return ATZ_E_REF_UB;      // main.cpp:406 reads rBuffer[-1]
  // ---- chunk layout exactly as searchInfile reads the file (main.cpp:405-415) ----
  std::vector<Chunk>& chunks = S.chunks;
  chunks.clear();
  {
    uint64_t g = F < cs ? F : cs;
    chunks.push_back({0, g, h[0], true});
    bool eof = g < cs;
    uint64_t pos = g;
    uint8_t last = h[g - 1];
    while (!eof) {
      uint64_t gg = F - pos < cs - 1 ? F - pos : cs - 1;
      Chunk ch{pos - 1, gg + 1, last, h[pos - 1] == last};
      chunks.push_back(ch);
      eof = gg < cs - 1;
      if (gg >= 2) last = h[pos + gg - 2];      // rBuffer[gcount-1] with data at rBuffer[1..gcount]
      else if (gg == 1) last = ch.b0;
      pos += gg;
    }
  }
  // ---- all header pairs of the file, in file order (GPU: count pass, host prefix, write pass),
  // packed position << 5 | header type ----
  std::vector<uint64_t>& pairs = S.pairs;
  pairs.clear();
  {
    const uint64_t nb = std::max<uint64_t>(1, std::min<uint64_t>(8192, (F + 65535) / 65536));
    const uint64_t seg = ((F + nb - 1) / nb + 4095) & ~4095ull;
    if (int r = c->d_cnt.reserve(nb * 4 + 64)) return r;
    if (int r = c->d_hbase.reserve(nb * 8 + 64)) return r;
    kbeg(c, 3);
    hipLaunchKernelGGL(k_headers_ordered, dim3((uint32_t)nb), dim3(256), 0, c->st, d_file, F, seg,
                       c->d_cnt.as<uint32_t>(), nullptr, nullptr, 0);
    kend(c);
    KCHECK("k_headers_ordered");
    std::vector<uint32_t> cnt(nb);
    HIPCHK(hipMemcpyAsync(cnt.data(), c->d_cnt.p, nb * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    std::vector<uint64_t> hb(nb);
    uint64_t npairs = 0;
    for (uint64_t b = 0; b < nb; b++) { hb[b] = npairs; npairs += cnt[b]; }
    if (npairs) {
      if (int r = upload(c, c->d_hbase, hb.data(), nb * 8)) return r;
      if (int r = c->d_pos.reserve(npairs * 8 + 64)) return r;
      kbeg(c, 3);
      hipLaunchKernelGGL(k_headers_ordered, dim3((uint32_t)nb), dim3(256), 0, c->st, d_file, F, seg,
                         nullptr, c->d_hbase.as<uint64_t>(), c->d_pos.as<uint64_t>(), 1);
      kend(c);
      KCHECK("k_headers_ordered");
      pairs.resize(npairs);
      HIPCHK(hipMemcpyAsync(pairs.data(), c->d_pos.p, npairs * 8, hipMemcpyDeviceToHost, c->st));
      HIPCHK(hipStreamSynchronize(c->st));
    }
    kcollect(c);
  }
  TMARK("scan: layout+ordered pairs");
  // ---- candidates per chunk: i >= 1 are file pairs, i == 0 uses buffer[0] ----
  S.cands.clear();
  S.cands.reserve(pairs.size() + chunks.size());
  S.cbeg.assign(chunks.size() + 1, 0);
  {
    size_t pi = 0;
    for (uint32_t j = 0; j < chunks.size(); j++) {
      S.cbeg[j] = S.cands.size();
      const Chunk& ch = chunks[j];
      if (ch.len < 2) continue;
      const int t0 = header_type_host(ch.b0, h[ch.co + 1]);
      if (t0 >= 0) S.cands.push_back({j, t0, 0});
      const uint64_t lo = ch.co + 1, hi = ch.co + ch.len - 2;   // file pairs scanned as i = 1 .. len-2
      while (pi < pairs.size() && (pairs[pi] >> 5) < lo) pi++;
      for (; pi < pairs.size() && (pairs[pi] >> 5) <= hi; pi++)
        S.cands.push_back({j, (int32_t)(pairs[pi] & 31), (pairs[pi] >> 5) - ch.co});
    }
    S.cbeg[chunks.size()] = S.cands.size();
  }
  S.cres.assign(S.cands.size(), InfRes{});
  S.pend0.assign(chunks.size(), -1);
  S.cont0.assign(chunks.size(), InfRes{});
  S.need_more = false;
  S.pd = ScanPend{};
  // a slot (ARENA_SLOT) is claimed at a candidate's first flush (4 KiB of output): room for a slot
  // per 8 KiB of input (C4: 6.5 GB of slots for 1 GB), capped; a candidate that finds the arena full
  // keeps no output and is inflated again if it becomes a record (n_reinflated)
  S.arena_cap = arena_cap_for(F);
  c->stats.n_candidates = S.cands.size();
  TMARK("scan: candidates");
  return 0;
}

// greedy selection in chunk j from position i0 (main.cpp:218-241); records go to *out.  Returns
// the pending candidate index or -1.
static long scan_select(const ScanState& S, uint32_t j, uint64_t i0, std::vector<Rec>* out) {
  const Chunk& ch = S.chunks[j];
  uint64_t i = i0;
  for (size_t k = S.cbeg[j]; k < S.cbeg[j + 1]; k++) {
    const ScanCand& cd = S.cands[k];
    if (cd.i < i) continue;
    const InfRes& r = S.cres[k];
    if (r.consumed <= 16) continue;
    if (r.status == INF_END) {
      if (out) {
        out->push_back({cd.i + ch.co, r.consumed, r.produced, cd.type, 0, r.arena_off});
        out->back().noshort = (r.err & INF_HINT_NOSHORT) != 0;
        out->back().mhint = (uint8_t)((r.err >> INF_HINT_MLEV_SHIFT) & 15u);
      }
      i = cd.i + r.consumed;
    } else if (r.consumed == ch.len - cd.i) {
      return (long)k;
    }
  }
  return -1;
}

// Chunks [ja, jb): candidate inflates (their outputs kept in the arena, which is reset: earlier
// pieces' records were gathered out of it already) and speculative first continuations.
static int scan_candidates(atz_ctx* c, const uint8_t* h, const uint8_t* d_file, ScanState& S, uint32_t ja, uint32_t jb) {
  auto tm_ = std::chrono::steady_clock::now();
  const std::vector<Chunk>& chunks = S.chunks;
  const size_t k0 = S.cbeg[ja], k1 = S.cbeg[jb];
  {
    // file-backed jobs (output kept in an arena slot), and materialized buffers for chunk starts
    // whose buffer[0] is not the file byte
    std::vector<InfJob>& fjobs = S.fjobs;
    std::vector<size_t>& fk = S.fk;
    fjobs.clear();
    fk.clear();
    std::vector<InfJob> vjobs;
    std::vector<size_t> vk;
    std::vector<uint8_t> virt;
    fjobs.reserve(k1 - k0);
    fk.reserve(k1 - k0);
    for (size_t k = k0; k < k1; k++) {
      const ScanCand& cd = S.cands[k];
      const Chunk& ch = chunks[cd.chunk];
      if (cd.i == 0 && !ch.b0_file) {
        InfJob jb2;
        jb2.in_off = virt.size(); jb2.in_len = ch.len; jb2.out_off = NO_OUT; jb2.out_cap = 0;
        std::vector<uint8_t> v;
        chunk_bytes(h, ch, v);
        virt.insert(virt.end(), v.begin(), v.end());
        virt.resize((virt.size() + 3) & ~(size_t)3);
        vjobs.push_back(jb2);
        vk.push_back(k);
      } else {
        fjobs.push_back({ch.co + cd.i, ch.len - cd.i, ARENA_OUT, ARENA_SLOT});
        fk.push_back(k);
      }
    }
    std::vector<InfRes>& fr = S.fr;
    std::vector<InfRes> vr;
    if (int r = run_inflate_jobs(c, d_file, nullptr, fjobs, fr, S.arena_cap)) return r;
    if (!vjobs.empty()) {
      if (int r = upload(c, c->d_virt, virt.data(), virt.size())) return r;
      if (int r = run_inflate_jobs(c, c->d_virt.as<uint8_t>(), nullptr, vjobs, vr)) return r;
    }
    for (size_t q = 0; q < fk.size(); q++) S.cres[fk[q]] = fr[q];
    for (size_t q = 0; q < vk.size(); q++) S.cres[vk[q]] = vr[q];
  }
  TMARK("scan: candidate inflate");
  return 0;
}

// the pending candidate of each chunk of [ja, jb) for a selection from i = 0 (S.pend0); returns the
// chunks that have one (their first continuation is needed)
static std::vector<uint32_t> scan_pending(ScanState& S, uint32_t ja, uint32_t jb) {
  std::vector<uint32_t> todo;
  for (uint32_t j = ja; j < jb && j + 1 < S.chunks.size(); j++) {
    const long k = scan_select(S, j, 0, nullptr);
    S.pend0[j] = k;
    if (k >= 0) todo.push_back(j);
  }
  return todo;
}

static int scan_continuations(atz_ctx* c, const uint8_t* h, const uint8_t* d_file, ScanState& S, uint32_t ja, uint32_t jb) {
  (void)h;
  auto tm_ = std::chrono::steady_clock::now();
  const std::vector<Chunk>& chunks = S.chunks;
  {
    // speculative first continuations: pending candidate of chunk j (selection from 0) + buffer
    // j+1, assembled in HBM by k_gather from file ranges and the chunks' buffer[0] bytes.  The first
    // pass offers only the first CONT_PROBE bytes of buffer j+1: a decode that ends or fails inside
    // them reads no further, so its status / total_in / total_out are those of the whole buffer
    // (k_inflate consumes exactly zlib's bits); one that runs out of input is decoded again with
    // the whole buffer.  (The duplicated byte almost always ends them within a few symbols.)
    static constexpr uint64_t CONT_PROBE = 65536;
    std::vector<uint32_t> todo = scan_pending(S, ja, jb);
    c->stats.n_continuations += todo.size();
    TMARK("scan: cont select");
    for (int pass = 0; pass < 2 && !todo.empty(); pass++) {
      std::vector<Seg> segs;
      std::vector<uint8_t> meta;
      uint64_t out = 0;
      auto add_file = [&](uint64_t off, uint64_t len) { if (len) segs.push_back({SEG_FILE, 0, off, out, len}); out += len; };
      auto add_byte = [&](uint8_t b) { segs.push_back({SEG_META, 0, meta.size(), out, 1}); meta.push_back(b); out += 1; };
      std::vector<InfJob> cj;
      std::vector<bool> cut;
      for (uint32_t j : todo) {
        const ScanCand& cd = S.cands[S.pend0[j]];
        const Chunk& ch = chunks[j];
        const Chunk& nx = chunks[j + 1];
        InfJob jb2;
        jb2.in_off = out;
        if (cd.i == 0) { add_byte(ch.b0); add_file(ch.co + 1, ch.len - 1); }
        else add_file(ch.co + cd.i, ch.len - cd.i);
        add_byte(nx.b0);
        const uint64_t take = (pass == 0 && nx.len - 1 > CONT_PROBE) ? CONT_PROBE : nx.len - 1;
        add_file(nx.co + 1, take);
        cut.push_back(take < nx.len - 1);
        // output into arena slots after the scan's (small-ring decoder); the bytes are not used
        jb2.in_len = out - jb2.in_off; jb2.out_off = ARENA_OUT; jb2.out_cap = ARENA_SLOT;
        cj.push_back(jb2);
        out = (out + 3) & ~3ull;
      }
      TMARK("scan: cont segs");
      if (int r = upload(c, c->d_meta, meta.data(), meta.size())) return r;
      if (int r = upload(c, c->d_segs, segs.data(), segs.size() * sizeof(Seg))) return r;
      if (int r = c->d_virt.reserve(out + 4096)) return r;
      TMARK("scan: cont upload+reserve");
      const uint32_t nseg = (uint32_t)segs.size();
      const uint32_t blocks = std::min<uint32_t>((nseg + 3) / 4, 65535u);
      kbeg(c, 3);
      hipLaunchKernelGGL(k_gather, dim3(blocks), dim3(256), 0, c->st, c->d_meta.as<uint8_t>(), nullptr, d_file,
                         c->d_virt.as<uint8_t>(), c->d_segs.as<Seg>(), nseg);
      kend(c);
      KCHECK("k_gather");
      TMARK("scan: cont gather launch");
      std::vector<InfRes> cr;
      if (int r = run_inflate_jobs(c, c->d_virt.as<uint8_t>(), nullptr, cj, cr, S.arena_cap, false, false)) return r;
      if (timing_on()) {
        uint64_t cmax = 0, ctot = 0, pmax = 0, st[4] = {};
        for (size_t q = 0; q < cj.size(); q++) {
          cmax = std::max<uint64_t>(cmax, cr[q].consumed); ctot += cr[q].consumed;
          pmax = std::max<uint64_t>(pmax, cr[q].produced); st[cr[q].status & 3]++;
        }
        std::fprintf(stderr, "atz: continuations pass %d: %zu jobs, %.1f MB offered, consumed %.1f MB (max %llu), "
                     "max produced %llu, end/error/need/retry %llu/%llu/%llu/%llu, %.2f ms\n", pass, cj.size(), out / 1e6,
                     ctot / 1e6, (unsigned long long)cmax, (unsigned long long)pmax, (unsigned long long)st[0],
                     (unsigned long long)st[1], (unsigned long long)st[2], (unsigned long long)st[3], ms_since(tm_));
      }
      std::vector<uint32_t> again;
      for (size_t q = 0; q < cj.size(); q++) {
        if (cut[q] && cr[q].status == INF_NEED) again.push_back(todo[q]);
        else S.cont0[todo[q]] = cr[q];
      }
      todo.swap(again);
    }
  }
  TMARK("scan: continuations");
  return 0;
}

static int scan_inflate(atz_ctx* c, const uint8_t* h, const uint8_t* d_file, ScanState& S, uint32_t ja, uint32_t jb) {
  if (int r = scan_candidates(c, h, d_file, S, ja, jb)) return r;
  return scan_continuations(c, h, d_file, S, ja, jb);
}

// The sequential replay of chunks [ja, jb) (main.cpp:205-246 over searchInfile's chunk sequence),
// appending to c->recs; needs the candidate results and first continuations of those chunks.
static int scan_replay(atz_ctx* c, const uint8_t* h, ScanState& S, uint32_t ja, uint32_t jb,
                       std::vector<Rec>* recs_out = nullptr) {
  std::vector<Rec>& recs = recs_out ? *recs_out : c->recs;
  auto tm_ = std::chrono::steady_clock::now();
  const std::vector<Chunk>& chunks = S.chunks;
  ScanPend& pd = S.pd;
  auto materialize = [&](const ScanPend& q, std::vector<uint8_t>& v) {
    v.clear();
    const Chunk& c0 = chunks[q.j0];
    if (q.i0 == 0) chunk_bytes(h, c0, v);
    else v.assign(h + c0.co + q.i0, h + c0.co + c0.len);
    for (uint32_t k = 1; k <= q.napp; k++) chunk_bytes(h, chunks[q.j0 + k], v);
  };
  // c->recs never reallocates while the sweep reads it (capacity = S.max_records())
  auto room = [&]() { return recs.capacity() - recs.size() >= (S.cbeg[jb] - S.cbeg[ja]) + (jb - ja); };
  if (!room()) return ATZ_E_INTERNAL;
  for (uint32_t j = ja; j < jb; j++) {
    const Chunk& ch = chunks[j];
    uint64_t i = 0;
    if (S.need_more) {
      uint64_t avail;
      int st;
      if (pd.state == INF_NEED) {
        InfRes rr;
        if (pd.refills == 0 && pd.spec_chunk == (long)j - 1) {
          rr = S.cont0[j - 1];
        } else {
          std::vector<uint8_t> v;
          materialize(pd, v);
          chunk_bytes(h, ch, v);
          if (int r = inflate_bytes(c, v, rr)) return r;
        }
        pd.napp++;
        pd.size += ch.len;
        pd.refills++;
        pd.state = (int)rr.status; pd.in = rr.consumed; pd.out = rr.produced;
        // the first block's memLevel hint: a partial decode has it only if that block ended before the
        // chunk boundary; the continuation decodes the stream from its header (a shard's blob of another
        // rank's continuation carries no hint bits: whole tables are then just not built up front)
        if (!pd.mhint && rr.status == INF_END) pd.mhint = (uint8_t)((rr.err >> INF_HINT_MLEV_SHIFT) & 15u);
        avail = pd.size - rr.consumed;
        st = (int)rr.status;
      } else if (pd.state == INF_END) {  // inflate() in DONE mode returns Z_STREAM_END again
        avail = ch.len; st = INF_END;
      } else {                           // BAD mode: Z_DATA_ERROR, nothing consumed
        avail = ch.len; st = INF_ERROR;
      }
      if (st == INF_END) {
        recs.push_back({pd.off, pd.in, pd.out, pd.type, 1});
        recs.back().noshort = pd.noshort;
        recs.back().mhint = pd.mhint;
        i = ch.len - avail;
      }
      S.need_more = avail == 0;
    }
    if (!S.need_more) {
      const long k = scan_select(S, j, i, &recs);
      if (k >= 0) {
        const ScanCand& cd = S.cands[k];
        S.need_more = true;
        pd.off = cd.i + ch.co; pd.type = cd.type; pd.state = (int)S.cres[k].status;
        pd.in = S.cres[k].consumed; pd.out = S.cres[k].produced;
        pd.noshort = (S.cres[k].err & INF_HINT_NOSHORT) != 0;
        pd.mhint = (uint8_t)((S.cres[k].err >> INF_HINT_MLEV_SHIFT) & 15u);
        pd.j0 = j; pd.i0 = cd.i; pd.napp = 0;
        pd.size = cd.i == 0 ? ch.len : ch.len - cd.i;
        pd.spec_chunk = (i == 0 && S.pend0[j] == k) ? (long)j : -2;
        pd.refills = 0;
      }
    }
  }
  TMARK("scan: replay");
  return 0;
}

static int scan_piece(atz_ctx* c, const uint8_t* h, const uint8_t* d_file, ScanState& S, uint32_t ja, uint32_t jb) {
  if (int r = scan_inflate(c, h, d_file, S, ja, jb)) return r;
  return scan_replay(c, h, S, ja, jb);
}

// ---------------------------------------------------------------------------------------------
// The scan's opt-in extensions: containers, stitching, probe, flush segments.  Their
// rules -- what a list kernel's positions make of jobs, what the jobs' results make of records -- are
// atz_scanext.h's, which alone reads the host copy of the file; here are the list kernels' launches and, per
// extension, a merge that runs the jobs between the header's job step and its accept step.

// An ordered list kernel's two passes over the file (count pass, host prefix over the blocks, write pass):
// launch(nb, seg, cnt, base, out, write) starts one pass of `name`; *kernel_ms: both passes' device time.
template <class Launch>
static int ordered_list_dev(atz_ctx* c, uint64_t F, const char* name, Launch launch, std::vector<uint64_t>& out,
                            double* kernel_ms) {
  const uint64_t nb = std::max<uint64_t>(1, std::min<uint64_t>(8192, (F + 65535) / 65536));
  const uint64_t seg = ((F + nb - 1) / nb + 4095) & ~4095ull;
  if (int r = c->d_cnt.reserve(nb * 4 + 64)) return r;
  if (int r = c->d_hbase.reserve(nb * 8 + 64)) return r;
  const double other0 = c->stats.k_other_ms;
  kbeg(c, 3);
  launch((uint32_t)nb, seg, c->d_cnt.as<uint32_t>(), (const uint64_t*)nullptr, (uint64_t*)nullptr, 0);
  kend(c);
  KCHECK(name);
  std::vector<uint32_t> cnt(nb);
  HIPCHK(hipMemcpyAsync(cnt.data(), c->d_cnt.p, nb * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  std::vector<uint64_t> hb(nb);
  uint64_t na = 0;
  for (uint64_t b = 0; b < nb; b++) { hb[b] = na; na += cnt[b]; }
  if (na) {
    if (int r = upload(c, c->d_hbase, hb.data(), nb * 8)) return r;
    if (int r = c->d_pos.reserve(na * 8 + 64)) return r;
    kbeg(c, 3);
    launch((uint32_t)nb, seg, (uint32_t*)nullptr, c->d_hbase.as<uint64_t>(), c->d_pos.as<uint64_t>(), 1);
    kend(c);
    KCHECK(name);
    out.resize(na);
    HIPCHK(hipMemcpyAsync(out.data(), c->d_pos.p, na * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  }
  kcollect(c);
  *kernel_ms = c->stats.k_other_ms - other0;
  return 0;
}

// the positions an ordered list kernel without further arguments finds in the file (ProbeList, MarkerList)
template <class Kernel, class List>
static int positions_dev(atz_ctx* c, const uint8_t* d_file, uint64_t F, Kernel kernel, const char* name, List& L) {
  L.pos.clear();
  L.kernel_ms = 0;
  if (!F) return 0;
  auto launch = [&](uint32_t nb, uint64_t seg, uint32_t* cnt, const uint64_t* base, uint64_t* dst, int write) {
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, c->st, d_file, F, seg, cnt, base, dst, write);
  };
  return ordered_list_dev(c, F, name, launch, L.pos, &L.kernel_ms);
}

// the anchors of the file, ascending: position << 5 | kind
static int anchors_dev(atz_ctx* c, const uint8_t* d_file, uint64_t F, uint32_t mask, std::vector<uint64_t>& out) {
  out.clear();
  if (!mask || !F) return 0;
  const auto t0 = std::chrono::steady_clock::now();
  double kms = 0;
  auto launch = [&](uint32_t nb, uint64_t seg, uint32_t* cnt, const uint64_t* base, uint64_t* dst, int write) {
    hipLaunchKernelGGL(k_anchors_ordered, dim3(nb), dim3(256), 0, c->st, d_file, F, seg, mask, cnt, base, dst, write);
  };
  if (int r = ordered_list_dev(c, F, "k_anchors_ordered", launch, out, &kms)) return r;
  if (timing_on())
    std::fprintf(stderr, "atz: k_anchors_ordered: %llu anchors, kernels %.3f ms (both passes), host %.2f ms\n",
                 (unsigned long long)out.size(), kms, ms_since(t0));
  return 0;
}

// k_anchors_ordered's mask for the context's extensions: the container kinds and, for a stitch mask, kind 2
static uint32_t ext_anchor_mask(const atz_ctx* c) { return c->cont_mask | ((c->stitch_mask & 1u) ? 4u : 0u); }
static int probe_dev(atz_ctx* c, const uint8_t* d_file, uint64_t F, ProbeList& P) {
  return positions_dev(c, d_file, F, k_probe_ordered, "k_probe_ordered", P);
}
static int markers_dev(atz_ctx* c, const uint8_t* d_file, uint64_t F, MarkerList& M) {
  return positions_dev(c, d_file, F, k_marker_ordered, "k_marker_ordered", M);
}

// k_gather of the segments into dst (device): metadata, resident payloads, file ranges
static int gather_segments(atz_ctx* c, const uint8_t* d_file, const std::vector<uint8_t>& meta,
                           const std::vector<Seg>& segs, uint8_t* dst) {
  if (int r = upload(c, c->d_meta, meta.data(), meta.size())) return r;
  if (int r = upload(c, c->d_segs, segs.data(), segs.size() * sizeof(Seg))) return r;
  const uint32_t nseg = (uint32_t)segs.size();
  const uint32_t blocks = std::min<uint32_t>((nseg + 3) / 4, 65535u);
  kbeg(c, 3);
  hipLaunchKernelGGL(k_gather, dim3(blocks ? blocks : 1), dim3(256), 0, c->st, c->d_meta.as<uint8_t>(),
                     INFL_BASE, d_file, dst, c->d_segs.as<Seg>(), nseg);
  kend(c);
  KCHECK("k_gather");
  HIPCHK(hipStreamSynchronize(c->st));
  kcollect(c);
  return 0;
}

// The merges below add an extension's records to c->recs (every record made before, complete, in file order),
// which keeps its capacity (the sweep's tables are sized for it).  The decoded outputs go to the scan's arena,
// behind the earlier candidates' (fresh_arena: no job ran before).
static int raw_merge(atz_ctx* c, const uint8_t* h, const uint8_t* d_file, uint64_t arena_cap, bool fresh_arena,
                     const std::vector<RawCand>& cands) {
  if (cands.empty()) return 0;
  auto tm_ = std::chrono::steady_clock::now();
  std::vector<InfJob> jobs;
  raw_jobs(cands, jobs);
  std::vector<InfRes> res;
  if (int r = run_inflate_jobs(c, d_file, nullptr, jobs, res, arena_cap, false, fresh_arena, true)) return r;
  std::vector<Rec> kept;
  if (int r = raw_accept(h, cands, res, c->recs, kept)) return r;
  if (int r = splice(c->recs, kept)) return r;
  TMARK("scan: raw candidates");
  return 0;
}

// The stitch buffer holds every candidate's run (atz_scanext.h: at most F + 256 * candidates bytes), plus the 4 KiB
// of zero slack that d_file has (the kernels read past an end).
static int stitch_merge(atz_ctx* c, const uint8_t* d_file, uint64_t arena_cap, bool fresh_arena, const StitchPlan& P) {
  if (P.cands.empty()) return 0;
  auto tm_ = std::chrono::steady_clock::now();
  if (int r = c->d_stitch.reserve(P.bytes + 4096)) return r;
  HIPCHK(hipMemsetAsync(c->d_stitch.as<uint8_t>() + P.bytes, 0, 4096, c->st));
  std::vector<Seg> segs;
  std::vector<InfJob> jobs;
  stitch_jobs(P, segs, jobs);
  const double other0 = c->stats.k_other_ms, infl0 = c->stats.k_inflate_ms;
  if (int r = gather_segments(c, d_file, {}, segs, c->d_stitch.as<uint8_t>())) return r;
  std::vector<InfRes> res;
  if (int r = run_inflate_jobs(c, c->d_stitch.as<uint8_t>(), nullptr, jobs, res, arena_cap, false, fresh_arena)) return r;
  if (timing_on())
    std::fprintf(stderr, "atz: stitch: %zu candidates, %llu bytes in %zu segments, k_gather %.3f ms, k_inflate %.3f ms\n",
                 P.cands.size(), (unsigned long long)P.bytes, segs.size(), c->stats.k_other_ms - other0,
                 c->stats.k_inflate_ms - infl0);
  std::vector<Rec> kept;
  if (int r = stitch_accept(P, res, c->recs, c->st_off, c->st_len, kept)) return r;
  if (int r = splice(c->recs, kept)) return r;
  TMARK("scan: stitched candidates");
  return 0;
}

static int probe_merge(atz_ctx* c, const uint8_t* d_file, uint64_t F, uint64_t arena_cap, bool fresh_arena,
                       const ProbeList& P) {
  auto tm_ = std::chrono::steady_clock::now();
  std::vector<InfJob> jobs;
  if (int r = probe_jobs(P.pos, F, c->recs, jobs)) return r;
  const double infl0 = c->stats.k_inflate_ms;
  std::vector<InfRes> res;
  if (int r = run_inflate_jobs(c, d_file, nullptr, jobs, res, arena_cap, false, fresh_arena, true)) return r;
  std::vector<Rec> kept;
  size_t accepted = 0;
  if (int r = probe_accept(jobs, res, c->recs, kept, accepted)) return r;
  if (timing_on())
    std::fprintf(stderr, "atz: k_probe_ordered: %zu survivors, kernels %.3f ms (both passes), %zu decoded, "
                 "k_inflate %.3f ms, %zu accepted, %zu kept\n", P.pos.size(), P.kernel_ms, jobs.size(),
                 c->stats.k_inflate_ms - infl0, accepted, kept.size());
  if (int r = splice(c->recs, kept)) return r;
  TMARK("scan: probe candidates");
  return 0;
}

// (the segments' jobs write no output: a replaced record's decode, in the arena or not, is its segments' side by side)
static int seg_merge(atz_ctx* c, const uint8_t* h, const uint8_t* d_file, uint64_t F, const MarkerList& M) {
  auto tm_ = std::chrono::steady_clock::now();
  std::vector<SegElig> el;
  std::vector<InfJob> jobs;
  if (int r = seg_jobs(h, F, c->recs, M.pos, el, jobs)) return r;
  const double infl0 = c->stats.k_inflate_ms;
  std::vector<InfRes> res;
  if (int r = run_inflate_jobs(c, d_file, nullptr, jobs, res, 0, true, true, INF_SEG)) return r;
  std::vector<Rec> merged;
  size_t chains = 0, made = 0;
  if (int r = seg_accept(h, c->recs, el, jobs, res, merged, chains, made)) return r;
  if (timing_on())
    std::fprintf(stderr, "atz: k_marker_ordered: %zu markers, kernels %.3f ms (both passes), %zu eligible records, "
                 "%zu jobs, k_inflate %.3f ms, %zu chains completed, %zu segments made\n", M.pos.size(), M.kernel_ms,
                 el.size(), jobs.size(), c->stats.k_inflate_ms - infl0, chains, made);
  if (chains)
    if (int r = put_records(c->recs, merged)) return r;
  TMARK("scan: flush segments");
  return 0;
}

// where record r's original bytes lie, as an offset from d_file (StreamDev::orig_off, DiffJob::orig_off: the
// kernels add it to the file base): the stitched copy's 64-bit distance from d_file for a stitched record
static uint64_t rec_src(const atz_ctx* c, const Rec& r, const uint8_t* d_file) {
  return r.stitch == ~0ull ? r.offset : (uint64_t)(uintptr_t)c->d_stitch.p + r.stitch - (uint64_t)(uintptr_t)d_file;
}

// The scan's opt-in extensions (container, stitch, probe, segment): what ext_prepare lists before the scan for
// ext_merge to turn into records after it.  Every list is empty without its mask.
struct ScanExt {
  std::vector<RawCand> raw;
  StitchPlan stitch;
  ProbeList& probe;    // the context's (their storage is reused from call to call)
  MarkerList& marks;
  explicit ScanExt(atz_ctx* c) : probe(c->probe), marks(c->marks) {}
  // the records ext_merge can add: the sweep's tables have room for them (a marker adds one at the most)
  size_t extra_records() const { return raw.size() + stitch.cands.size() + probe.pos.size() + marks.pos.size(); }
};
static bool ext_on(const atz_ctx* c) { return ext_anchor_mask(c) || c->probe_mask || c->seg_mask; }

// the list kernels and the host parsers of the masks that are on
static int ext_prepare(atz_ctx* c, const uint8_t* h, const uint8_t* d_file, uint64_t F, ScanExt& E) {
  E.raw.clear(); E.stitch = StitchPlan{}; E.probe.pos.clear(); E.marks.pos.clear();
  c->st_off.clear(); c->st_len.clear();
  std::vector<uint64_t> anchors;
  if (int r = anchors_dev(c, d_file, F, ext_anchor_mask(c), anchors)) return r;   // (no mask: no anchor)
  if (int r = raw_candidates(h, F, anchors, E.raw)) return r;
  if (int r = stitch_candidates(h, F, anchors, E.stitch)) return r;
  if (c->probe_mask)
    if (int r = probe_dev(c, d_file, F, E.probe)) return r;
  if (c->seg_mask)
    if (int r = markers_dev(c, d_file, F, E.marks)) return r;
  return 0;
}

// The extensions' records merged into c->recs (the reference's, complete), each step seeing the records of the
// steps before it.  The decoded outputs go to the scan's arena, which is fresh for a step while no job ran
// before it: none of the scan's own (S.fjobs) and none of an earlier step's.  A step with candidates runs its
// jobs whether it accepts one or not, so its non-empty candidate list clears the flag.  (probe_merge goes through
// run_inflate_jobs even with no job.)
static int ext_merge(atz_ctx* c, const uint8_t* h, const uint8_t* d_file, uint64_t F, const ScanState& S, const ScanExt& E) {
  bool fresh = S.fjobs.empty();
  if (int r = raw_merge(c, h, d_file, S.arena_cap, fresh, E.raw)) return r;
  fresh = fresh && E.raw.empty();
  if (int r = stitch_merge(c, d_file, S.arena_cap, fresh, E.stitch)) return r;
  fresh = fresh && E.stitch.cands.empty();
  if (c->probe_mask)
    if (int r = probe_merge(c, d_file, F, S.arena_cap, fresh, E.probe)) return r;
  if (c->seg_mask)
    if (int r = seg_merge(c, h, d_file, F, E.marks)) return r;
  return 0;
}

// Every record, one piece.  (atz_scan; precompress_dev scans piece by piece while the sweep runs)
static int scan_impl(atz_ctx* c, const uint8_t* h, const uint8_t* d_file, uint64_t F) {
  auto t0 = std::chrono::steady_clock::now();
  c->recs.clear();
  ScanState S;
  if (int r = scan_plan(c, h, d_file, F, S)) return r;
  ScanExt E(c);
  if (int r = ext_prepare(c, h, d_file, F, E)) return r;
  c->recs.reserve(S.max_records() + E.extra_records());
  if (int r = scan_piece(c, h, d_file, S, 0, (uint32_t)S.chunks.size())) return r;
  if (int r = ext_merge(c, h, d_file, F, S, E)) return r;
  c->stats.scan_ms = ms_since(t0);
  return 0;
}

// Inflated bytes of records [r0, r1) (Phase 3's doInflate, main.cpp:431-453) into `slab`:
// c->infl_off[s] receives the absolute device address of stream s's bytes (the kernels take a null
// base), so the records of different pieces may live in different allocations.
static int inflate_records(atz_ctx* c, const uint8_t* d_file, uint64_t F, size_t r0, size_t r1, DBuf& slab) {
  auto tm_ = std::chrono::steady_clock::now();
  if (c->infl_off.size() < r1) c->infl_off.resize(r1);
  if (c->adler.size() < r1) c->adler.resize(r1);
  uint64_t tot = 0;
  std::vector<uint64_t> loc(r1 - r0);
  for (size_t s = r0; s < r1; s++) {
    const Rec& r = c->recs[s];
    if (r.offset + r.hull() > F) return ATZ_E_REF_UB;   // reads past EOF (uninitialised rBuffer)
    loc[s - r0] = tot;
    tot += (r.infl_len + 255) & ~255ull;
  }
  if (int r = slab.reserve(tot + 65536)) return r;
  const uint64_t base = (uint64_t)(uintptr_t)slab.p;
  // Streams whose scan decode kept its full output in the arena are copied; the others are
  // inflated again from the file with their exact length (doInflate, main.cpp:461-486) -- the
  // same bytes from the same offset, so both give the same result.
  std::vector<InfJob> jobs, raw_jobs, st_jobs, seg_jobs;
  std::vector<size_t> job_rec, raw_rec, st_rec, seg_rec;
  std::vector<Seg> segs;
  for (size_t s = r0; s < r1; s++) {
    const Rec& r = c->recs[s];
    c->infl_off[s] = base + loc[s - r0];
    if (r.arena_off != ~0ull) {
      segs.push_back({SEG_META, 0, r.arena_off, loc[s - r0], r.infl_len});
    } else {
      InfJob jb;
      jb.in_off = r.offset; jb.in_len = r.comp_len; jb.out_off = loc[s - r0]; jb.out_cap = r.infl_len;
      if (r.stitch != ~0ull) jb.in_off = r.stitch;   // (its input base is the stitch buffer)
      // (flags bit 7: a flush-terminated segment of the segment extension, which ends at its marker)
      const bool seg = r.type >= 24 && (r.flags & 128u);
      (r.stitch != ~0ull ? st_jobs : seg ? seg_jobs : r.type >= 24 ? raw_jobs : jobs).push_back(jb);
      (r.stitch != ~0ull ? st_rec : seg ? seg_rec : r.type >= 24 ? raw_rec : job_rec).push_back(s);
    }
  }
  if (!segs.empty()) {
    if (int r = upload(c, c->d_segs, segs.data(), segs.size() * sizeof(Seg))) return r;
    const uint32_t nseg = (uint32_t)segs.size();
    const uint32_t blocks = std::min<uint32_t>((nseg + 3) / 4, 65535u);
    kbeg(c, 3);
    hipLaunchKernelGGL(k_gather, dim3(blocks), dim3(256), 0, c->st, c->d_arena.as<uint8_t>(), nullptr, nullptr,
                       slab.as<uint8_t>(), c->d_segs.as<Seg>(), nseg);
    kend(c);
    KCHECK("k_gather");
  }
  TMARK("records: arena gather launch");
  std::vector<InfRes> res;
  if (int r = run_inflate_jobs(c, d_file, slab.as<uint8_t>(), jobs, res)) return r;
  if (!raw_jobs.empty()) {   // raw records (the container extension): the decoder without HEAD and CHECK
    std::vector<InfRes> rres;
    if (int r = run_inflate_jobs(c, d_file, slab.as<uint8_t>(), raw_jobs, rres, 0, false, true, true)) return r;
    jobs.insert(jobs.end(), raw_jobs.begin(), raw_jobs.end());
    job_rec.insert(job_rec.end(), raw_rec.begin(), raw_rec.end());
    res.insert(res.end(), rres.begin(), rres.end());
  }
  if (!seg_jobs.empty()) {   // flush-terminated segments (the segment extension): the decoder that stops at a marker
    std::vector<InfRes> gres;
    if (int r = run_inflate_jobs(c, d_file, slab.as<uint8_t>(), seg_jobs, gres, 0, false, true, INF_SEG)) return r;
    jobs.insert(jobs.end(), seg_jobs.begin(), seg_jobs.end());
    job_rec.insert(job_rec.end(), seg_rec.begin(), seg_rec.end());
    res.insert(res.end(), gres.begin(), gres.end());
  }
  if (!st_jobs.empty()) {   // stitched records (the stitch extension): from their contiguous copies
    std::vector<InfRes> sres;
    if (int r = run_inflate_jobs(c, c->d_stitch.as<uint8_t>(), slab.as<uint8_t>(), st_jobs, sres)) return r;
    jobs.insert(jobs.end(), st_jobs.begin(), st_jobs.end());
    job_rec.insert(job_rec.end(), st_rec.begin(), st_rec.end());
    res.insert(res.end(), sres.begin(), sres.end());
  }
  if (timing_on()) {
    uint64_t mx = 0, tot = 0;
    for (const InfJob& jb : jobs) { mx = std::max(mx, jb.in_len); tot += jb.in_len; }
    std::fprintf(stderr, "atz: records: %zu re-inflated (%llu input bytes, largest %llu)\n", jobs.size(),
                 (unsigned long long)tot, (unsigned long long)mx);
  }
  TMARK("records: re-inflate");
  for (size_t q = 0; q < jobs.size(); q++) {
    const size_t s = job_rec[q];
    if (res[q].status != INF_END) return ATZ_E_REF_ABORT;          // main.cpp:450-452
    if (res[q].produced != c->recs[s].infl_len || res[q].consumed != c->recs[s].comp_len) return ATZ_E_REF_UB;
  }
  c->stats.n_reinflated += jobs.size();
  for (size_t s = r0; s < r1; s++) {
    // Adler-32 of the inflated bytes = the verified trailer (atz_sweep: saved by atz_scan, whose
    // host buffer the caller need not keep alive)
    if (c->recs[s].type >= 24) { c->adler[s] = 0; continue; }   // a raw body has no trailer (TM_RAW trials write none)
    c->adler[s] = c->hfile ? rec_trailer(c->recs[s], c->hfile, c->st_off, c->st_len) : c->scan_trailer[s];
  }
  HIPCHK(hipStreamSynchronize(c->st));
  kcollect(c);
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Phase 3
// Hash buckets per (stream, memLevel), built on demand and cached for the sweep (8 bytes per
// position) in the context's DevArena chain_arena, up to CHAIN_CACHE_CAP.  Past the cap, a round
// builds its missing tables in its pipe's own d_chains (Pipe::tmp_chains), which forget_tmp_chains
// drops at the round's end.
static constexpr uint64_t CHAIN_CACHE_CAP = 48ull << 30;
static bool bucket_verify() {   // ATZ_BUCKETS_VERIFY=1 (read per call): check k_buckets_sort against the others
  const char* e = std::getenv("ATZ_BUCKETS_VERIFY");
  return e && std::atoi(e) != 0;
}
static constexpr uint32_t BSORT_MAX_NPAD = std::min<uint32_t>(65472u, ((160u * 1024u - 256u - BSORT_CNT_BYTES) / 2u) & ~63u);   // LDS limit (256 B static)
static_assert(bsort_lds_bytes(BSORT_MAX_NPAD) + 256u <= 160u * 1024u && BSORT_MAX_NPAD < 65536u, "k_buckets_sort LDS class");
static int ensure_chains_on(atz_ctx* x, Pipe* c, const std::vector<std::pair<uint32_t, int>>& need, ChainBufs& B);
// Builds the missing tables of `need` on the pipe's stream.
static int ensure_chains(atz_ctx* x, Pipe* c, const std::vector<std::pair<uint32_t, int>>& need) {
  return ensure_chains_on(x, c, need, c->cb);
}
// The deepest-bucket sizes (symbol replay's budget-free test) of pairs not known yet, without building
// their tables (k_bucket_depth; streams < 64 Ki positions, larger ones are never budget-free): a pair
// whose trials all turn out to be replays never needs its tables.  Runs on the pipe's stream.
// need_b[i]: the largest walk budget B of a trial on pair need[i] (budget-free: depth <= B).
// memLevels with the same hash shift s = (memLevel + 9) / 3 -- {1, 2}, {3, 4, 5}, {6, 7, 8}, {9} --
// hash a trigram to the same value (c0 << 2s) ^ (c1 << s) ^ c2 masked to memLevel + 7 bits, so a
// smaller memLevel's buckets are unions of a larger one's and its depth is at least theirs: a pair
// whose known lower bound already exceeds B cannot be budget-free and its depth is not computed
// (it stays unknown, which budget_free reads as "not budget-free").
static int ensure_depths(atz_ctx* x, Pipe* c, const std::vector<std::pair<uint32_t, int>>& need,
                         const std::vector<uint32_t>& need_b, DBuf& d_jobs) {
  if (!x->depth_pin.p) return 0;
  uint32_t* dp = x->depth_pin.as<uint32_t>();
  std::vector<ChainJob> byl[10];
  size_t tot = 0;
  for (size_t qi = 0; qi < need.size(); qi++) {
    const uint32_t s = need[qi].first;
    const int m = need[qi].second;
    const size_t i = 10 * (size_t)s + (size_t)m;
    if (dp[i] != ~0u || x->recs[s].infl_len >= 65536) continue;
    const int top = m <= 2 ? 2 : m <= 5 ? 5 : m <= 8 ? 8 : 9;
    uint32_t lb = 0;
    for (int m2 = m + 1; m2 <= top; m2++) {
      const uint32_t d = dp[10 * (size_t)s + (size_t)m2];
      if (d < 0xfffffffeu && d > lb) lb = d;
    }
    if (lb > need_b[qi]) continue;
    dp[i] = 0xfffffffeu;   // queued (the kernel overwrites it)
    ChainJob jb{};
    jb.infl_off = x->infl_off[s];
    jb.n = x->recs[s].infl_len;
    jb.memlevel = (uint32_t)m;
    jb.dslot = (uint32_t)i;
    byl[m].push_back(jb);
    tot++;
  }
  if (!tot) return 0;
  std::vector<ChainJob> all;
  all.reserve(tot);
  size_t beg[11] = {};
  for (int m = 0; m < 10; m++) { beg[m] = all.size(); all.insert(all.end(), byl[m].begin(), byl[m].end()); }
  beg[10] = all.size();
  if (int r = upload(c, d_jobs, all.data(), all.size() * sizeof(ChainJob))) return r;
  for (int m = 1; m < 10; m++) {
    const size_t cnt = beg[m + 1] - beg[m];
    if (!cnt) continue;
    kbeg(c, 2);
    hipLaunchKernelGGL(k_bucket_depth, dim3((uint32_t)cnt), dim3(BDEPTH_THREADS), 4u << (m + 6), c->st, INFL_BASE,
                       d_jobs.as<ChainJob>() + beg[m], (uint32_t)cnt, dp);
    kend(c);
    KCHECK("k_bucket_depth");
  }
  for (const ChainJob& jb : all) c->stats.k_chains_alg_bytes += jb.n;
  return 0;
}
// The kernels of one set of bucket jobs, writing at chains + job.chain_off.
static int build_bucket_jobs(atz_ctx* x, Pipe* c, ChainBufs& B, std::vector<ChainJob> jobs, uint32_t* chains,
                             bool use_sort, uint32_t* depth = nullptr) {
  // streams whose sort fits in LDS: k_buckets_sort (every memLevel), one launch per size class
  if (use_sort) {
    static const uint32_t cls[] = {4096, 8192, 12288, 16384, 20480, BSORT_MAX_NPAD};
    constexpr int NC = 6;
    std::vector<ChainJob> byc[NC], rest;
    for (const ChainJob& jb : jobs) {
      const uint64_t npad = (jb.n + 63) & ~63ull;
      int k = 0;
      while (k < NC && npad > cls[k]) k++;
      (k < NC ? byc[k] : rest).push_back(jb);
    }
    std::vector<ChainJob> all;
    size_t beg[NC + 1] = {};
    for (int k = 0; k < NC; k++) { beg[k] = all.size(); all.insert(all.end(), byc[k].begin(), byc[k].end()); }
    beg[NC] = all.size();
    if (!all.empty()) {
      if (int r = upload(c, B.d_cjobs2, all.data(), all.size() * sizeof(ChainJob))) return r;
      for (int k = 0; k < NC; k++) {
        const size_t cnt = beg[k + 1] - beg[k];
        if (!cnt) continue;
        // a wave keeps its tile in registers: bsort_chunks(class) batches of 64 positions
        static_assert(bsort_chunks(4096) == 4 && bsort_chunks(20480) == 20 && bsort_chunks(BSORT_MAX_NPAD) == 64, "classes");
        auto kern = k == 0 ? k_buckets_sort<4> : k == 1 ? k_buckets_sort<8> : k == 2 ? k_buckets_sort<12>
                  : k == 3 ? k_buckets_sort<16> : k == 4 ? k_buckets_sort<20> : k_buckets_sort<64>;
        kbeg(c, 2);
        hipLaunchKernelGGL(kern, dim3((uint32_t)cnt), dim3(BSORT_THREADS), bsort_lds_bytes(cls[k]), c->st,
                           INFL_BASE, B.d_cjobs2.as<ChainJob>() + beg[k], chains,
                           (uint32_t)cnt, depth);
        kend(c);
        KCHECK("k_buckets_sort");
      }
    }
    for (const ChainJob& jb : all) c->stats.k_chains_alg_bytes += 9 * jb.n;
    jobs.swap(rest);
    if (jobs.empty()) return 0;
  }
  // hash tables of memLevel <= 8 and streams < 64 Ki positions: LDS kernels; memLevel 9: HBM scratch
  std::vector<ChainJob> tiny, small, mid, big;
  for (const ChainJob& jb : jobs) {
    const uint32_t hs = 1u << (jb.memlevel + 7);
    (jb.n >= 65536 || hs > 32768 ? big : hs <= 4096 ? tiny : hs <= 16384 ? small : mid).push_back(jb);
  }
  {
    std::vector<ChainJob> all(tiny);
    all.insert(all.end(), small.begin(), small.end());
    all.insert(all.end(), mid.begin(), mid.end());
    if (!all.empty()) {
      if (int r = upload(c, B.d_cjobs2, all.data(), all.size() * sizeof(ChainJob))) return r;
      const ChainJob* dj = B.d_cjobs2.as<ChainJob>();
      auto launch = [&](auto kern, size_t off, size_t cnt, const char* nm) -> int {
        if (!cnt) return 0;
        kbeg(c, 2);
        hipLaunchKernelGGL(kern, dim3((uint32_t)cnt), dim3(256), 0, c->st, INFL_BASE, dj + off,
                           chains, (uint32_t)cnt);
        kend(c);
        KCHECK(nm);
        return 0;
      };
      if (int r = launch(k_buckets_lds<4096>, 0, tiny.size(), "k_buckets_lds<4096>")) return r;
      if (int r = launch(k_buckets_lds<16384>, tiny.size(), small.size(), "k_buckets_lds<16384>")) return r;
      if (int r = launch(k_buckets_lds<32768>, tiny.size() + small.size(), mid.size(), "k_buckets_lds<32768>")) return r;
    }
  }
  std::vector<ChainJob> nine, rest;   // memLevel 9 with n < 64 Ki: packed LDS counters + HBM bases
  for (const ChainJob& jb : big) ((jb.memlevel == 9 && jb.n < 65536) ? nine : rest).push_back(jb);
  big.swap(rest);
  if (!nine.empty()) {   // memLevel 9 on packed 16-bit LDS counters
    const size_t nbs = 4096;   // HBM scratch slots for the bucket bases, reused in launch order
    if (int r = B.d_heads2.reserve(nbs * 65536 * 4)) return r;
    std::vector<ChainJob>& pk = nine;
    for (size_t k = 0; k < pk.size(); k++) pk[k].slot = (uint32_t)(k % nbs);
    if (int r = upload(c, B.d_cjobs3, pk.data(), pk.size() * sizeof(ChainJob))) return r;
    for (size_t b0 = 0; b0 < pk.size();) {
      const size_t nb = std::min(nbs - b0 % nbs, pk.size() - b0);   // a launch never holds two jobs of one slot
      kbeg(c, 2);
      hipLaunchKernelGGL(k_buckets_pk<16>, dim3((uint32_t)nb), dim3(256), 0, c->st, INFL_BASE,
                         B.d_cjobs3.as<ChainJob>() + b0, chains, B.d_heads2.as<uint32_t>(),
                         (uint32_t)nb);
      kend(c);
      KCHECK("k_buckets_pk");
      b0 += nb;
    }
  }
  const size_t batch = 4096;   // scratch: 65536 x 8-byte words per job slot
  if (!big.empty() && (int)B.d_heads.reserve(batch * 65536 * 8)) return ATZ_E_NOMEM;
  for (size_t k = 0; k < big.size(); k++) big[k].slot = (uint32_t)(k % batch);
  if (int r = upload(c, B.d_cjobs, big.data(), big.size() * sizeof(ChainJob))) return r;
  for (size_t b0 = 0; b0 < big.size(); b0 += batch) {   // launches on one stream reuse the slots in order
    size_t nb = std::min(batch, big.size() - b0);
    kbeg(c, 2);
    hipLaunchKernelGGL(k_buckets, dim3((uint32_t)nb), dim3(64), 0, c->st, INFL_BASE,
                       B.d_cjobs.as<ChainJob>() + b0, chains, B.d_heads.as<uint64_t>(),
                       (uint32_t)nb);
    kend(c);
    KCHECK("k_buckets");
  }
  for (const ChainJob& jb : jobs) c->stats.k_chains_alg_bytes += 9 * jb.n;  // read I_s, write 8*I_s
  return 0;
}

// Tables go into the context's bucket cache (chain_arena, kept for the stream's later trials by any
// pipe); once it is full, into this pipe's d_chains for the current round only (forgotten by
// forget_tmp_chains at the round's end).  Tables are addressed absolutely (null chains base).
static void forget_tmp_chains(atz_ctx* x, Pipe* c) {
  for (auto& q : c->tmp_chains) x->chain_off[q.first][q.second] = ~0ull;
  c->tmp_chains.clear();
  c->chains_next = 0;
}
static int ensure_chains_on(atz_ctx* x, Pipe* c, const std::vector<std::pair<uint32_t, int>>& need, ChainBufs& B) {
  auto bytes = [&](uint32_t s) { return 8 * ((x->recs[s].infl_len + 63) & ~63ull); };
  std::vector<ChainJob> jobs;
  std::vector<size_t> tmp;   // jobs whose table goes into d_chains (offset relative to it, for now)
  uint64_t tmp_bytes = 0;
  for (auto& q : need) {
    uint32_t s = q.first;
    int m = q.second;
    if (x->chain_off[s][m] != ~0ull) continue;
    ChainJob jb;
    jb.infl_off = x->infl_off[s];
    jb.n = x->recs[s].infl_len;
    jb.memlevel = (uint32_t)m;
    jb.slot = 0;
    jb.dslot = 10 * s + (uint32_t)m;
    jb.pad_ = 0;
    const uint64_t a = x->chain_arena.alloc(bytes(s));
    if (a) {
      jb.chain_off = a >> 2;
    } else {
      jb.chain_off = tmp_bytes >> 2;
      tmp_bytes += (bytes(s) + 255) & ~255ull;
      tmp.push_back(jobs.size());
      c->tmp_chains.push_back({s, m});
    }
    x->chain_off[s][m] = jb.chain_off;   // (relative ones are rebased below)
    jobs.push_back(jb);
    c->diag_builds++;
  }
  if (jobs.empty()) return 0;
  if (!tmp.empty()) {   // the round's own tables (the pipe's earlier rounds are done with these buffers)
    if (c->chains_next == c->d_chains.size()) c->d_chains.emplace_back(new DBuf());
    DBuf& tb = *c->d_chains[c->chains_next++];
    if (int r = tb.reserve(tmp_bytes + 4096)) return r;
    const uint64_t base = (uint64_t)(uintptr_t)tb.p >> 2;
    for (size_t k : tmp) {
      jobs[k].chain_off += base;
      x->chain_off[(uint32_t)(jobs[k].dslot / 10)][jobs[k].memlevel] = jobs[k].chain_off;
    }
  }
  if (int r = build_bucket_jobs(x, c, B, jobs, CHAIN_BASE, true, x->depth_pin.as<uint32_t>())) return r;
  if (bucket_verify()) {
    // diagnostics (ATZ_BUCKETS_VERIFY=1): the same jobs again on the in-order kernels, compared
    uint64_t tot = 0;
    std::vector<ChainJob> alt(jobs);
    for (ChainJob& jb : alt) { jb.chain_off = tot; tot += 2 * ((jb.n + 63) & ~63ull); }
    DBuf tmp;
    if (int r = tmp.reserve(tot * 4 + 4096)) return r;
    if (int r = build_bucket_jobs(x, c, B, alt, tmp.as<uint32_t>(), false, nullptr)) return r;
    std::vector<uint32_t> h1(tot), h2(tot);
    for (size_t k = 0; k < jobs.size(); k++)
      HIPCHK(hipMemcpyAsync(h1.data() + alt[k].chain_off, (const void*)(uintptr_t)(jobs[k].chain_off << 2),
                            8 * ((jobs[k].n + 63) & ~63ull), hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(h2.data(), tmp.p, tot * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    for (size_t k = 0; k < jobs.size(); k++) {
      const uint64_t npad = (alt[k].n + 63) & ~63ull, nh = alt[k].n >= 3 ? alt[k].n - 2 : 0;
      const uint32_t* a = h1.data() + alt[k].chain_off;
      const uint32_t* b2 = h2.data() + alt[k].chain_off;
      uint64_t start = 0, deepest = 0;
      for (uint64_t i = 0; i < nh; i++) {
        if (a[i] != b2[i] || a[npad + i] != b2[npad + i]) {
          std::fprintf(stderr, "atz: bucket mismatch: job %zu n %llu m %u at %llu\n", k, (unsigned long long)alt[k].n,
                       alt[k].memlevel, (unsigned long long)i);
          return ATZ_E_INTERNAL;
        }
        if (b2[npad + i] & BUCKET_FIRST) start = i;
        deepest = std::max(deepest, i - start);
      }
      const uint32_t dsort = x->depth_pin.p ? x->depth_pin.as<uint32_t>()[jobs[k].dslot] : 0u;
      // the deepest bucket k_buckets_sort reported (symbol replay's test; ~0: a job past its LDS limit)
      if (x->depth_pin.p && nh && dsort != ~0u && dsort != deepest) {
        std::fprintf(stderr, "atz: deepest bucket mismatch: job %zu n %llu m %u: %u vs %llu\n", k,
                     (unsigned long long)alt[k].n, alt[k].memlevel, dsort, (unsigned long long)deepest);
        return ATZ_E_INTERNAL;
      }
    }
  }
  return 0;
}

// Whole match tables in the first pass for the memLevel a stream's first block names (k_inflate's
// INF_HINT_MLEV): that trial is the stream's likely winner, which otherwise parses past its prefix and
// runs again with the rest of its table.  Same-box A/B (gpurun_out/mh*, 2 runs each): C4 1504-1515 vs
// 1442-1491 MB/s (reruns 105 k -> 29 k, k_trial 648-663 -> 559-565 ms summed); 50 000 streams
// 1270-1315 vs 1279-1282; 25 000 947-968 vs 938-967; 12 500 669-673 vs 684-686 (a small sweep's rounds
// are latency-bound, and the hinted trials' whole tables lengthen the first pass).  So: sweeps of more
// than 16 000 streams (ATZ_MHINT=0 / 1 forces it off / on).  (Speculating through a hinted stream's
// list up to its next entry at the hinted memLevel measured slower: DESIGN.md s3.6.)
// A small sweep on six pipes (one rank's share at 8 GPUs) gains from it too (12 500 streams, same box,
// 3 runs each: 697-716 -> 741-776 MB/s; with the 3072 prefix floor 749-802), one on three pipes does not.
static bool big_sweep(const atz_ctx* x) { return x->recs.size() > 16000 || x->pipes_running >= 6; }
static bool mhint_on(const atz_ctx* x) {
  static const int v = [] { const char* e = std::getenv("ATZ_MHINT"); return e ? std::atoi(e) : -1; }();
  return v < 0 ? big_sweep(x) : v != 0;
}
// Match-table prefix for a trial that may stop early: enough positions for the blocks that decide
// the shortcut (~3 positions per symbol, lit_bufsize symbols per block); the rest on demand.  The
// floor covers the shortcut's 512 output bytes at memLevel 1-2, whose blocks hold 127-255 symbols: a
// floor of 1024 left 29 k memLevel 1-2 trials on C4 to run again with the rest of their table, 3072
// leaves none (same box, 3 runs each: 1521-1540 vs 1443-1454 MB/s; 6144 1463-1569; on another box
// 1497-1499 vs 1484-1488).  A small sweep's latency-bound rounds prefer the short first pass (12 500
// streams on three pipes: 663-687 with 3072 vs 700 with 1024), so the floor is 3072 where mhint_on
// applies, big_sweep (ATZ_PREFIX_MIN overrides).
static uint64_t match_prefix(uint64_t n, int memlevel, bool big) {   // 2 x lit_bufsize positions, floor
  static const uint64_t mul = [] { const char* e = std::getenv("ATZ_PREFIX_MUL"); return e ? (uint64_t)std::max(1, std::atoi(e)) : 2ull; }();
  static const uint64_t lo = [] { const char* e = std::getenv("ATZ_PREFIX_MIN"); return e ? (uint64_t)std::max(64, std::atoi(e)) : 0ull; }();
  const uint64_t floor = lo ? lo : big ? 3072 : 1024;
  return std::min(n, std::max<uint64_t>(floor, mul << (memlevel + 6)));
}

static uint32_t lazy_host(uint32_t level) {   // max_lazy of levels 7-9 (Z/deflate.c:141-143)
  return level == 7 ? 32u : level == 8 ? 128u : 258u;
}
static uint32_t nice_host(uint32_t level) {   // nice_length of levels 7-9
  return level == 7 ? 128u : 258u;
}
static uint64_t c_cfg_host(uint32_t level) {   // max_chain of a level (Z/deflate.c:131-143)
  static const uint16_t chain[10] = {0, 4, 8, 32, 16, 32, 128, 256, 1024, 4096};
  return chain[level < 10 ? level : 9];
}
// Every job runs on k_match_lds: the block stages the window its walks can touch (the stream bytes
// [p0 - MAX_DIST, p1 + 282) and their 16-bit prev[] chain: 3 bytes per staged position), one launch per
// size class so the dynamic LDS -- and with it the blocks per CU -- fits the class.  A job whose window
// exceeds the largest class (streams past 48 KiB: C3's PNG-like streams) is cut into position ranges of
// at most match_win() positions, each with its own window (<= 16320 + 282 + 32506 + 3 <= 49152 bytes).
// ATZ_MATCH_WIN=0 sends such jobs to k_match instead, which walks the buckets in HBM (the round-5 path).
static uint64_t match_win() {
  static const uint64_t v = [] { const char* e = std::getenv("ATZ_MATCH_WIN"); return e ? (uint64_t)std::atoll(e) : 16320ull; }();
  return v;
}
static uint64_t match_span(const MatchJob& m) {   // bytes k_match_lds stages for the job
  const uint64_t md = (1ull << m.window) - 262;
  const uint64_t lo = m.p0 > md ? (m.p0 - md) & ~3ull : 0ull;
  return std::min<uint64_t>(m.p1 + 258 + 24, m.n) - lo;
}
static int launch_match(atz_ctx* x, Pipe* c, const std::vector<MatchJob>& mj_in) {
  if (mj_in.empty()) return 0;
  static const uint64_t cls[] = {4096, 8192, 12288, 16384, 24576, 32768, 40960, 49152};
  constexpr int NC = 8;
  std::vector<MatchJob> cut;
  const bool win = match_win() > 0;
  if (win)
    for (const MatchJob& m : mj_in) {
      if (match_span(m) <= cls[NC - 1]) { cut.push_back(m); continue; }
      for (uint64_t a = m.p0; a < m.p1; a += std::min<uint64_t>(match_win(), 16320)) {
        MatchJob h = m;
        h.p0 = a;
        h.p1 = std::min<uint64_t>(m.p1, a + std::min<uint64_t>(match_win(), 16320));
        cut.push_back(h);
      }
    }
  const std::vector<MatchJob>& mj0 = win ? cut : mj_in;
  auto class_of = [&](const MatchJob& m) -> int {
    const uint64_t b = match_span(m);
    for (int k = 0; k < NC; k++) if (b <= cls[k] && (win || k < 6)) return k;
    return NC;
  };
  // one launch per class; within a launch the longest walks go first (LPT)
  auto group_of = [](int k) -> int { return k; };
  std::vector<MatchJob> mj;
  mj.reserve(mj0.size());
  size_t cnt[NC + 1] = {};
  int gmax[NC + 1];
  for (int k = 0; k <= NC; k++) gmax[k] = -1;
  for (const MatchJob& m : mj0) {
    const int k = class_of(m), g = group_of(k);
    cnt[g]++;
    gmax[g] = std::max(gmax[g], k);
  }
  size_t beg[NC + 2] = {};
  for (int k = 0; k <= NC; k++) beg[k + 1] = beg[k] + cnt[k];
  mj.resize(mj0.size());
  {
    size_t at[NC + 1];
    for (int k = 0; k <= NC; k++) at[k] = beg[k];
    for (const MatchJob& m : mj0) mj[at[group_of(class_of(m))]++] = m;
    auto work = [](const MatchJob& m) -> uint64_t {   // positions x expected chain length
      const uint64_t chain = std::min<uint64_t>(c_cfg_host(m.level), (m.p1 >> (m.memlevel + 7)) + 1);
      return (m.p1 - m.p0) * chain;
    };
    for (int k = 0; k <= NC; k++)
      std::stable_sort(mj.begin() + beg[k], mj.begin() + beg[k + 1],
                       [&](const MatchJob& a, const MatchJob& b) { return work(a) > work(b); });
  }
  if (int r = upload(c, c->d_mjobs, mj.data(), mj.size() * sizeof(MatchJob))) return r;
  for (int k = 0; k <= NC; k++) {
    if (!cnt[k]) continue;
    kbeg(c, 4);
    if (k < NC)
      hipLaunchKernelGGL(k_match_lds, dim3((uint32_t)cnt[k]), dim3(MATCH_THREADS), (uint32_t)(3 * cls[gmax[k]] + 64), c->st,
                         INFL_BASE, CHAIN_BASE, c->d_R.as<uint2>(),
                         c->d_mjobs.as<MatchJob>() + beg[k]);
    else
      hipLaunchKernelGGL(k_match, dim3((uint32_t)cnt[k]), dim3(256), 0, c->st, INFL_BASE,
                         CHAIN_BASE, c->d_R.as<uint2>(), c->d_mjobs.as<MatchJob>() + beg[k]);
    kend(c);
    KCHECK("k_match");
  }
  for (const MatchJob& m : mj) c->stats.k_match_positions += m.p1 - m.p0;
  return 0;
}

// Trials with small blocks (memLevel <= 2: lit_bufsize <= 256 symbols; <= 4 in small rounds, below) run
// on the multi-wave kernels (round 3, C4, same box, 2 runs each: 1302-1363 vs 1250-1264 MB/s without;
// the 12 500-stream file 574-593 vs 484-498)
// (k_trial_{fast,slow}_mw: one parse wave, MW_F flusher waves; k_deflate.hip MWSlot).  Their symbols
// stay in HBM for the whole stream (the flushers read each block at its own offset).
// Multi-wave trials up to memLevel Pipe::mw_cap: 2, or 4 for a round of a sweep with at most 16 000
// streams left (about: the pipe's batch times the pipes) -- one rank's share at 8 GPUs, the late rounds
// of a full file -- whose rounds wait for their slowest trials: a multi-wave trial ends sooner, at more
// cost.  ATZ_MW=m forces m (0: none; tests/test_gpu_knobs.py).
static uint32_t mw_cap_for(size_t n_streams) {
  static const int v = [] { const char* e = std::getenv("ATZ_MW"); return (int)(e ? std::max(0, std::min(9, std::atoi(e))) : -1); }();
  return v >= 0 ? (uint32_t)v : n_streams <= 16000 ? 4u : 2u;
}
static bool mw_trial(const Pipe* c, int kind, uint32_t memlevel) { return kind != 0 && memlevel <= c->mw_cap; }
// the kernel a trial of kind k runs on: bit 0 multi-wave, bits 1-2 its strategy (Trial::host & TH_STRAT:
// 1 Z_FILTERED on the slow kind, 3 Z_RLE / 2 Z_HUFFMAN_ONLY on the table-less kind 0)
// bit 3: the GNU deflater family (Trial::host & TH_GNU), always single-wave; bit 4: the flush-capable kernels
// (Trial::host & TH_FLUSH), default strategy, single- or multi-wave
static uint32_t trial_variant(const Pipe* c, int k, const Trial& t) {
  if (t.host & TH_GNU) return 8u;
  if (t.host & TH_FLUSH) return 16u | (mw_trial(c, k, t.memlevel) ? 1u : 0u);
  return (mw_trial(c, k, t.memlevel) ? 1u : 0u) | ((t.host & TH_STRAT) << 1);
}
// (a GNU-family trial's blocks hold up to 32 767 symbols whatever the stream's tables)
static uint64_t sym_words(const Pipe* c, int kind, const DeflSpec& p, uint64_t n) {   // symbol buffer of a trial (u32 units)
  if (p.gnu) return 32768 + 64;
  return (mw_trial(c, kind, (uint32_t)p.memlevel) ? n + 64 : 0) + (1ull << (p.memlevel + 6)) + 64;
}
// (deflateBound reads the memLevel a GNU-family trial does not have: it takes the general bound)
static uint64_t bound(uint64_t n, const DeflSpec& p) { return bound(n, p.window, p.gnu ? 0 : p.memlevel); }
static_assert(TM_RAW == 2 && TM_FLUSH == 64, "DeflSpec::mode() writes these bits");
// The trials of one batch on a pipe, by kind (0 stored, 1 fast, 2 slow levels), each with its slice of the
// pipe's output and symbol scratch.  Every trial descriptor is made here (Round, strategy_pass, deflate_dev).
struct TrialBatch {
  std::vector<Trial> tr[3];
  uint64_t out_tot = 0, sym_tot = 0;
  // the raw pass of a context with the segment mask: every default-strategy zlib trial goes to the flush-capable
  // kernels (TH_FLUSH), so that a list step's flush-terminated and finished trials share their launches
  bool flush_kernels = false;
  // A trial of stream s (len inflated bytes) with the parameters p and the mode bits p does not give (TM_FULL).
  // Z_RLE and Z_HUFFMAN_ONLY ignore the level and read no tables (the stored kind's kernels); Z_FILTERED
  // only changes deflate_slow, so on levels 1-3 it is the default strategy.  A GNU-family trial (level 1-9,
  // raw, default strategy: the callers' checks) parses at memLevel 8 and carries TH_GNU.
  // Returns (kind, index in tr[kind]).
  std::pair<int, uint32_t> add(const Pipe* c, uint32_t s, uint64_t len, const DeflSpec& p, uint8_t mode,
                               uint64_t best_ident) {
    const uint32_t strat = p.strategy == 1 && p.level < 4 ? 0 : p.strategy;
    const int kind = p.level == 0 || strat >= 2 ? 0 : p.level <= 3 ? 1 : 2;
    Trial t{};
    t.stream = s; t.clevel = (uint8_t)p.level; t.window = (uint8_t)p.window; t.memlevel = (uint8_t)p.table_memlevel();
    t.mode = mode | p.mode();
    t.host = strat | (p.gnu ? (uint32_t)TH_GNU : 0u) |
             (p.flush || (flush_kernels && p.raw && !strat && !p.gnu) ? (uint32_t)TH_FLUSH : 0u);
    t.best_ident = best_ident;
    t.out_off = out_tot; t.out_cap = bound(len, p) + 64 + (p.flush ? 5 : 0);
    out_tot += (t.out_cap + 255) & ~255ull;
    t.sym_off = sym_tot; sym_tot += sym_words(c, kind, p, len);
    tr[kind].push_back(t);
    return {kind, (uint32_t)tr[kind].size() - 1};
  }
  int reserve(Pipe* c) const {
    if (int r = c->d_out.reserve(out_tot + 4096)) return r;
    return c->d_syms.reserve(sym_tot * 4 + 4096);
  }
};

// A launch lasts as long as its slowest wave, so the trials go in longest-expected-first order
// (classic LPT): low memLevels mean many blocks (one tree build each), fast levels mean hole
// fallbacks, and the work grows with the stream.  Multi-wave trials lead each kind (a launch of their own).
// ATZ_STOPFLAG=0: speculative rounds without the stop flag (SweepArgs::stopj): every trial of a round
// runs to its own end
static bool stopflag_on() {
  static const bool v = [] { const char* e = std::getenv("ATZ_STOPFLAG"); return !e || std::atoi(e) != 0; }();
  return v;
}
static void trials_order(atz_ctx* x, const Pipe* c, std::vector<Trial>* in, TrialSet& S) {
  for (int k = 0; k < 3; k++) {
    const size_t n = in[k].size();
    S.perm[k].resize(n);
    // one 64-bit key per trial, sorted descending: multi-wave bit, the place in the round (stop flag),
    // expected work (< 2^38), then the index complemented (ties keep the caller's order, as a stable
    // sort would)
    std::vector<uint64_t> key(n);
    const uint32_t mwm = c->mw_cap;
    const bool packed = n < (1u << 20);
    bool strat = false;   // strategy trials among them
    for (size_t q = 0; q < n; q++) {
      const Trial& t = in[k][q];
      strat |= (t.host & (TH_STRAT | TH_GNU | TH_FLUSH)) != 0;
      const uint64_t w = x->recs[t.stream].infl_len * (uint64_t)(k == 1 ? 3 : 1) * (uint64_t)(10 - t.memlevel) *
                         (uint64_t)((t.mode & TM_REPLAY) ? 1 : 4);   // replays skip the match walks
      const uint64_t mw = k != 0 && t.memlevel <= mwm;
      // with the stop flag, a stream's earlier trials of the round first: a stop they find ends the later
      // ones
      const uint64_t jr = stopflag_on() ? 15 - std::min<uint32_t>(t.spec_j, 15) : 0;
      key[q] = packed ? (mw << 63) | (jr << 59) | (std::min<uint64_t>(w, (1ull << 39) - 1) << 20) | ((1u << 20) - 1 - q) : w;
      S.perm[k][q] = (uint32_t)q;
    }
    if (packed) {
      std::sort(key.begin(), key.end(), std::greater<uint64_t>());
      for (size_t q = 0; q < n; q++) S.perm[k][q] = (uint32_t)((1u << 20) - 1 - (key[q] & ((1u << 20) - 1)));
    } else {
      std::stable_sort(S.perm[k].begin(), S.perm[k].end(), [&](uint32_t a, uint32_t b) {
        const bool ma = mw_trial(c, k, in[k][a].memlevel), mb = mw_trial(c, k, in[k][b].memlevel);
        return ma != mb ? ma : key[a] > key[b];
      });
    }
    // strategy and GNU-family trials run on kernels of their own: one run per variant, in the order above
    if (strat)
      std::stable_sort(S.perm[k].begin(), S.perm[k].end(), [&](uint32_t a, uint32_t b) {
        return trial_variant(c, k, in[k][a]) < trial_variant(c, k, in[k][b]);
      });
    S.tr[k].resize(n);
    for (size_t q = 0; q < n; q++) S.tr[k][q] = in[k][S.perm[k][q]];
    S.res[k].clear();
  }
  S.base = 0;
}
// the trial kernels over h[0, cnt) (one kind, multi-wave ones first), at slots [base, base + cnt)
static int trials_launch(atz_ctx* x, Pipe* c, const uint8_t* d_cmp, const SweepOpts& so, int k, const Trial* h,
                         size_t cnt, size_t base) {
  // the trial kernels by (kind, strategy, multi-wave); no row: no such trial.  (The rows' order is the
  // order in which the templates are instantiated, and so the kernels' order in the code object.)
  struct Kern { int kind; uint32_t strat; bool mw; void (*fn)(SweepArgs); const char* name; };
  static const Kern kerns[] = {
      {0, 0, false, k_trial_stored, "k_trial_stored"},
      {0, 2, false, k_trial_huff, "k_trial_huff"},
      {0, 3, false, k_trial_rle, "k_trial_rle"},
      {1, 0, true, k_trial_fast_mw<BITMAP_BITS>, "k_trial_fast"},
      {1, 0, false, k_trial_fast<BITMAP_BITS>, "k_trial_fast"},
      {2, 0, true, k_trial_slow_mw, "k_trial_slow"},
      {2, 0, false, k_trial_slow, "k_trial_slow"},
      {2, 1, true, k_trial_slow_filt_mw, "k_trial_slow_filt"},
      {2, 1, false, k_trial_slow_filt, "k_trial_slow_filt"},
      {1, 4, false, k_trial_fast_gnu, "k_trial_fast_gnu"},   // (strat 4: trial_variant's bit 3, the GNU family)
      {2, 4, false, k_trial_slow_gnu, "k_trial_slow_gnu"},
      {0, 8, false, k_trial_stored_flush, "k_trial_stored_flush"},   // (strat 8: trial_variant's bit 4, TH_FLUSH)
      {1, 8, true, k_trial_fast_flush_mw, "k_trial_fast_flush"},
      {1, 8, false, k_trial_fast_flush, "k_trial_fast_flush"},
      {2, 8, true, k_trial_slow_flush_mw, "k_trial_slow_flush"},
      {2, 8, false, k_trial_slow_flush, "k_trial_slow_flush"},
  };
  for (size_t i = 0; i < cnt; i++)   // a waiting trial or a duplicate never reaches a launch
    if (h[i].host & (TH_WAITS | TH_DUP)) return ATZ_E_INTERNAL;
  // the trial descriptors first, then the launches
  for (size_t i = 0; i < cnt;) {
    const bool mw = mw_trial(c, k, h[i].memlevel);
    size_t j = i + 1;
    while (j < cnt && mw_trial(c, k, h[j].memlevel) == mw) j++;
    HIPCHK(pipe_copy(c, c->d_trials.as<Trial>() + base + i, h + i, (j - i) * sizeof(Trial), hipMemcpyHostToDevice));
    i = j;
  }
  auto launch1 = [&](const Trial* hh, size_t n1, size_t b1, uint32_t variant) -> int {
    (void)hh;
    const bool mw = variant & 1u;
    const Kern* kn = nullptr;
    for (const Kern& e : kerns)
      if (e.kind == k && e.strat == variant >> 1 && e.mw == mw) kn = &e;
    if (!kn) return ATZ_E_INTERNAL;
    SweepArgs A;
    A.file = d_cmp; A.infl = INFL_BASE; A.chains = CHAIN_BASE;
    A.R = c->d_R.as<uint2>();
    A.streams = x->d_streams.as<StreamDev>(); A.trials = c->d_trials.as<Trial>() + b1;
    A.res = c->d_tres.as<TrialRes>() + b1; A.out = c->d_out.as<uint8_t>(); A.syms = c->d_syms.as<uint32_t>();
    A.adler = x->d_adler.as<uint32_t>(); A.o = so; A.ntrials = (uint32_t)n1;
    A.stopj = c->stopj_cur;
    dim3 g((uint32_t)n1), b(mw ? MW_THREADS : 64);
    kbeg(c, variant & 8u ? 5 : 0);
    hipLaunchKernelGGL(kn->fn, g, b, 0, c->st, A);
    kend(c);
    KCHECK(kn->name);
    return 0;
  };
  size_t i = 0;
  while (i < cnt) {   // runs of equal multi-wave-ness (and strategy): trials_order made them contiguous
    const uint32_t v = trial_variant(c, k, h[i]);
    size_t j = i + 1;
    while (j < cnt && trial_variant(c, k, h[j]) == v) j++;
    if (int r = launch1(h + i, j - i, base + i, v)) return r;
    i = j;
  }
  return 0;
}
// ATZ_EARLY=0: every first-pass match table waits for the round's plan (Round::plan)
static bool early_match_on() {
  static const bool v = [] { const char* e = std::getenv("ATZ_EARLY"); return !e || std::atoi(e) != 0; }();
  return v;
}
// A trial's match table in the round's d_R (c->r_next on) and its first pass: whole where the trial must
// parse the whole stream, and for the memLevel the stream's first block names (its likely winner: no
// rerun with the rest of the table); else a prefix.  Sets t.r_off and t.x_lim.
static MatchJob first_match_job(atz_ctx* x, Pipe* c, int k, Trial& t) {
  const uint64_t n = x->recs[t.stream].infl_len;
  t.r_off = c->r_next;
  c->r_next += ((n + 63) & ~63ull) + 256;   // + the double-buffered window's over-read
  t.x_lim = (t.mode & TM_FULL) || (mhint_on(x) && t.memlevel == x->recs[t.stream].mhint) ? n : match_prefix(n, t.memlevel, big_sweep(x));
  MatchJob m{};
  m.infl_off = x->infl_off[t.stream]; m.n = n; m.chain_off = t.chain_off; m.r_off = t.r_off;
  m.p0 = 0; m.p1 = t.x_lim; m.level = t.clevel; m.window = t.window; m.fast = k == 1; m.memlevel = t.memlevel;
  return m;
}
// The launches of a first pass (match tables, trials); results at d_tres + bases[k] in launch order.
// Match tables go into d_R from c->r_next on (reset by the caller: Round, run_trials); a trial whose
// x_lim is set already has its first-pass table (launched early by Round::plan).
static int trials_first_launch(atz_ctx* x, Pipe* c, const uint8_t* d_cmp, TrialSet& S, const SweepOpts& so,
                               size_t bases[3]) {
  std::vector<Trial>* tr = S.tr;
  std::vector<TrialRes>* res = S.res;
  std::vector<MatchJob> mj;
  for (int k = 0; k < 3; k++)
    for (const Trial& t : tr[k])
      if (x->recs[t.stream].infl_len >= (1ull << 31)) {   // trial kernels keep 32-bit positions
        std::fprintf(stderr, "atz: stream of %llu inflated bytes exceeds the 2 GiB trial limit\n",
                     (unsigned long long)x->recs[t.stream].infl_len);
        return ATZ_E_ARG;
      }
  for (int k = 1; k < 3; k++)
    for (Trial& t : tr[k]) {
      const uint64_t n = x->recs[t.stream].infl_len;
      if (tm_unchecked_replay(t.mode)) { t.r_off = 0; t.x_lim = n; continue; }   // unchecked replays: no match table
      if (t.x_lim) continue;   // its table's first pass is already launched (Round::plan)
      if (MatchJob m = first_match_job(x, c, k, t); m.p1 > m.p0) mj.push_back(m);
    }
  if (int r = c->d_R.reserve(c->r_next * sizeof(uint2) + 4096)) return r;
  c->lap(6);
  if (int r = launch_match(x, c, mj)) return r;
  c->lap(7);
  const size_t tot_trials = tr[0].size() + tr[1].size() + tr[2].size();
  if (int r = c->d_trials.reserve(2 * tot_trials * sizeof(Trial) + 64)) return r;
  if (int r = c->d_tres.reserve(2 * tot_trials * sizeof(TrialRes) + 64)) return r;
  size_t base = 0;
  for (int k = 0; k < 3; k++) {
    bases[k] = base;
    res[k].resize(tr[k].size());
    if (tr[k].empty()) continue;
    if (int r = trials_launch(x, c, d_cmp, so, k, tr[k].data(), tr[k].size(), base)) return r;
    base += tr[k].size();
  }
  S.base = base;
  c->lap(8);
  return 0;
}
// First pass: match-table prefixes, every trial once, results read back.  Chain tables must exist.
static int trials_first_finish(Pipe* c, TrialSet& S, const size_t bases[3]);
static int trials_first(atz_ctx* x, Pipe* c, const uint8_t* d_cmp, TrialSet& S, const SweepOpts& so) {
  size_t bases[3];
  if (int r = trials_first_launch(x, c, d_cmp, S, so, bases)) return r;
  return trials_first_finish(c, S, bases);
}
// a first pass's results read back (after trials_first_launch)
static int trials_first_finish(Pipe* c, TrialSet& S, const size_t bases[3]) {
  std::vector<Trial>* tr = S.tr;
  std::vector<TrialRes>* res = S.res;
  for (int k = 0; k < 3; k++)
    if (!tr[k].empty())
      HIPCHK(pipe_copy(c, res[k].data(), c->d_tres.as<TrialRes>() + bases[k], tr[k].size() * sizeof(TrialRes), hipMemcpyDeviceToHost));
  HIPCHK(pipe_sync(c));
  kcollect(c);
  c->lap(9);
  return 0;
}
// Reruns: the TR_NEED_R trials for which want(trial) holds get the rest of their match table and run
// again (their r_off region keeps the prefix).  The others keep TR_NEED_R.
static int trials_rerun(atz_ctx* x, Pipe* c, const uint8_t* d_cmp, TrialSet& S, const SweepOpts& so,
                        const std::function<bool(const Trial&)>& want) {
  std::vector<Trial>* tr = S.tr;
  std::vector<TrialRes>* res = S.res;
  std::vector<Trial> again[3];
  std::vector<size_t> where[3];
  std::vector<MatchJob> mj;
  for (int k = 1; k < 3; k++)
    for (size_t q = 0; q < tr[k].size(); q++) {
      if (res[k][q].state != TR_NEED_R || (want && !want(tr[k][q]))) continue;
      Trial t = tr[k][q];
      const uint64_t n = x->recs[t.stream].infl_len;
      MatchJob m{};
      m.infl_off = x->infl_off[t.stream]; m.n = n; m.chain_off = t.chain_off; m.r_off = t.r_off;
      m.p0 = t.x_lim; m.p1 = n; m.level = t.clevel; m.window = t.window; m.fast = k == 1; m.memlevel = t.memlevel;
      if (m.p1 > m.p0) mj.push_back(m);
      t.x_lim = n;
      again[k].push_back(t);
      where[k].push_back(q);
      c->stats.n_trials_rerun++;
    }
  if (again[1].empty() && again[2].empty()) return 0;
  // (slots past the first pass's: d_trials / d_tres hold 2 x the set)
  if (int r = launch_match(x, c, mj)) return r;
  std::vector<TrialRes> rr[3];
  size_t base = S.base, bases[3] = {0, 0, 0};
  if (base + again[1].size() + again[2].size() > 2 * (tr[0].size() + tr[1].size() + tr[2].size())) return ATZ_E_INTERNAL;
  for (int k = 1; k < 3; k++) {
    bases[k] = base;
    if (again[k].empty()) continue;
    if (int r = trials_launch(x, c, d_cmp, so, k, again[k].data(), again[k].size(), base)) return r;
    rr[k].resize(again[k].size());
    base += again[k].size();
  }
  for (int k = 1; k < 3; k++)
    if (!again[k].empty())
      HIPCHK(pipe_copy(c, rr[k].data(), c->d_tres.as<TrialRes>() + bases[k], again[k].size() * sizeof(TrialRes), hipMemcpyDeviceToHost));
  HIPCHK(pipe_sync(c));
  kcollect(c);
  for (int k = 1; k < 3; k++)
    for (size_t q = 0; q < again[k].size(); q++) {
      if (rr[k][q].state == TR_NEED_R) return ATZ_E_INTERNAL;
      res[k][where[k][q]] = rr[k][q];
      tr[k][where[k][q]].x_lim = again[k][q].x_lim;
    }
  S.base = base;
  return 0;
}
// results in the caller's order
static void trials_results(const TrialSet& S, std::vector<TrialRes>* res) {
  for (int k = 0; k < 3; k++) {
    res[k].resize(S.tr[k].size());
    for (size_t q = 0; q < S.tr[k].size(); q++) res[k][S.perm[k][q]] = S.res[k][q];
  }
}
// Runs the trials tr[k] to completion (first pass, then every rerun); res[k] receives their results.
static int run_trials(atz_ctx* x, Pipe* c, const uint8_t* d_cmp, std::vector<Trial>* tr, const SweepOpts& so,
                      std::vector<TrialRes>* res) {
  TrialSet S;
  trials_order(x, c, tr, S);
  c->r_next = 0;
  if (int r = trials_first(x, c, d_cmp, S, so)) return r;
  if (int r = trials_rerun(x, c, d_cmp, S, so, nullptr)) return r;
  trials_results(S, res);
  return 0;
}

// ATZ_REPLAY=0 disables symbol replay (every trial parses); 2 saves sequences but never replays them,
// 3 replays only between budget-free trials (diagnostics)
static int replay_mode() {
  static const int v = [] { const char* e = std::getenv("ATZ_REPLAY"); return (int)(e ? std::atoi(e) : 1); }();
  return v;
}
static bool replay_on() { return replay_mode() != 0; }
static constexpr uint64_t RP_ARENA_CAP = 24ull << 30;   // saved sequences, all pipes

// a trial replays entry e's saved sequence: unchecked if budget-free, else against the saved reads
// ATZ_DEDUP=0: launch duplicate trials anyway (diagnostics)
static bool dedup_on() {
  static const int v = [] { const char* e = std::getenv("ATZ_DEDUP"); return (int)(e ? std::atoi(e) : 1); }();
  return v != 0;
}
// A budget-free replay whose saved sequence fits one block of both its own and the saver's
// lit_bufsize (at most lit_bufsize - 2 symbols: with lit_bufsize - 1 the tally flushes a block and the
// end adds an empty final one) compresses to the saver's bytes: same symbols, same single block,
// same header (level, window).  Its result can then only equal the saver's, which the stream's rule
// already applied without stopping, so it is not launched (TH_DUP; TR_CANT_BEAT on the host).
static void replay_from(Trial& t, const RpEntry& e, bool bf) {
  if (bf) {
    t.mode |= TM_REPLAY;
    const uint32_t lm = std::min<uint32_t>(e.memlevel, t.memlevel);
    if (dedup_on() && (uint64_t)e.nsym + 2 <= (1ull << (lm + 6))) t.host |= TH_DUP;
  } else if (e.tab) {
    t.mode |= TM_REPLAY | TM_CHECKED;
    t.rp_tab = e.tab;
  } else {
    return;
  }
  t.rp_syms = e.addr; t.rp_nsym = e.nsym; t.rp_flags = e.flags;
}
static bool budget_free(atz_ctx* x, int kind, const Trial& t) {
  const uint32_t Bq = (uint32_t)(c_cfg_host(t.clevel) >> (kind == 1 ? 0 : 2));
  return x->depth_pin.as<uint32_t>()[10 * (size_t)t.stream + t.memlevel] <= Bq;
}
// Budget-free AND memLevel-free: a node at distance exactly MAX_DIST is walked when it is the hash
// head (deflate_fast / deflate_slow test strstart - hash_head <= MAX_DIST) but not as a chain
// successor (longest_match continues only while cur_match > strstart - MAX_DIST, Z/deflate.c:1227),
// so whether it is visited depends on which other trigrams share its bucket, i.e. on the memLevel.
// Replays across memLevels are therefore exact only for streams in which no candidate can sit at
// that distance (n <= MAX_DIST); levels at one memLevel (level_dups) share the buckets and are not
// affected.  (Found on the C5 workload: w13 streams of 13-16 KB.)
static bool replay_free(atz_ctx* x, int kind, const Trial& t) {
  return x->recs[t.stream].infl_len <= (1ull << t.window) - 262 && budget_free(x, kind, t);
}

// Cross-level duplicates.  Levels 7, 8 and 9 write the same zlib header (FLEVEL 3) and differ only in
// good_length, max_lazy, nice_length and max_chain (Z/deflate.c:141-143).  When both levels are
// budget-free at the stream's (window, memLevel) -- every walk visits all its same-trigram nodes,
// under either budget, so good_length has no effect -- a level-L' trial parses exactly like an
// earlier level-L trial there if, over what that trial parsed, no read length reached L''s
// nice_length (its walks would stop no earlier) and no lazy read improved a match of length >= L''s
// max_lazy (the reads L' skips are ones that did not change the parse).  Same symbols, same
// blocks, same header: the output, and so the result, is the earlier trial's, which the stream's
// rule already applied without stopping.  Such a trial is not launched (TH_DUP).
static bool budget_free(atz_ctx* x, int kind, const Trial& t);
static void level_dups(atz_ctx* x, std::vector<StreamState>& ss, std::vector<Trial>& slow) {
  for (Trial& t : slow) {
    if (t.clevel < 7 || t.clevel > 9 || (t.mode & TM_FULL)) continue;
    const StreamState& st = ss[t.stream];
    for (const auto& r : st.xl) {
      // only a twin at a higher level: its lazy/nice bounds (main.cpp:739-745 lists levels descending)
      // are at least this level's, so it made every read this level would; r[2] < L proves nothing
      if (r[0] != t.window || r[1] != t.memlevel || r[2] <= t.clevel) continue;
      if (r[3] < lazy_host(t.clevel) && r[4] < nice_host(t.clevel) && budget_free(x, 2, t)) t.host |= TH_DUP;
      break;
    }
  }
}
// after a round: what the budget-free level-7-9 trials that ran parsed (a replay parsed its saver's
// whole sequence)
// (streams for which mine(stream) holds)
template <class Mine>
static void level_record(atz_ctx* x, std::vector<StreamState>& ss, const std::vector<Trial>& slow,
                         const std::vector<TrialRes>& res, const Mine& mine) {
  for (size_t q = 0; q < slow.size(); q++) {
    const Trial& t = slow[q];
    const TrialRes& r = res[q];
    if (!mine(t.stream)) continue;
    if (t.clevel < 7 || t.clevel > 9 || (t.host & TH_DUP) || r.state == TR_NEED_R || r.state == TR_OVERFLOW ||
        r.state == TR_SKIPPED)
      continue;
    if (!budget_free(x, 2, t)) continue;
    StreamState& st = ss[t.stream];
    bool have = false;
    for (const auto& e : st.xl) have |= e[0] == t.window && e[1] == t.memlevel;
    if (have) continue;
    uint32_t rm = r.reads_max;
    if (r.saved_flags & 4) {   // a replay: its saver's reads
      if (st.rp < 0) continue;
      rm = x->rp_pool[st.rp][t.clevel - 1].reads_max;
    }
    st.xl.push_back({(uint16_t)t.window, (uint16_t)t.memlevel, (uint16_t)t.clevel, (uint16_t)(rm >> 16),
                     (uint16_t)(rm & 0xffffu)});
  }
}

// Symbol replay (trial_body).  A trial at level L, window w, memLevel m whose deepest bucket holds at
// most B + 1 positions is "budget-free": its walks cannot reach their budget, so they walk exactly
// like those of every other budget-free memLevel (B = max_chain for deflate_fast, levels 1-3, whose
// prev_length stays below good_match; max_chain / 4 for deflate_slow, its budget after a good match).
// The first budget-free trial at (L, w) of a stream whose window never slides saves its symbol
// sequence (slow levels: and the match-table entries its parse read).  Once a complete sequence is
// saved, the stream's later trials at (L, w) replay it: unchecked when budget-free too, else (slow
// levels) only if their own table agrees on those entries, which the kernel checks before parsing.
static void plan_replay(atz_ctx* x, Pipe* c, std::vector<StreamState>& ss, int kind, std::vector<Trial>& trs,
                        std::vector<std::array<uint32_t, 4>>& savers) {
  const bool checked = replay_mode() != 3 && kind == 2;   // ATZ_REPLAY=3: budget-free replays only
  for (size_t q = 0; q < trs.size(); q++) {
    Trial& t = trs[q];
    if (t.clevel < 1 || t.clevel > 9 || (t.mode & TM_FULL) || (t.host & TH_DUP)) continue;
    const uint64_t n = x->recs[t.stream].infl_len;
    const uint64_t wsz = 1ull << t.window;
    if (n > wsz + (wsz - 262)) continue;                                  // the window may slide
    const bool bf = replay_free(x, kind, t);
    if (!bf && !checked) continue;
    StreamState& st = ss[t.stream];
    const uint32_t L = t.clevel;
    const bool saved = (st.rp_saved >> L) & 1u, busy = (st.rp_busy >> L) & 1u;   // entry state 2 / 1 (else 0)
    const bool same_w = st.rp_win[L] == t.window;
    if (saved && same_w) {
      if (replay_mode() == 2) continue;
      replay_from(t, x->rp_pool[st.rp][L - 1], bf);
    } else if (busy && same_w && replay_mode() != 2 && (bf || x->rp_pool[st.rp][L - 1].tab)) {
      t.host |= TH_WAITS;   // its saver runs in this round: wait for it (second launch of the round)
    } else if (!saved && !busy && bf) {
      if (st.rp < 0) {   // the pool holds one entry per stream at most: never past its reserve
        std::lock_guard<std::mutex> lk(x->rp_mu);
        if (x->rp_pool.size() == x->rp_pool.capacity()) continue;
        st.rp = (int32_t)x->rp_pool.size();
        x->rp_pool.emplace_back();
      }
      RpEntry& e = x->rp_pool[st.rp][L - 1];
      const uint64_t sb = (4 * (n + 64) + 255) & ~255ull, tb = kind == 2 ? ((8 * n + 255) & ~255ull) : 0;
      if (!e.addr) {
        e.addr = x->rp_arena.alloc(sb + tb);
        if (!e.addr) continue;
        e.tab = tb ? e.addr + sb : 0;
      }
      e.state = 1;
      e.window = t.window;
      e.memlevel = t.memlevel;
      st.rp_busy |= (uint16_t)(1u << L);
      st.rp_win[L] = t.window;
      t.mode |= TM_SAVE;
      t.rp_syms = e.addr;
      if (e.tab) { t.mode |= TM_SAVE_TAB; t.rp_tab = e.tab; }
      savers.push_back({(uint32_t)kind, (uint32_t)q, (uint32_t)st.rp, (uint32_t)(t.clevel - 1)});   // indices: rp_pool may grow
    }
  }
}

// Trials that cannot make their stream recompressible.  The ATZ1 records a stream only if its best
// trial differs from the original in at most recomp_tresh bytes (main.cpp:454), so a trial whose
// mismatches already exceed recomp_tresh (ident <= C - recomp_tresh - 1 whatever follows) changes the
// file only through the stream's running best ident -- and it cannot change that either:
//  * every recompressible trial's ident exceeds every such trial's, so the recompressible
//    improvements (and with them the chosen c, w, m and the diffs) are the same with or without it;
//  * with mismatch_tol <= recomp_tresh it cannot meet the stop rule (ident + tol >= C, main.cpp:700),
//    nor change the brute-window test (C - ident >= tol, main.cpp:590: true either way).
// So such a trial may stop as soon as its mismatches pass recomp_tresh: its best_ident is raised to
// C - recomp_tresh - 1 and the kernels' "cannot beat" exit does the rest (early_exit).  Only the
// reference's unobservable ident / c, w, m of streams it does not recompress change, which is why
// atz_sweep (which reports them) keeps the exact rule.  Symbol-saving trials keep it too: their
// whole sequence serves the stream's replays.  ATZ_ELIG=0 turns it off (tests/test_gpu_knobs.py).
static uint64_t elig_floor(const atz_ctx* x, uint64_t C) {
  static const bool on = [] { const char* e = std::getenv("ATZ_ELIG"); return !e || std::atoi(e) != 0; }();
  if (!on || x->exact_idents || x->o.mismatch_tol > x->o.recomp_tresh || C <= x->o.recomp_tresh) return 0;
  return C - x->o.recomp_tresh - 1;
}

// match tables + output scratch of one round, over all pipes
static constexpr uint64_t ROUND_BUDGET_BYTES = 24ull << 30;

// Sweep scheduling.  Every pipe sweeps a fixed interleaved share of the streams (sweep_publish), all
// of them in every round: it takes its queue (sched_take), runs one round on it (each stream's next K
// trials: tables, trial launches, the reference's rule per stream; a trial that parsed past its
// match-table prefix, TR_NEED_R, is rerun with its whole table inside the round, before its stream's
// rule walk goes on) and hands back the streams that have not stopped (sched_give).  Measured and not
// kept: one queue shared by the pipes with each stream's next step as soon as its own
// round is done, a done pipe taking part of another's share, whole match tables for speculative rounds.
// Pipe g's next batch into `batch` (false: the sweep is over for this pipe).
static bool sched_take(atz_ctx* x, int g, std::vector<uint32_t>& batch) {
  auto& Q = x->sched;
  std::unique_lock<std::mutex> lk(Q.mu);
  batch.clear();
  auto stop = [&] { return Q.abort || x->sweep_abort.load(std::memory_order_relaxed); };
  std::deque<uint32_t>& q = Q.q[g];
  Q.cv.wait(lk, [&] { return stop() || !q.empty() || (Q.closed && Q.unfinished[g] == 0); });
  if (stop() || q.empty()) return false;
  batch.assign(q.begin(), q.end());
  q.clear();
  return true;
}
// After a round: the batch's streams that have not stopped go back (`waiting`, which the round's
// budget left out, first).
static void sched_give(atz_ctx* x, int g, const std::vector<StreamState>& ss, const std::vector<uint32_t>& active,
                       const std::vector<uint32_t>& waiting) {
  auto& Q = x->sched;
  std::lock_guard<std::mutex> lk(Q.mu);
  std::vector<uint32_t> front(waiting);
  size_t done = 0;
  for (uint32_t s : active) { if (ss[s].phase == 2) done++; else front.push_back(s); }
  Q.unfinished[g] -= done;
  Q.q[g].insert(Q.q[g].begin(), front.begin(), front.end());
  Q.cv.notify_all();
}
static void sched_abort(atz_ctx* x) {
  std::lock_guard<std::mutex> lk(x->sched.mu);
  x->sched.abort = true;
  x->sched.cv.notify_all();
}

static size_t round_target(const atz_ctx* x);
// Per-trial counters of pipe c (per kind x level: count, cycles total/tree/emit/heap/fallback, parsed
// bytes, symbols, scan/send cycles, parse window phases) and the algorithmic bytes.
static void account_trial(atz_ctx* x, Pipe* c, int k, const Trial& t, const TrialRes& r) {
  const uint64_t C = x->recs[t.stream].comp_len;
  c->stats.trial_parsed_bytes += r.parsed;
  c->stats.n_fast_fallbacks += r.fallbacks & 0xffffffffull;
  c->stats.n_fast_restarts += r.fallbacks >> 32;
  c->stats.n_trials_skipped += r.state == TR_SKIPPED;
  c->stats.trial_cyc_total += r.cyc_total; c->stats.trial_cyc_tree += r.cyc_tree;
  c->stats.trial_cyc_emit += r.cyc_emit; c->stats.trial_blocks += r.blocks;
  c->stats.trial_cyc_heap += r.cyc_heap; c->stats.trial_cyc_fallback += r.cyc_fallback;
  c->stats.trial_symbols += r.symbols;
  uint64_t* gk = c->kind[k][t.clevel];
  gk[0]++; gk[1] += r.cyc_total; gk[2] += r.cyc_tree; gk[3] += r.cyc_emit; gk[4] += r.cyc_heap;
  gk[5] += r.cyc_fallback; gk[6] += r.parsed; gk[7] += r.symbols; gk[8] += r.cyc_scan; gk[9] += r.cyc_send;
  for (int i = 0; i < 4; i++) gk[10 + i] += r.cyc_sec[i];
  // trial input read + compare read (bytes emitted and compared against the original)
  if (!(t.host & TH_DUP))   // duplicates are not launched; a trial never rerun stopped at its prefix
    c->stats.k_trial_alg_bytes += r.state == TR_NEED_R || r.state == TR_SKIPPED ? r.parsed
                                  : x->recs[t.stream].infl_len + (r.out_len < C ? r.out_len : C);
  if (timing_level() >= 3 && !(t.host & TH_DUP)) {
    c->diag_rt.push_back({r.rt0, r.rt1});
    if (c->diag_path.size() <= t.stream) { c->diag_path.resize(x->recs.size(), 0); c->diag_ntr.resize(x->recs.size(), 0); }
    c->diag_path[t.stream] += (uint32_t)(r.rt1 - r.rt0);
    c->diag_ntr[t.stream]++;
  }
}
// A batch outside the sweep's rounds (strategy_pass, deflate_dev) gets bucket tables of its own: every
// earlier table is dropped (the last batch's kernels are done: run_trials synchronised) and those of
// `need` are built on pipe p, complete on return.
static int private_chains(atz_ctx* c, Pipe* p, const std::vector<std::pair<uint32_t, int>>& need) {
  for (auto& a : c->chain_off) a.fill(~0ull);
  c->chain_arena.reset(cap_bytes(CHAIN_CACHE_CAP));
  p->tmp_chains.clear();
  p->chains_next = 0;
  if (int r = ensure_chains(c, p, need)) return r;
  HIPCHK(hipStreamSynchronize(p->st));
  return 0;
}

// The reference's rule for one trial result of a stream of C compressed bytes (testDeflateParams and its
// callers, main.cpp:685-700): `best`, the stream's best ident so far, rises on an improvement; the stream
// stops on a full match or one within mismatch_tol; an improvement within recomp_tresh wants its
// mismatch list (C - ident entries; diffs are only ever written for recompressible streams).
struct RuleTally { uint64_t ntr = 0, nsc = 0, nhz = 0; };   // trials, shortcut exits, overlay hazards
struct RuleStep { bool improved = false, stop = false, diff = false; };
static int rule_step(const atz_opts_t& o, uint64_t C, const TrialRes& r, uint64_t& best, RuleTally& n, RuleStep& out) {
  n.ntr++;
  if (r.state == TR_SHORTCUT) n.nsc++;
  if (r.flags & 1) n.nhz++;
  if (r.state == TR_OVERFLOW) return ATZ_E_REF_ABORT;   // deflate() without Z_STREAM_END, main.cpp:663-665
  out = RuleStep{};
  if (r.state == TR_FULL && r.ident > best) {
    best = r.ident;
    out.improved = true;
    out.stop = r.ident == C || r.ident + o.mismatch_tol >= C;
    out.diff = r.ident != C && C - r.ident <= o.recomp_tresh;
  }
  return 0;
}

// Mismatch lists (main.cpp:699-714) of the jobs dj, from the trial outputs in the pipe's d_out: job q's
// positions and values into pos[q] / val[q] (dj[q].cap entries each; dst is assigned here).
static int run_diffs(Pipe* c, const uint8_t* d_file, std::vector<DiffJob>& dj, std::vector<std::vector<uint32_t>>& pos,
                     std::vector<std::vector<uint8_t>>& val) {
  pos.assign(dj.size(), {});
  val.assign(dj.size(), {});
  if (dj.empty()) return 0;
  uint64_t dpos = 0;
  for (DiffJob& d : dj) { d.dst = dpos; dpos += d.cap; }
  if (int r = upload(c, c->d_diffjobs, dj.data(), dj.size() * sizeof(DiffJob))) return r;
  if (int r = c->d_diffpos.reserve(dpos * 4 + 64)) return r;
  if (int r = c->d_diffval.reserve(dpos + 64)) return r;
  if (int r = c->d_diffcnt.reserve(dj.size() * 8 + 64)) return r;
  kbeg(c, 3);
  hipLaunchKernelGGL(k_diffs, dim3((uint32_t)dj.size()), dim3(64), 0, c->st, c->d_out.as<uint8_t>(), d_file,
                     c->d_diffjobs.as<DiffJob>(), c->d_diffpos.as<uint32_t>(), c->d_diffval.as<uint8_t>(),
                     c->d_diffcnt.as<uint64_t>(), (uint32_t)dj.size());
  kend(c);
  KCHECK("k_diffs");
  std::vector<uint32_t> hp(dpos);
  std::vector<uint8_t> hv(dpos);
  std::vector<uint64_t> cnt(dj.size());
  HIPCHK(pipe_copy(c, hp.data(), c->d_diffpos.p, dpos * 4, hipMemcpyDeviceToHost));
  HIPCHK(pipe_copy(c, hv.data(), c->d_diffval.p, dpos, hipMemcpyDeviceToHost));
  HIPCHK(pipe_copy(c, cnt.data(), c->d_diffcnt.p, dj.size() * 8, hipMemcpyDeviceToHost));
  HIPCHK(pipe_sync(c));
  kcollect(c);
  for (size_t q = 0; q < dj.size(); q++) {
    if (cnt[q] != dj[q].cap) return ATZ_E_INTERNAL;
    pos[q].assign(hp.begin() + dj[q].dst, hp.begin() + dj[q].dst + dj[q].cap);
    val[q].assign(hv.begin() + dj[q].dst, hv.begin() + dj[q].dst + dj[q].cap);
  }
  return 0;
}

// One round of pipe c over its batch `active`: the next K list entries of every stream (speculatively:
// a stream that stops at its j-th trial discards the results of the later ones), K sized so the rounds
// fill the GPU.  Results are applied per stream strictly in list order, so the outcome is the
// reference's sequential one; the speculation only changes how much work runs per launch.
struct Round : TrialBatch {
  atz_ctx* x; Pipe* c; const uint8_t* d_file; std::vector<StreamState>& ss; const SweepOpts& so;
  std::vector<uint32_t>& active;
  std::vector<uint32_t>& waiting;   // streams the round's scratch budget left out (next round, first)
  uint32_t K = 1;
  std::vector<TrialRes> trres[3];   // of TrialBatch::tr (k = 0 stored, 1 fast, 2 slow levels)
  // per stream, its trials of this round in list order: stream a's are mine[mbeg[a] .. mbeg[a + 1]),
  // each (kind, index in tr[kind])
  std::vector<std::pair<int, uint32_t>> mine;
  std::vector<uint32_t> mbeg;
  std::vector<std::pair<uint32_t, int>> need;   // (stream, memLevel) pairs whose bucket tables trials read
  std::vector<uint32_t> need_b;                 // per need entry: the trial's walk budget (budget-free test)
  std::vector<std::array<uint32_t, 4>> savers;  // (kind, index in tr[kind], rp_pool entry, level - 1)
  uint64_t r_bound = 0;             // d_R entries if every table-reading trial got a table (uint2 units)
  size_t nbuild = 0;
  // streams of the batch by index a into active: held[a] = its rule walk waits for a rerun
  std::vector<uint8_t> held;
  TrialSet SA, SB;                 // A: every trial neither a duplicate nor waiting for a saver; B: the waiting ones
  std::vector<uint32_t> ia[3], ib[3];   // their indices in tr[k]
  bool waiting_trials = false;
  struct PendDiff { bool live = false; DiffJob d{}; };
  std::vector<PendDiff> pend;      // a stream's live diff job: its latest improvement within recomp_tresh
  std::vector<uint32_t> jpos;      // where each stream's rule walk resumes
  RuleTally tally;
  uint64_t nspec = 0;

  Round(atz_ctx* x_, Pipe* c_, const uint8_t* f, std::vector<StreamState>& ss_, const SweepOpts& so_,
        std::vector<uint32_t>& a_, std::vector<uint32_t>& w_)
      : x(x_), c(c_), d_file(f), ss(ss_), so(so_), active(a_), waiting(w_) {}

  bool is_held(uint32_t s) const { return held[c->slot[s]] != 0; }

  // The trials of the next K list entries of every stream, within the round's scratch budget.
  void build_lists() {
    K = (uint32_t)std::max<size_t>(1, std::min<size_t>(32, round_target(x) / active.size()));
    c->mw_cap = mw_cap_for(std::min(x->sweep_nmax, active.size() * x->pipes_running));
    mbeg.assign(active.size() + 1, 0);
    mine.reserve(active.size() * K);
    uint64_t round_bytes = 0;
    const uint64_t round_budget = cap_bytes(ROUND_BUDGET_BYTES) / x->pipes_running;
    for (size_t a = 0; a < active.size(); a++) {
      mbeg[a] = (uint32_t)mine.size();
      const uint32_t s = active[a];
      StreamState& st = ss[s];
      // scratch of a round (match tables, outputs, symbols) is bounded: streams past the budget
      // wait for the next round, where they go first
      if (a > 0 && round_bytes > round_budget) {
        waiting.insert(waiting.begin(), active.begin() + a, active.end());
        active.resize(a);
        break;
      }
      for (uint32_t j = 0; j < K && st.idx + j < st.list->size(); j++) {
        const DeflSpec p = DeflSpec::from_word((*st.list)[st.idx + j]);
        const uint64_t len = x->recs[s].infl_len;
        const auto at = add(c, s, len, p, 0, st.ident);
        const int kind = at.first;
        Trial& t = tr[kind][at.second];
        t.spec_j = j;
        round_bytes += 8 * (len + 320) + t.out_cap + 4 * sym_words(c, kind, p, len);
        if (kind) {
          r_bound += ((len + 63) & ~63ull) + 256;
          need.push_back({s, p.memlevel});
          need_b.push_back((uint32_t)(c_cfg_host((uint32_t)p.level) >> (kind == 1 ? 0 : 2)));
        }
        mine.push_back(at);
      }
    }
    mbeg.resize(active.size() + 1);
    mbeg[active.size()] = (uint32_t)mine.size();
    held.assign(active.size(), 0);
    if (c->slot.size() < x->recs.size()) c->slot.resize(x->recs.size());
    for (size_t a = 0; a < active.size(); a++) c->slot[active[a]] = (uint32_t)a;
    pend.assign(active.size(), PendDiff{});
    jpos.assign(mbeg.begin(), mbeg.end() - 1);
  }

  // Replays first (they need the pairs' bucket depths only), duplicates, the eligibility floor, then the
  // bucket tables the other trials read (stream-ordered before the match walks: no sync).
  int plan() {
    c->r_next = 0;   // the round's match tables (early ones below, the rest in launch) never move
    if (int r = c->d_R.reserve(r_bound * sizeof(uint2) + 4096)) return r;
    c->stopj_cur = nullptr;
    if (K > 1 && stopflag_on()) {   // ~0 per stream: no stop found yet (stream-ordered before the trials)
      if (int r = c->d_stopj.reserve(x->recs.size() * sizeof(uint32_t) + 64)) return r;
      HIPCHK(hipMemsetAsync(c->d_stopj.p, 0xff, x->recs.size() * sizeof(uint32_t), c->st));
      c->stopj_cur = c->d_stopj.as<uint32_t>();
    }
    if (replay_on() && x->depth_pin.p) {
      // Replay planning reads the pairs' deepest buckets.  A trial that can only parse (its stream has no
      // saved sequence at its (level, window) to replay, nor a higher level's run to duplicate) needs its
      // table whatever the plan, and the table's build yields the depth: those pairs are built now, and
      // only the others get a depth pass first (k_bucket_depth), to spare the tables of trials that
      // will replay.  (Round 1 of a sweep has no saved sequences: no depth passes at all.)
      std::vector<std::pair<uint32_t, int>> dfirst, direct;
      std::vector<uint32_t> dfirst_b;
      std::vector<std::pair<int, uint32_t>> early;   // (kind, index) of the direct pairs' trials
      for (int k = 1; k < 3; k++) {
        uint32_t cur = ~0u;
        uint16_t seen[16] = {};   // the stream's levels so far in tr[k] per window (its trials are contiguous)
        for (uint32_t q = 0; q < tr[k].size(); q++) {
          const Trial& t = tr[k][q];
          if (t.stream != cur) { cur = t.stream; std::memset(seen, 0, sizeof seen); }
          const bool again = (seen[t.window & 15] >> t.clevel) & 1u;   // may wait for a saver of this round
          seen[t.window & 15] |= (uint16_t)(1u << t.clevel);
          const StreamState& st = ss[t.stream];
          bool maybe = false;
          if (st.rp >= 0) maybe = ((st.rp_saved >> t.clevel) & 1u) && st.rp_win[t.clevel] == t.window;
          if (!maybe && k == 2 && t.clevel >= 7)
            for (const auto& r : st.xl) maybe |= r[0] == t.window && r[1] == t.memlevel && r[2] > t.clevel;
          static const bool all_first = [] { const char* e = std::getenv("ATZ_DFIRST"); return e && std::atoi(e) == 0; }();
          if (maybe || all_first) {
            dfirst.push_back({t.stream, (int)t.memlevel});
            dfirst_b.push_back((uint32_t)(c_cfg_host(t.clevel) >> (k == 1 ? 0 : 2)));
          } else {
            direct.push_back({t.stream, (int)t.memlevel});
            if (!again) early.push_back({k, q});
          }
        }
      }
      for (auto& q : direct) nbuild += x->chain_off[q.first][q.second] == ~0ull;
      if (int r = ensure_depths(x, c, dfirst, dfirst_b, c->d_djobs)) return r;
      if (int r = ensure_chains(x, c, direct)) return r;
      c->lap(1);
      if (early_match_on() && !early.empty()) {
        // A direct pair's trials can become neither replays nor duplicates (no saved sequence at their
        // level and window, no higher level's twin) unless an earlier trial of their stream in this
        // round may save one (speculative rounds), so the others' first-pass tables need no plan: they
        // run while the host plans the rest, once the depths (the builds) are in.
        if (!c->ev_built) HIPCHK(hipEventCreateWithFlags(&c->ev_built, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->ev_built, c->st));
        std::vector<MatchJob> mj;
        mj.reserve(early.size());
        for (const auto& e : early) {
          Trial& t = tr[e.first][e.second];
          t.chain_off = x->chain_off[t.stream][t.memlevel];
          if (MatchJob m = first_match_job(x, c, e.first, t); m.p1 > m.p0) mj.push_back(m);
        }
        if (int r = launch_match(x, c, mj)) return r;
        c->lap(6);
        const auto t_ev = std::chrono::steady_clock::now();
        HIPCHK(hipEventSynchronize(c->ev_built));
        c->t_sync += ms_since(t_ev);
        c->n_sync++;
      } else {
        HIPCHK(pipe_sync(c));
      }
      c->lap(2);
      if (dedup_on()) level_dups(x, ss, tr[2]);
      for (int k = 1; k < 3; k++) plan_replay(x, c, ss, k, tr[k], savers);
      c->lap(3);
      need.clear();
      for (int k = 1; k < 3; k++)
        for (const Trial& t : tr[k])
          if (!tm_unchecked_replay(t.mode) && !(t.host & TH_DUP)) need.push_back({t.stream, (int)t.memlevel});
    }
    for (int k = 0; k < 3; k++)
      for (Trial& t : tr[k])
        if (!(t.mode & TM_SAVE)) t.best_ident = std::max(t.best_ident, elig_floor(x, x->recs[t.stream].comp_len));
    for (auto& q : need) nbuild += x->chain_off[q.first][q.second] == ~0ull;
    if (int r = ensure_chains(x, c, need)) return r;   // (stream-ordered before the match walks: no sync)
    for (int k = 1; k < 3; k++)
      for (Trial& t : tr[k]) {
        const uint64_t off = x->chain_off[t.stream][t.memlevel];
        t.chain_off = off == ~0ull ? 0 : off;   // unchecked replays read no table
      }
    for (int k = 1; k < 3; k++)
      for (const Trial& t : tr[k])   // saved sequences stay inside the arena (a bad slot would fault the GPU)
        if ((t.mode & TM_RP_SYMS) && !replay_slot_ok(t)) return ATZ_E_INTERNAL;
    if (int r = reserve(c)) return r;
    c->lap(4);
    return 0;
  }
  bool replay_slot_ok(const Trial& t) const {
    const uint64_t n = x->recs[t.stream].infl_len;
    const bool syms_ok = !(t.mode & TM_RP_SYMS) || x->rp_arena.holds(t.rp_syms, 4 * (n + 64));
    const bool tab_ok = !(t.mode & TM_RP_TAB) || x->rp_arena.holds(t.rp_tab, 8 * n);
    if (syms_ok && tab_ok && !((t.mode & TM_REPLAY) && t.rp_nsym > n)) return true;
    std::fprintf(stderr, "atz: symbol replay slot out of its arena (stream %u)\n", t.stream);
    return false;
  }

  // A complete saved sequence serves the stream's later trials at that level (held streams' savers wait
  // for their reruns: a saver stopped by TR_NEED_R runs again).
  void finish_savers(bool held_ones) {
    for (const auto& sv : savers) {
      if (is_held(tr[sv[0]][sv[1]].stream) != held_ones) continue;
      const TrialRes& r = trres[sv[0]][sv[1]];
      RpEntry& e = x->rp_pool[sv[2]][sv[3]];
      StreamState& st = ss[tr[sv[0]][sv[1]].stream];
      const uint16_t bit = (uint16_t)(1u << (sv[3] + 1));
      st.rp_busy &= (uint16_t)~bit;
      // a skipped trial never reached its stream's walk: its sequence is not relied on even if complete
      if (r.state != TR_NEED_R && r.state != TR_SKIPPED && (r.saved_flags & 1u)) {
        e.state = 2; e.nsym = r.saved_syms; e.flags = r.saved_flags; e.reads_max = r.reads_max;
        st.rp_saved |= bit;
      } else {
        e.state = 0;   // the slot stays for the next saving trial
      }
    }
  }
  void collect(const TrialSet& S, const std::vector<uint32_t>* idx) {
    std::vector<TrialRes> rr[3];
    trials_results(S, rr);
    for (int k = 0; k < 3; k++)
      for (size_t j = 0; j < idx[k].size(); j++) trres[k][idx[k][j]] = rr[k][j];
  }

  // First passes.  Duplicates are not launched; trials waiting for a saver of this round go in a second
  // launch set (speculative rounds, K > 1: small files, the sweep's tail) once the saver's sequence is in.
  int launch() {
    TrialRes dup{};
    dup.state = TR_CANT_BEAT;
    for (int k = 1; k < 3; k++)
      for (const Trial& t : tr[k]) waiting_trials |= (t.host & TH_WAITS) != 0;
    {
      std::vector<Trial> ta[3];
      for (int k = 0; k < 3; k++) {
        trres[k].assign(tr[k].size(), dup);
        for (uint32_t q = 0; q < tr[k].size(); q++) {
          if (tr[k][q].host & (TH_WAITS | TH_DUP)) continue;
          ta[k].push_back(tr[k][q]);
          ia[k].push_back(q);
        }
      }
      trials_order(x, c, ta, SA);
    }
    c->lap(5);
    {
      size_t bases[3];
      if (int r = trials_first_launch(x, c, d_file, SA, so, bases)) return r;
      if (int r = trials_first_finish(c, SA, bases)) return r;
    }
    if (!waiting_trials) {
      collect(SA, ia);
      return 0;
    }
    // the savers complete (reruns included) before the trials that wait for them
    if (int r = trials_rerun(x, c, d_file, SA, so, nullptr)) return r;
    collect(SA, ia);
    finish_savers(false);
    std::vector<Trial> t3[3];
    for (int k = 1; k < 3; k++)
      for (uint32_t q = 0; q < tr[k].size(); q++) {
        Trial& t = tr[k][q];
        if (!(t.host & TH_WAITS)) continue;
        t.host &= ~TH_WAITS;
        const RpEntry& e = x->rp_pool[ss[t.stream].rp][t.clevel - 1];
        if (e.state == 2 && e.window == t.window) replay_from(t, e, replay_free(x, k, t));
        if (t.host & TH_DUP) continue;
        if ((t.mode & TM_REPLAY) && !replay_slot_ok(t)) return ATZ_E_INTERNAL;
        t3[k].push_back(t);
        ib[k].push_back(q);
      }
    trials_order(x, c, t3, SB);
    if (int r = trials_first(x, c, d_file, SB, so)) return r;
    collect(SB, ib);
    return 0;
  }

  // The reference's sequential rule for stream a, in list order (main.cpp:685-700), walked up to the
  // stream's stop; with defer, a walk that reaches a trial still to be rerun (TR_NEED_R) waits there
  // (held) and resumes after the reruns.
  int walk(size_t a, bool defer) {
    const uint32_t s = active[a];
    StreamState& st = ss[s];
    const uint64_t C = x->recs[s].comp_len;
    const uint32_t phase0 = st.phase;
    held[a] = 0;
    for (uint32_t j = jpos[a]; j < mbeg[a + 1]; j++) {
      if (st.phase != phase0) { nspec += mbeg[a + 1] - j; break; }   // stopped earlier this round
      const Trial& t = tr[mine[j].first][mine[j].second];
      const TrialRes& r = trres[mine[j].first][mine[j].second];
      if (r.state == TR_NEED_R) {
        if (!defer) return ATZ_E_INTERNAL;   // every rerun a walk waits for has run
        jpos[a] = j;
        held[a] = 1;
        return 0;
      }
      if (r.state == TR_SKIPPED) return ATZ_E_INTERNAL;   // only trials past the stream's stop end so
      st.trials++;
      RuleStep step;
      if (int e = rule_step(x->o, C, r, st.ident, tally, step)) return e;
      if (step.improved) {
        st.c = t.clevel; st.w = t.window; st.m = t.memlevel;
        st.first_diff = -1;
        st.rawdiff.clear(); st.diffval.clear();
        pend[a].live = step.diff;   // an earlier improvement's diffs are superseded
        if (step.diff) pend[a].d = DiffJob{t.out_off, r.out_len, rec_src(x, x->recs[s], d_file), C, 0, C - r.ident};
      }
      st.idx++;
      if (step.stop) st.idx = (uint32_t)st.list->size();   // testParamRange/tryParams return
      if (st.idx >= st.list->size()) {
        if (st.phase == 0 && (C - st.ident) >= x->o.mismatch_tol && x->o.brute_window) {
          st.list = &trial_list(x->recs[s].type, true);
          st.idx = 0;
          st.phase = 1;
        } else {
          st.phase = 2;
        }
      }
    }
    jpos[a] = mbeg[a + 1];
    return 0;
  }

  // The bookkeeping that reads or writes a stream's state, for streams that are done with this round.
  void settle(bool held_ones) {
    finish_savers(held_ones);
    if (dedup_on() && x->depth_pin.p)
      level_record(x, ss, tr[2], trres[2], [&](uint32_t s) { return is_held(s) == held_ones; });
  }

  // Every stream's walk; the reruns of the held streams (every TR_NEED_R trial of theirs: which ones the
  // walk needs depends on the trials before), then their walks' rest.
  int apply() {
    for (size_t a = 0; a < active.size(); a++)
      if (int r = walk(a, true)) return r;
    settle(false);
    bool any_held = false;
    for (uint8_t h : held) any_held |= h != 0;
    if (!any_held) return 0;
    auto want = [&](const Trial& t) { return is_held(t.stream); };
    if (int r = trials_rerun(x, c, d_file, SA, so, want)) return r;
    collect(SA, ia);
    if (waiting_trials) {
      if (int r = trials_rerun(x, c, d_file, SB, so, want)) return r;
      collect(SB, ib);
    }
    for (size_t a = 0; a < active.size(); a++)
      if (held[a]) {
        held[a] = 0;
        if (int r = walk(a, false)) return r;
        held[a] = 1;   // (settle's selector)
      }
    settle(true);
    return 0;
  }

  // The bucket tables of the streams this round finished go back to the cache's free lists (no kernel
  // reads them any more).
  void release_done() {
    for (uint32_t s : active) {
      if (ss[s].phase != 2) continue;
      const uint64_t bytes = 8 * ((x->recs[s].infl_len + 63) & ~63ull);
      for (int m = 1; m <= 9; m++) {
        uint64_t& off = x->chain_off[s][m];
        if (off == ~0ull) continue;
        if (x->chain_arena.holds(off << 2, bytes)) x->chain_arena.release(off << 2, bytes);
        off = ~0ull;
      }
    }
  }

  // Mismatch lists (main.cpp:699-714) of the live diff jobs, from the trials' outputs.
  int flush_diffs() {
    std::vector<DiffJob> dj;
    std::vector<size_t> dja;
    for (size_t a = 0; a < active.size(); a++) {
      if (!pend[a].live) continue;
      pend[a].live = false;
      dj.push_back(pend[a].d);
      dja.push_back(a);
    }
    std::vector<std::vector<uint32_t>> pos;
    std::vector<std::vector<uint8_t>> val;
    if (int r = run_diffs(c, d_file, dj, pos, val)) return r;
    for (size_t q = 0; q < dj.size(); q++) {
      StreamState& st = ss[active[dja[q]]];
      st.rawdiff.swap(pos[q]); st.diffval.swap(val[q]);
      st.first_diff = st.rawdiff.empty() ? -1 : (int64_t)st.rawdiff[0];
    }
    return 0;
  }

  // The pipe's counters (per-kind x level: count, cycles total/tree/emit/heap/fallback, parsed bytes,
  // symbols, scan/send cycles, parse window phases) and diagnostics.
  void account(uint64_t round) {
    for (int k = 1; k < 3; k++)
      for (size_t q = 0; q < tr[k].size(); q++) {
        c->stats.n_trials_replayed += (trres[k][q].saved_flags >> 2) & 1u;
        c->stats.n_replay_checked += (tr[k][q].mode & TM_CHECKED) != 0;
        c->stats.n_trials_duplicate += (tr[k][q].host & TH_DUP) != 0;
        if (timing_on() && !tm_unchecked_replay(tr[k][q].mode) && !(tr[k][q].host & TH_DUP)) {
          if (c->diag_need.size() <= tr[k][q].stream) c->diag_need.resize(tr[k][q].stream + 1, 0);
          c->diag_need[tr[k][q].stream] |= (uint16_t)(1u << tr[k][q].memlevel);
        }
      }
    for (int k = 0; k < 3; k++)
      for (size_t q = 0; q < tr[k].size(); q++) account_trial(x, c, k, tr[k][q], trres[k][q]);
    if (!timing_on()) return;
    if (timing_level() >= 3) {   // when the round's first-pass trials ended, from the first one's start (us)
      std::vector<uint32_t> st0, en;
      for (int k = 0; k < 3; k++)
        for (size_t q = 0; q < tr[k].size(); q++)
          if (!(tr[k][q].host & TH_DUP) && trres[k][q].rt1) { st0.push_back(trres[k][q].rt0); en.push_back(trres[k][q].rt1); }
      if (!en.empty()) {
        const uint32_t b = *std::min_element(st0.begin(), st0.end());
        std::sort(en.begin(), en.end());
        auto q = [&](double f) { return (en[std::min(en.size() - 1, (size_t)(f * (double)en.size()))] - b) / 100.0; };
        std::fprintf(stderr, "atz: pipe %d round %llu ends (us after the first start): n %zu p50 %.0f p90 %.0f p95 %.0f p98 %.0f p99 %.0f max %.0f\n",
                     c->id, (unsigned long long)round, en.size(), q(0.5), q(0.9), q(0.95), q(0.98), q(0.99), q(1.0));
      }
    }
    // slowest trials of the round (diagnostics)
    std::vector<std::pair<uint64_t, std::pair<int, size_t>>> top;
    for (int k = 0; k < 3; k++)
      for (size_t q = 0; q < tr[k].size(); q++) top.push_back({trres[k][q].cyc_total, {k, q}});
    std::sort(top.begin(), top.end(), [](auto& p1, auto& p2) { return p1.first > p2.first; });
    for (size_t i = 0; i < top.size() && i < 3; i++) {
      const Trial& t = tr[top[i].second.first][top[i].second.second];
      const TrialRes& r = trres[top[i].second.first][top[i].second.second];
      std::fprintf(stderr, "atz: round %llu slow trial: stream %u I=%llu c%u w%u m%u state %u cyc %.1fM syms %llu blocks %llu "
                   "fallbacks %llu tree %.1fM emit %.1fM (heap %.1fM scan %.1fM send %.1fM fb %.1fM)\n", (unsigned long long)round, t.stream,
                   (unsigned long long)x->recs[t.stream].infl_len, t.clevel, t.window, t.memlevel, r.state,
                   r.cyc_total / 1e6, (unsigned long long)r.symbols, (unsigned long long)r.blocks,
                   (unsigned long long)(r.fallbacks & 0xffffffffull), r.cyc_tree / 1e6, r.cyc_emit / 1e6, r.cyc_heap / 1e6,
                   r.cyc_scan / 1e6, r.cyc_send / 1e6, r.cyc_fallback / 1e6);
    }
  }
};

// The sweep work of pipe c: rounds on the batches sched_take hands it.
static int sweep_pipe(atz_ctx* x, Pipe* c, const uint8_t* d_file, std::vector<StreamState>& ss) {
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint32_t> active;
  const SweepOpts so{x->o.recomp_tresh, x->o.sizediff_tresh, x->o.shortcut_len, x->o.mismatch_tol};
  uint64_t rounds = 0;
  while (sched_take(x, c->id, active)) {
    rounds++;
    std::vector<uint32_t> waiting;
    struct Give {   // the batch goes back on every exit from the round (an error aborts the sweep anyway)
      atz_ctx* x; Pipe* c; const std::vector<StreamState>& ss; const std::vector<uint32_t>& a, &w;
      ~Give() {
        c->stopj_cur = nullptr;
        forget_tmp_chains(x, c);
        sched_give(x, c->id, ss, a, w);
      }
    } give{x, c, ss, active, waiting};
    Round R(x, c, d_file, ss, so, active, waiting);
    const auto tl0 = std::chrono::steady_clock::now();
    c->lap_start();
    R.build_lists();
    c->lap(0);
    const auto ta = std::chrono::steady_clock::now();
    if (int r = R.plan()) return r;
    const auto tb = std::chrono::steady_clock::now();
    if (int r = R.launch()) return r;
    const auto tc = std::chrono::steady_clock::now();
    if (int r = R.apply()) return r;
    c->lap(10);
    if (int r = R.flush_diffs()) return r;
    R.release_done();
    c->lap(11);
    const auto td = std::chrono::steady_clock::now();
    c->t_chains += std::chrono::duration<double, std::milli>(tb - ta).count();
    c->t_trials += std::chrono::duration<double, std::milli>(tc - tb).count();
    if (timing_level() >= 2)
      std::fprintf(stderr, "atz: pipe %d round %llu at %.1f ms: active %zu K %u trials %zu/%zu/%zu list %.1f chains %.1f (%zu builds) trials %.1f ms, reruns+apply %.1f ms\n",
                   c->id, (unsigned long long)rounds, std::chrono::duration<double, std::milli>(ta - t0).count(), active.size(), R.K,
                   R.tr[0].size(), R.tr[1].size(), R.tr[2].size(), std::chrono::duration<double, std::milli>(ta - tl0).count(),
                   std::chrono::duration<double, std::milli>(tb - ta).count(), R.nbuild,
                   std::chrono::duration<double, std::milli>(tc - tb).count(),
                   std::chrono::duration<double, std::milli>(td - tc).count());
    R.account(rounds);
    c->lap(12);
    c->t_apply += ms_since(tc);
    c->stats.n_trials += R.tally.ntr; c->stats.n_trials_shortcut += R.tally.nsc; c->stats.n_hazard += R.tally.nhz;
    c->stats.n_trials_speculative += R.nspec;
  }
  c->stats.n_rounds = rounds;
  c->stats.sweep_ms = ms_since(t0);
  return 0;
}

// Phase 3 driver: streams partitioned over the context's pipes (interleaved, so every pipe gets
// the same mix of header classes and sizes), one host thread per pipe.
static int ensure_pipes(atz_ctx* c, size_t np) {
  while (c->pipes.size() < np) {
    std::unique_ptr<Pipe> p(new Pipe());
    p->id = (int)c->pipes.size();
    if (hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking) != hipSuccess) return ATZ_E_HIP;
    // the idle second stream (see Pipe::pst): with it two pipes share a hardware queue and their
    // kernels run back to back, so fewer LDS-heavy kernels co-run (measured faster)
    if (hipStreamCreateWithFlags(&p->pst, hipStreamNonBlocking) != hipSuccess) return ATZ_E_HIP;
    c->pipes.push_back(std::move(p));
  }
  return 0;
}
// ATZ_PIPES=k (1..8), default 3.  C4 A/B after the 1024-thread match blocks (interleaved, 4 runs each):
// 2 pipes ~988, 3 ~1022, 4 ~854 MB/s (earlier, with slower match walks, 2 was best)
// Pipes for a sweep of n streams (ATZ_PIPES overrides).  Three pipes, two of which share a hardware
// queue, keep the GPU full on a large file (more, or one queue each, let LDS-heavy kernels displace
// each other: DESIGN s3.6).  A small sweep -- one rank's share of a file split over many GPUs -- is
// bound by its rounds' slowest trials instead; with >= 8 hardware queues in the process
// (GPU_MAX_HW_QUEUES, read at HIP init; bench.py sets it for such runs) six pipes overlap more rounds:
// a 12 500-stream share 696-710 vs 628-655 MB/s on one MI355X (25 000: 904 vs 923, so only below 16 000).
// (Read once, thread-safely; GPU_MAX_HW_QUEUES only holds if it was set before HIP initialised.)
// Round 4 re-measured it after the round rework (12 500 streams, one box, 4 runs each, `gpurun_out/rts`):
// 3 pipes 651-675 MB/s, 6 pipes on 8 queues 714-744 (round target 4096) and 707-753 (8192).
static size_t sweep_pipes(size_t n) {
  static const std::pair<int, int> cfg = [] {
    const char* e = std::getenv("ATZ_PIPES");
    const char* q = std::getenv("GPU_MAX_HW_QUEUES");
    return std::make_pair(e ? std::max(1, std::min(8, std::atoi(e))) : -1, q ? std::atoi(q) : 4);
  }();
  if (cfg.first > 0) return (size_t)cfg.first;
  return n <= 16000 && cfg.second >= 8 ? 6 : 3;
}
// Trials per round and pipe (K = target / the pipe's active streams, 1..32).  ATZ_TARGET overrides.
// A sweep of few streams -- one rank's share of a file split over 4 or 8 GPUs -- runs the same ~16 rounds
// as the whole file with a fraction of the trials each, so its rounds are latency-bound and a deeper
// round pays on three pipes (same box, 2 runs each: 12 500 streams 677-690 -> 713-763 MB/s, 25 000
// 928-938 -> 981-994, on another box 926-934 -> 940-965; the whole C4 file: no difference, 1439-1501 vs
// 1466-1539), and is neutral on six (707-753 vs 714-744).
static size_t round_target(const atz_ctx* x) {
  static const int env = [] { const char* e = std::getenv("ATZ_TARGET"); return e ? std::max(256, std::atoi(e)) : 0; }();
  if (env) return (size_t)env;
  return x->sched.published.load() <= 32000 ? 8192 : 4096;
}
// The sweep runs while the scan is still producing records: sweep_begin starts one host thread
// per pipe, sweep_publish hands a range of ready records (inflated, Adler-32 known) to the pipes,
// sweep_finish closes the inboxes, joins the threads and folds their counters.  Host tables are
// sized for the scan's upper bound on records up front, so nothing the pipes read reallocates.
struct SweepRun {
  const uint8_t* d_file = nullptr;
  std::vector<StreamState>* ss = nullptr;
  size_t np = 0, published = 0;
  std::vector<StreamDev> sd;      // host staging of the device stream table
  std::vector<std::thread> th;
  std::vector<int> rc;
  std::chrono::steady_clock::time_point t0;
  bool running = false;
};

// abort: the pipes stop at their next round (an error, or a withdrawn speculative scan); else they
// finish the published streams
static void sweep_close(atz_ctx* c, SweepRun& R, bool abort = false) {
  {
    std::lock_guard<std::mutex> lk(c->sched.mu);
    c->sched.closed = true;
    if (abort) c->sched.abort = true;
    c->sched.cv.notify_all();
  }
  for (auto& t : R.th) t.join();
  R.th.clear();
  R.running = false;
}

static int sweep_begin(atz_ctx* c, const uint8_t* d_file, std::vector<StreamState>& ss, size_t n_max, SweepRun& R) {
  R.t0 = std::chrono::steady_clock::now();
  R.d_file = d_file;
  R.ss = &ss;
  R.published = 0;
  ss.assign(n_max, StreamState());
  c->chain_off.assign(n_max, {});
  for (auto& a : c->chain_off) a.fill(~0ull);
  c->chain_arena.reset(cap_bytes(CHAIN_CACHE_CAP));
  c->rp_arena.reset(cap_bytes(RP_ARENA_CAP));
  c->rp_pool.clear();
  c->rp_pool.reserve(n_max);
  if (int r = c->depth_pin.reserve(n_max * 40 + 64)) return r;
  std::memset(c->depth_pin.p, 0xff, n_max * 40);
  if (c->infl_off.size() < n_max) c->infl_off.resize(n_max);
  if (c->adler.size() < n_max) c->adler.resize(n_max);
  R.sd.assign(n_max, StreamDev{});
  if (int r = c->d_adler.reserve(n_max * 4 + 4096)) return r;
  if (int r = c->d_streams.reserve(n_max * sizeof(StreamDev) + 4096)) return r;
  R.np = std::max<size_t>(1, std::min(sweep_pipes(n_max), (n_max + 255) / 256));
  c->pipes_running = R.np;
  c->sweep_nmax = n_max;
  if (int r = ensure_pipes(c, R.np)) return r;
  {
    auto& Q = c->sched;
    std::lock_guard<std::mutex> lk(Q.mu);
    Q.q.assign(R.np, std::deque<uint32_t>());
    Q.unfinished.assign(R.np, 0);
    Q.closed = false;
    Q.abort = false;
    Q.published = 0;
  }
  for (size_t g = 0; g < R.np; g++) {
    Pipe* p = c->pipes[g].get();
    p->tmp_chains.clear();
    p->stats = atz_stats_t{};
    p->t_list = p->t_chains = p->t_trials = p->t_apply = p->t_copy = p->t_sync = 0;
    p->n_copy = p->n_sync = 0;
    std::memset(p->ph, 0, sizeof(p->ph));
    std::memset(p->ph_wait, 0, sizeof(p->ph_wait));
    std::memset(p->kind, 0, sizeof(p->kind));
  }
  R.rc.assign(R.np, 0);
  R.running = true;
  for (size_t g = 0; g < R.np; g++)
    R.th.emplace_back([c, &R, &ss, g]() {
      if (hipSetDevice(c->dev) != hipSuccess) { R.rc[g] = ATZ_E_HIP; sched_abort(c); return; }
      HostProf::Enroll prof_enroll;
      try {   // no exception may leave a thread (guarded() covers the calling one)
        R.rc[g] = sweep_pipe(c, c->pipes[g].get(), R.d_file, ss);
      } catch (const std::bad_alloc&) {
        R.rc[g] = ATZ_E_NOMEM;
      } catch (...) {
        R.rc[g] = ATZ_E_INTERNAL;
      }
      if (R.rc[g]) sched_abort(c);   // the other pipes stop too (streams this one held never come back)
    });
  return 0;
}

// records [r0, r1) are inflated (infl_off, adler set): device table entries, then the queues
static int sweep_publish(atz_ctx* c, SweepRun& R, size_t r0, size_t r1) {
  if (r1 <= r0) return 0;
  if (r1 > R.sd.size()) return ATZ_E_INTERNAL;
  for (size_t s = r0; s < r1; s++) {
    StreamDev& d = R.sd[s];
    d.orig_off = rec_src(c, c->recs[s], R.d_file); d.infl_off = c->infl_off[s];
    d.comp_len = c->recs[s].comp_len; d.infl_len = c->recs[s].infl_len;
    (*R.ss)[s].list = &trial_list(c->recs[s].type, false);
  }
  HIPCHK(hipMemcpyAsync(c->d_adler.as<uint32_t>() + r0, c->adler.data() + r0, (r1 - r0) * 4, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipMemcpyAsync(c->d_streams.as<StreamDev>() + r0, R.sd.data() + r0, (r1 - r0) * sizeof(StreamDev),
                        hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));   // the pipes' streams read these tables
  {
    auto& Q = c->sched;
    std::lock_guard<std::mutex> lk(Q.mu);
    // interleaved over the pipes by global index: every pipe gets the same mix of classes and sizes
    // (a raw record has no reference walk: done at once; raw_pass walks it after the sweep)
    for (size_t s = r0; s < r1; s++) {
      if (c->recs[s].type >= 24) { (*R.ss)[s].phase = 2; continue; }
      Q.q[s % R.np].push_back((uint32_t)s); Q.unfinished[s % R.np]++;
    }
    Q.published = r1;
    Q.cv.notify_all();
  }
  R.published = r1;
  return 0;
}

static int sweep_finish(atz_ctx* c, SweepRun& R) {
  sweep_close(c, R);
  const size_t np = R.np, n = R.published;
  std::vector<StreamState>& ss = *R.ss;
  for (size_t g = 0; g < np; g++) if (R.rc[g]) return R.rc[g];
  ss.resize(n);
  // fold the pipes' counters into the context's
  uint64_t kind[3][10][14] = {};
  double tch = 0, ttr = 0, tap = 0;
  for (size_t g = 0; g < np; g++) {
    const Pipe* p = c->pipes[g].get();
    const atz_stats_t& q = p->stats;
    atz_stats_t& t = c->stats;
    t.n_trials += q.n_trials; t.n_trials_shortcut += q.n_trials_shortcut; t.n_hazard += q.n_hazard;
    t.n_rounds = std::max(t.n_rounds, q.n_rounds); t.n_trials_speculative += q.n_trials_speculative;
    t.k_trial_ms += q.k_trial_ms; t.k_chains_ms += q.k_chains_ms; t.k_other_ms += q.k_other_ms; t.k_match_ms += q.k_match_ms;
    t.k_trial_launches += q.k_trial_launches; t.k_chains_launches += q.k_chains_launches;
    t.k_match_launches += q.k_match_launches;
    t.k_trial_alg_bytes += q.k_trial_alg_bytes; t.k_chains_alg_bytes += q.k_chains_alg_bytes;
    t.trial_parsed_bytes += q.trial_parsed_bytes; t.k_match_positions += q.k_match_positions;
    t.n_trials_rerun += q.n_trials_rerun; t.n_fast_fallbacks += q.n_fast_fallbacks; t.n_fast_restarts += q.n_fast_restarts;
    t.trial_cyc_total += q.trial_cyc_total; t.trial_cyc_tree += q.trial_cyc_tree; t.trial_cyc_emit += q.trial_cyc_emit;
    t.trial_blocks += q.trial_blocks; t.trial_cyc_heap += q.trial_cyc_heap; t.trial_cyc_fallback += q.trial_cyc_fallback;
    t.trial_symbols += q.trial_symbols; t.n_trials_replayed += q.n_trials_replayed; t.n_replay_checked += q.n_replay_checked;
    t.n_trials_duplicate += q.n_trials_duplicate; t.n_trials_skipped += q.n_trials_skipped;
    tch = std::max(tch, p->t_chains); ttr = std::max(ttr, p->t_trials); tap = std::max(tap, p->t_apply);
    for (int k = 0; k < 3; k++) for (int l = 0; l < 10; l++) for (int i = 0; i < 14; i++) kind[k][l][i] += p->kind[k][l][i];
  }
  if (timing_on()) {
    std::fprintf(stderr, "atz: sweep host: chains %.1f ms (incl. kernels), trials %.1f ms (incl. kernels), apply %.1f ms, total %.1f ms\n",
                 tch, ttr, tap, ms_since(R.t0));
    std::fprintf(stderr, "atz: device/pinned allocations so far: %llu allocs, %llu frees, %.1f ms in them\n",
                 (unsigned long long)g_dev.n_alloc.load(), (unsigned long long)g_dev.n_free.load(), g_dev.alloc_us.load() / 1e3);
    for (size_t g = 0; g < np; g++) {
      Pipe* p = c->pipes[g].get();
      std::fprintf(stderr, "atz: pipe %zu: %llu copy calls %.1f ms, %llu syncs %.1f ms\n", g, (unsigned long long)p->n_copy,
                   p->t_copy, (unsigned long long)p->n_sync, p->t_sync);
      static const char* phn[Pipe::NPH] = {"list", "tables-enq", "tables-sync", "replay-plan", "plan-rest", "order",
                                           "match-jobs", "match-launch", "trial-launch", "results", "apply", "diffs", "account"};
      std::string line;
      char b[96];
      for (int i = 0; i < Pipe::NPH; i++) {
        std::snprintf(b, sizeof b, " %s %.1f(%.1f)", phn[i], p->ph[i], p->ph_wait[i]);
        line += b;
      }
      std::fprintf(stderr, "atz: pipe %zu host phases ms (waiting):%s\n", g, line.c_str());
    }
    uint64_t nb = 0, nn = 0;
    for (size_t g = 0; g < np; g++) {
      Pipe* p = c->pipes[g].get();
      nb += p->diag_builds;
      for (uint16_t v : p->diag_need) nn += (uint64_t)__builtin_popcount(v);
      p->diag_builds = 0;
      p->diag_need.clear();
    }
    std::fprintf(stderr, "atz: bucket builds %llu, (stream, memLevel) pairs a table-reading trial used %llu; bucket cache "
                 "%.2f GB allocated, %.2f GB served from released tables; saved sequences %.2f GB; device peak %.2f GB\n",
                 (unsigned long long)nb, (unsigned long long)nn, c->chain_arena.total / 1e9, c->chain_arena.reused / 1e9,
                 c->rp_arena.total / 1e9, g_dev.peak.load() / 1e9);
  }
  if (timing_level() >= 3) {   // per-stream critical path: each stream's trials run one after another
    std::vector<uint64_t> path(n, 0), ntr(n, 0);
    for (size_t g = 0; g < np; g++) {
      Pipe* p = c->pipes[g].get();
      for (size_t s2 = 0; s2 < p->diag_path.size() && s2 < n; s2++) { path[s2] += p->diag_path[s2]; ntr[s2] += p->diag_ntr[s2]; }
      p->diag_path.clear();
      p->diag_ntr.clear();
    }
    std::vector<uint32_t> ord(n);
    for (size_t s2 = 0; s2 < n; s2++) ord[s2] = (uint32_t)s2;
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return path[a] > path[b]; });
    if (n) {
      auto q = [&](double f) { return path[ord[std::min(n - 1, (size_t)(f * (double)n))]] / 1e5; };
      std::fprintf(stderr, "atz: per-stream trial time (ms, summed over its trials): max %.2f p1 %.2f p5 %.2f p10 %.2f p50 %.2f\n",
                   q(0.0), q(0.01), q(0.05), q(0.10), q(0.5));
      for (size_t i = 0; i < n && i < 8; i++)
        std::fprintf(stderr, "atz:   stream %u: %.2f ms over %llu trials, I=%llu C=%llu ident %llu type %d phase %u\n", ord[i],
                     path[ord[i]] / 1e5, (unsigned long long)ntr[ord[i]], (unsigned long long)c->recs[ord[i]].infl_len,
                     (unsigned long long)c->recs[ord[i]].comp_len, (unsigned long long)ss[ord[i]].ident, c->recs[ord[i]].type,
                     ss[ord[i]].phase);
    }
  }
  if (timing_level() >= 3) {   // trials running at once over the sweep (first passes only: reruns overwrite)
    std::vector<std::pair<uint32_t, int>> ev;
    for (size_t g = 0; g < np; g++) {
      Pipe* p = c->pipes[g].get();
      for (auto& e : p->diag_rt) { ev.push_back({e.first, 1}); ev.push_back({e.second, -1}); }
      p->diag_rt.clear();
    }
    if (!ev.empty()) {
      std::sort(ev.begin(), ev.end());
      const uint32_t t0 = ev.front().first, t1 = ev.back().first;
      double area = 0;
      int cur = 0, peak = 0;
      uint32_t last = t0;
      std::vector<double> bin((size_t)((t1 - t0) / 500000u) + 1, 0.0);   // 5 ms bins (100 MHz clock)
      for (auto& e : ev) {
        // bins relative to t0, in 64 bits (the next 5 ms boundary of an absolute time near 2^32 would wrap)
        for (uint64_t a = last - t0; a < (uint64_t)(e.first - t0);) {
          const uint64_t b = std::min<uint64_t>(e.first - t0, (a / 500000u + 1u) * 500000u);
          bin[(size_t)(a / 500000u)] += (double)cur * (double)(b - a);
          a = b;
        }
        area += (double)cur * (e.first - last);
        cur += e.second;
        peak = std::max(peak, cur);
        last = e.first;
      }
      std::fprintf(stderr, "atz: trials in flight: mean %.0f over %.1f ms, peak %d; per 5 ms:", area / std::max<uint32_t>(1, t1 - t0),
                   (t1 - t0) / 1e5, peak);
      for (double v : bin) std::fprintf(stderr, " %.0f", v / 500000.0);
      std::fprintf(stderr, "\n");
    }
  }
  if (timing_on())
    for (int k = 0; k < 3; k++)
      for (int l = 0; l < 10; l++) {
        const uint64_t* gk = kind[k][l];
        if (!gk[0]) continue;
        std::fprintf(stderr, "atz: kind %d level %d: trials %llu cyc %.3fT (tree %.3fT [heap %.3fT scan %.3fT] emit %.3fT [send %.3fT] fb %.3fT) "
                     "parsed %.1f MB syms %.1f M cyc/byte %.0f\n", k, l, (unsigned long long)gk[0], gk[1] / 1e12,
                     gk[2] / 1e12, gk[4] / 1e12, gk[8] / 1e12, gk[3] / 1e12, gk[9] / 1e12, gk[5] / 1e12, gk[6] / 1e6, gk[7] / 1e6,
                     gk[6] ? (double)gk[1] / gk[6] : 0.0);
        std::fprintf(stderr, "atz:     window phases: refill %.3fT steps %.3fT path %.3fT tally+flush %.3fT\n",
                     gk[10] / 1e12, gk[11] / 1e12, gk[12] / 1e12, gk[13] / 1e12);
      }
  for (size_t s = 0; s < n; s++) {
    StreamState& st = ss[s];
    const uint64_t C = c->recs[s].comp_len;
    st.recomp = (C - st.ident) <= c->o.recomp_tresh && st.ident > 0;
  }
  c->stats.sweep_ms = ms_since(R.t0);
  return 0;
}

// joins the pipe threads on every exit path of a caller that started them
struct SweepGuard {
  atz_ctx* c;
  SweepRun& R;
  ~SweepGuard() { if (R.running) sweep_close(c, R, true); }
};

// ---------------------------------------------------------------------------------------------
// Opt-in strategy trials (atz_set_strategies): strategy_list (atz_params.h) and its pass.
// One round per list position on pipe 0, the streams of a round in batches within the scratch budget (each
// batch builds the bucket tables its filtered trials read, as deflate_dev does).  A stream the pass
// records gets clevel = strategy << 4 | level; the others keep what the reference walk left.
// raw: the same pass over the container extension's records (raw_list; TM_RAW trials), see raw_pass.
static int ext_pass(atz_ctx* c, const uint8_t* d_file, std::vector<StreamState>& ss, bool raw) {
  const auto t0 = std::chrono::steady_clock::now();
  const size_t n = ss.size();
  struct Ext {
    std::vector<uint32_t> list;
    uint32_t best = 0;
    uint64_t ident = 0;
    bool done = false;
    std::vector<uint32_t> rawdiff;
    std::vector<uint8_t> diffval;
  };
  std::vector<Ext> ex(n);
  std::vector<uint32_t> todo;
  size_t longest = 0;
  for (size_t s = 0; s < n; s++) {
    if (ss[s].recomp || c->recs[s].infl_len >= (1ull << 31)) continue;
    if (raw) raw_list(ex[s].list, c->recs[s].type, c->defl_mask, (c->recs[s].flags & 128u) != 0);
    else strategy_list(ex[s].list, c->recs[s].type, c->strat_mask);
    if (ex[s].list.empty()) continue;
    todo.push_back((uint32_t)s);
    longest = std::max(longest, ex[s].list.size());
  }
  if (todo.empty()) return 0;
  if (int r = ensure_pipes(c, 1)) return r;
  HIPCHK(hipStreamSynchronize(c->st));
  Pipe* p = c->pipes[0].get();
  c->pipes_running = 1;
  p->mw_cap = mw_cap_for(todo.size());
  p->stopj_cur = nullptr;
  const atz_stats_t before = p->stats;
  const double gnu_before = p->kt.gnu_ms;
  const SweepOpts so{c->o.recomp_tresh, c->o.sizediff_tresh, c->o.shortcut_len, c->o.mismatch_tol};
  const uint64_t budget = cap_bytes(ROUND_BUDGET_BYTES);
  RuleTally tally;
  for (size_t j = 0; j < longest; j++) {
    std::vector<uint32_t> act;
    for (uint32_t s : todo)
      if (!ex[s].done && j < ex[s].list.size()) act.push_back(s);
    if (act.empty()) break;
    for (size_t a0 = 0; a0 < act.size();) {
      size_t a1 = a0;
      uint64_t bytes = 0;
      while (a1 < act.size() && (a1 == a0 || bytes <= budget)) {
        const uint32_t s = act[a1];
        const DeflSpec q = DeflSpec::from_word(ex[s].list[j]);
        const uint64_t len = c->recs[s].infl_len;
        bytes += 9 * len + 4 * sym_words(p, 2, q, len) + bound(len, q) + 4096;
        a1++;
      }
      std::vector<std::pair<uint32_t, int>> need;
      for (size_t a = a0; a < a1; a++) {
        const DeflSpec q = DeflSpec::from_word(ex[act[a]].list[j]);
        if (q.needs_tables()) need.push_back({act[a], q.table_memlevel()});
      }
      if (int r = private_chains(c, p, need)) return r;
      TrialBatch B;   // never saves, replays or stands for a duplicate
      B.flush_kernels = raw && c->seg_mask;
      for (size_t a = a0; a < a1; a++) {
        const uint32_t s = act[a];
        const DeflSpec q = DeflSpec::from_word(ex[s].list[j]);   // (raw_list's entries carry the raw bit themselves)
        const auto at = B.add(p, s, c->recs[s].infl_len, q, 0, std::max(ex[s].ident, elig_floor(c, c->recs[s].comp_len)));
        if (at.first) B.tr[at.first][at.second].chain_off = c->chain_off[s][q.table_memlevel()];
      }
      if (int r = B.reserve(p)) return r;
      std::vector<TrialRes> rr[3];
      if (int r = run_trials(c, p, d_file, B.tr, so, rr)) return r;
      // the rule on each stream's trial; the mismatch lists of the improvements within recomp_tresh from
      // the outputs, which the next batch overwrites
      std::vector<DiffJob> dj;
      std::vector<uint32_t> djs;
      for (int k = 0; k < 3; k++)
        for (size_t q = 0; q < B.tr[k].size(); q++) {
          const Trial& t = B.tr[k][q];
          const TrialRes& r = rr[k][q];
          const uint32_t s = t.stream;
          const uint64_t C = c->recs[s].comp_len;
          Ext& e = ex[s];
          if (r.state == TR_NEED_R || r.state == TR_SKIPPED) return ATZ_E_INTERNAL;
          ss[s].trials++;
          RuleStep step;
          if (int err = rule_step(c->o, C, r, e.ident, tally, step)) return err;
          if (!step.improved) continue;
          e.best = e.list[j];
          e.rawdiff.clear(); e.diffval.clear();
          e.done = step.stop;
          if (step.diff) {
            dj.push_back(DiffJob{t.out_off, r.out_len, rec_src(c, c->recs[s], d_file), C, 0, C - r.ident});
            djs.push_back(s);
          }
        }
      std::vector<std::vector<uint32_t>> pos;
      std::vector<std::vector<uint8_t>> val;
      if (int r = run_diffs(p, d_file, dj, pos, val)) return r;
      for (size_t q = 0; q < dj.size(); q++) { ex[djs[q]].rawdiff.swap(pos[q]); ex[djs[q]].diffval.swap(val[q]); }
      a0 = a1;
    }
  }
  forget_tmp_chains(c, p);
  for (uint32_t s : todo) {
    Ext& e = ex[s];
    const uint64_t C = c->recs[s].comp_len;
    if (!(e.ident > 0 && C - e.ident <= c->o.recomp_tresh)) continue;   // main.cpp:454
    StreamState& st = ss[s];
    const auto cwm = DeflSpec::from_word(e.best).desc();
    st.c = cwm[0]; st.w = cwm[1]; st.m = cwm[2];
    st.ident = e.ident;
    st.rawdiff.swap(e.rawdiff); st.diffval.swap(e.diffval);
    st.first_diff = st.rawdiff.empty() ? -1 : (int64_t)st.rawdiff[0];
    st.recomp = true;
  }
  atz_stats_t& t = c->stats;
  const atz_stats_t& q = p->stats;
  t.n_trials += tally.ntr; t.n_trials_shortcut += tally.nsc; t.n_hazard += tally.nhz;
  t.k_trial_ms += q.k_trial_ms - before.k_trial_ms; t.k_trial_launches += q.k_trial_launches - before.k_trial_launches;
  t.k_chains_ms += q.k_chains_ms - before.k_chains_ms; t.k_chains_launches += q.k_chains_launches - before.k_chains_launches;
  t.k_match_ms += q.k_match_ms - before.k_match_ms; t.k_match_launches += q.k_match_launches - before.k_match_launches;
  t.k_other_ms += q.k_other_ms - before.k_other_ms;
  t.sweep_ms += ms_since(t0);
  if (timing_on()) std::fprintf(stderr, "atz: %s pass: %zu streams, %llu trials  %9.2f ms\n", raw ? "raw" : "strategy",
                                todo.size(), (unsigned long long)tally.ntr, ms_since(t0));
  if (timing_on() && raw && c->defl_mask)
    std::fprintf(stderr, "atz: raw pass: k_trial_fast_gnu + k_trial_slow_gnu %9.3f ms of k_trial %9.3f ms\n",
                 p->kt.gnu_ms - gnu_before, q.k_trial_ms - before.k_trial_ms);
  return 0;
}
static int strategy_pass(atz_ctx* c, const uint8_t* d_file, std::vector<StreamState>& ss) {
  return c->strat_mask ? ext_pass(c, d_file, ss, false) : 0;
}

// The raw walk (the container extension) over raw_list's candidates (atz_params.h).
static int raw_pass(atz_ctx* c, const uint8_t* d_file, std::vector<StreamState>& ss) {
  return (c->cont_mask || c->probe_mask || c->seg_mask) ? ext_pass(c, d_file, ss, true) : 0;
}

// the sweep of every record of the context (atz_sweep)
static int sweep_impl(atz_ctx* c, const uint8_t* d_file, std::vector<StreamState>& ss) {
  const size_t n = c->recs.size();
  SweepRun R;
  SweepGuard guard{c, R};
  if (int r = sweep_begin(c, d_file, ss, n, R)) return r;
  if (int r = sweep_publish(c, R, 0, n)) return r;
  if (int r = sweep_finish(c, R)) return r;
  if (int r = strategy_pass(c, d_file, ss)) return r;
  return raw_pass(c, d_file, ss);
}

// ---------------------------------------------------------------------------------------------
// Phase 4: ATZ1 assembled in HBM
// The context's records as the writer takes them (atz_format.h); the pointers are into ss, infl_off, st_off / st_len.
static auto write_recs(const atz_ctx* c, const std::vector<StreamState>& ss) {
  return [c, &ss](size_t s) {
    const Rec& r = c->recs[s];
    const StreamState& st = ss[s];
    WriteRec x;
    x.off = r.offset; x.comp_len = r.comp_len; x.infl_len = r.infl_len;
    x.recomp = st.recomp; x.c = st.c; x.w = st.w; x.m = st.m;
    x.first_diff = st.first_diff; x.nd = st.rawdiff.size(); x.pos = st.rawdiff.data(); x.val = st.diffval.data();
    x.payload = c->infl_off[s];   // absolute address (INFL_BASE)
    if (r.stitch != ~0ull) { x.k = r.pk; x.piece_off = c->st_off.data() + r.p0; x.piece_len = c->st_len.data() + r.p0; }
    return x;
  };
}

static int write_impl(atz_ctx* c, const uint8_t* d_file, uint64_t F, const std::vector<StreamState>& ss,
                      uint64_t* atz_len) {
  auto t0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> meta;
  std::vector<Seg> segs;
  uint64_t out = 0;
  if (int r = write_file(c->recs.size(), write_recs(c, ss), F, meta, segs, out)) return r;
  if (int r = c->d_atz.reserve(out + 4096)) return r;
  if (int r = gather_segments(c, d_file, meta, segs, c->d_atz.as<uint8_t>())) return r;
  *atz_len = out;
  c->stats.write_ms = ms_since(t0);
  return 0;
}

static bool spec_cont_on() {   // ATZ_SPEC_CONT=0: the scan waits for the first continuations
  static const int v = [] { const char* e = std::getenv("ATZ_SPEC_CONT"); return (int)(e ? std::atoi(e) : 1); }();
  return v != 0;
}
static bool spec_abort_test() {   // ATZ_SPEC_ABORT_TEST=1 (read per call): withdraw the speculative sweep
  const char* e = std::getenv("ATZ_SPEC_ABORT_TEST");
  return e && *e == '1';
}

// ---------------------------------------------------------------------------------------------
// Opt-in nesting (atz_set_nesting)
static int precompress_dev(atz_ctx* c, const uint8_t* d_file, const uint8_t* h, uint64_t F, uint64_t* atz_len,
                           std::vector<StreamState>* ss_out);

// The context's child: same device and options, its own stream, buffers and records
static int nest_child(atz_ctx* c, atz_ctx** out) {
  if (!c->nest_child) {
    std::unique_ptr<atz_ctx> k(new atz_ctx());
    k->o = c->o;
    k->o.device = c->dev;
    k->dev = c->dev;
    if (hipStreamCreateWithFlags(&k->st, hipStreamNonBlocking) != hipSuccess) return ATZ_E_HIP;
    c->nest_child = k.release();
  }
  *out = c->nest_child;
  return 0;
}

static void close_ctx(atz_ctx* c) {
  if (!c) return;
  close_ctx(c->nest_child);
  c->nest_child = nullptr;
  hipStreamSynchronize(c->st);
  hipStreamDestroy(c->st);
  delete c;   // every DBuf member frees its device memory
}

// While the child runs, the parent's sweep is over: its pipes (their trial, symbol and match-table buffers and
// streams) and the chunks of its bucket-table and saved-sequence arenas serve the child, and come back with whatever
// the child added.  (A chunk list only grows at its end, so the owner's position in it stays valid.)
struct NestLend {
  atz_ctx *a, *b;
  NestLend(atz_ctx* a_, atz_ctx* b_) : a(a_), b(b_) { swap(); }
  ~NestLend() { swap(); }
  void swap() {
    std::swap(a->pipes, b->pipes);
    std::swap(a->chain_arena.chunks, b->chain_arena.chunks);
    std::swap(a->chain_arena.span, b->chain_arena.span);
    std::swap(a->rp_arena.chunks, b->rp_arena.chunks);
    std::swap(a->rp_arena.span, b->rp_arena.span);
  }
};

// Phase 4 of a context with a depth, after level 0's passes.  P is gathered from the payloads where they lie, the
// child precompresses it, and if the child recorded a stream the file is the nested one (nested = true): the
// stripped outer and the child's file behind the 20 header bytes.  Else nothing is written here and the caller
// writes the flat file.
static int nest_write(atz_ctx* c, const uint8_t* d_file, uint64_t F, const std::vector<StreamState>& ss,
                      uint64_t* atz_len, bool& nested) {
  nested = false;
  c->nest_ran = false;
  auto rec = write_recs(c, ss);
  std::vector<Seg> psegs;
  uint64_t plen = 0;
  if (!plan_payloads(c->recs.size(), rec, psegs, plen) || !plen) return 0;
  if (int r = c->d_nestp.reserve(plen + 4096)) return r;
  const std::vector<uint8_t> none(8, 0);
  if (int r = gather_segments(c, d_file, none, psegs, c->d_nestp.as<uint8_t>())) return r;
  HIPCHK(hipMemsetAsync(c->d_nestp.as<uint8_t>() + plen, 0, 4096, c->st));   // the slack a file has
  c->h_nestp.resize(plen);
  HIPCHK(hipMemcpyAsync(c->h_nestp.data(), c->d_nestp.p, plen, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  atz_ctx* k = nullptr;
  if (int r = nest_child(c, &k)) return r;
  k->o = c->o; k->o.device = c->dev;
  k->strat_mask = c->strat_mask; k->cont_mask = c->cont_mask; k->stitch_mask = c->stitch_mask;
  k->probe_mask = c->probe_mask; k->seg_mask = c->seg_mask; k->defl_mask = c->defl_mask;
  k->nest_depth = c->nest_depth - 1;
  k->nest_ran = false;
  uint64_t inner_len = 0;
  int rc;
  {
    NestLend lend(c, k);
    rc = precompress_dev(k, c->d_nestp.as<uint8_t>(), c->h_nestp.data(), plen, &inner_len, nullptr);
  }
  if (rc == ATZ_E_REF_ABORT || rc == ATZ_E_REF_UB) return 0;   // the reference itself would have died on P
  if (rc) return rc;
  c->nest_ran = true;
  if (!k->stats.n_recomp) return 0;
  auto t0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> meta;
  std::vector<Seg> segs;
  uint64_t outer_len = 0, out = 0;
  if (int r = write_file(c->recs.size(), rec, F, meta, segs, outer_len, true)) return r;
  if (int r = write_nest(meta, segs, outer_len, (uint64_t)(uintptr_t)k->d_atz.p, inner_len, out)) return r;
  if (int r = c->d_atz.reserve(out + 4096)) return r;
  if (int r = gather_segments(c, d_file, meta, segs, c->d_atz.as<uint8_t>())) return r;
  *atz_len = out;
  c->stats.write_ms = ms_since(t0);
  nested = true;
  return 0;
}

static int precompress_dev(atz_ctx* c, const uint8_t* d_file, const uint8_t* h, uint64_t F, uint64_t* atz_len,
                           std::vector<StreamState>* ss_out) {
  auto t0 = std::chrono::steady_clock::now();
  c->scan_valid = false; c->shard.stage = 0;
  c->stats = atz_stats_t{};
  c->hfile = h; c->flen = F;
  struct Drop { atz_ctx* c; ~Drop() { c->hfile = nullptr; } } drop{c};   // h is the caller's, valid for this call only
  c->stats.file_bytes = F;
  c->recs.clear();
  if (!c->scan_keep) c->scan_keep = std::make_shared<ScanState>();
  ScanState& S = *c->scan_keep;
  if (int r = scan_plan(c, h, d_file, F, S)) return r;
  ScanExt E(c);   // (the extensions' candidates, none without a mask: the sweep's tables have room for them)
  if (int r = ext_prepare(c, h, d_file, F, E)) return r;
  const size_t n_max = S.max_records() + E.extra_records();
  c->recs.reserve(n_max);
  std::vector<StreamState>& ss = c->ss_keep;
  SweepRun R;
  R.sd.swap(c->sd_keep);
  struct KeepSd { SweepRun& R; atz_ctx* c; ~KeepSd() { R.sd.swap(c->sd_keep); } } keep_sd{R, c};
  SweepGuard guard{c, R};
  const uint32_t nch = (uint32_t)S.chunks.size();
  // The scan runs as one piece: handing the sweep early records of a partial scan (several chunk
  // ranges, measured 2 pieces 840 vs 1025 MB/s) left late streams' round chains running on a half-empty
  // GPU.  The piece loop below stays for ATZ_SPEC_CONT=0 (scan, then sweep).
  const uint32_t P = 1;
  while (c->slabs.size() < P) c->slabs.emplace_back(new DBuf());
  // The sweep's host set-up (per-record tables sized for every candidate, pipe threads) runs on a
  // helper thread while the first piece's candidate inflates keep the GPU busy; with one piece
  // nothing reaches the pipes before that piece is scanned anyway.  (It touches no state of the
  // scan: c->recs, the scan buffers and the arena are the scan's; infl_off / adler are resized
  // here before inflate_records reads them.)
  int rc_begin = 0;
  std::thread t_begin([&]() {
    auto tsb = std::chrono::steady_clock::now();
    rc_begin = sweep_begin(c, d_file, ss, n_max, R);
    if (timing_on()) std::fprintf(stderr, "atz: sweep begin (%zu slots)       %9.2f ms\n", n_max, ms_since(tsb));
  });
  struct Join { std::thread& t; ~Join() { if (t.joinable()) t.join(); } } join_begin{t_begin};
  double scan_busy = ms_since(t0);
  // (with a container, stitch, probe or segment mask the added records need the reference's final ones: scan,
  // merge, then sweep)
  const bool spec = P == 1 && spec_cont_on() && !ext_on(c);
  if (spec) {
    // The first continuations of pending streams (each a decode of the stream from its header through
    // the chunk boundary) are latency-bound: one small launch, 15-30 ms.  The records do not wait for
    // it: they are replayed as if every continuation fails -- the refill repeats the chunk's last
    // byte, which almost always ends a pending stream with a data error (main.cpp:207-216) -- and
    // handed to the sweep; then the real continuations run beside the sweep's first rounds and the
    // replay is repeated with them.  Identical records confirm the speculation; otherwise the sweep
    // is withdrawn and restarted on the real records (ATZ_SPEC_ABORT_TEST=1 forces that path).
    auto tm_ = std::chrono::steady_clock::now();
    if (int r = scan_candidates(c, h, d_file, S, 0, nch)) return r;
    for (uint32_t j : scan_pending(S, 0, nch)) {
      InfRes e{};
      e.status = INF_ERROR;
      S.cont0[j] = e;
    }
    if (int r = scan_replay(c, h, S, 0, nch)) return r;
    t_begin.join();
    if (rc_begin) return rc_begin;
    const size_t r1 = c->recs.size();
    if (int r = inflate_records(c, d_file, F, 0, r1, *c->slabs[0])) return r;
    if (int r = sweep_publish(c, R, 0, r1)) return r;
    TMARK("scan: speculative records out");
    if (c->on_records) {
      // the ATZ1 size if every speculative record is recompressed with up to recomp_tresh diffs (9 bytes
      // each: delta + value), plus the whole file as residue.  Records the continuations add are not in
      // it; HostOut::take reallocates (and says so under ATZ_TIMING) if the file turns out larger.
      uint64_t est = F + 4096;
      for (size_t s = 0; s < r1; s++)
        est += c->recs[s].infl_len + 64 + 9 * std::min<uint64_t>(c->o.recomp_tresh, c->recs[s].comp_len);
      c->on_records(est);
    }
    if (int r = scan_continuations(c, h, d_file, S, 0, nch)) return r;
    S.need_more = false;
    S.pd = ScanPend{};
    std::vector<Rec>& check = S.check;
    check.clear();
    check.reserve(n_max);
    if (int r = scan_replay(c, h, S, 0, nch, &check)) return r;
    bool same = check.size() == r1;
    for (size_t i = 0; same && i < r1; i++) {
      const Rec &a = check[i], &b = c->recs[i];
      same = a.offset == b.offset && a.comp_len == b.comp_len && a.infl_len == b.infl_len && a.type == b.type &&
             a.flags == b.flags && a.arena_off == b.arena_off;
    }
    if (spec_abort_test()) same = false;
    if (!same) {
      c->sweep_abort.store(true);
      sweep_close(c, R, true);
      c->sweep_abort.store(false);
      c->recs.assign(check.begin(), check.end());   // capacity n_max: no reallocation
      if (int r = sweep_begin(c, d_file, ss, n_max, R)) return r;
      const size_t r2 = c->recs.size();
      if (int r = inflate_records(c, d_file, F, 0, r2, *c->slabs[0])) return r;
      if (int r = sweep_publish(c, R, 0, r2)) return r;
      if (timing_on()) std::fprintf(stderr, "atz: speculative scan withdrawn (%zu vs %zu records)\n", r1, r2);
    }
    TMARK("scan: continuations checked");
    scan_busy += ms_since(t0) - scan_busy;
  }
  for (uint32_t p = 0; p < P && !spec; p++) {
    auto tp = std::chrono::steady_clock::now();
    const uint32_t ja = (uint32_t)((uint64_t)nch * p / P), jb = (uint32_t)((uint64_t)nch * (p + 1) / P);
    const size_t r0 = c->recs.size();
    if (int r = scan_piece(c, h, d_file, S, ja, jb)) return r;
    if (int r = ext_merge(c, h, d_file, F, S, E)) return r;
    if (p == 0) {
      t_begin.join();
      if (rc_begin) return rc_begin;
    }
    const size_t r1 = c->recs.size();
    if (int r = inflate_records(c, d_file, F, r0, r1, *c->slabs[p])) return r;
    if (int r = sweep_publish(c, R, r0, r1)) return r;
    scan_busy += ms_since(tp);
  }
  c->stats.scan_ms = scan_busy;   // the scan thread's own time (the sweep runs beside it)
  if (int r = sweep_finish(c, R)) return r;
  if (int r = strategy_pass(c, d_file, ss)) return r;
  if (int r = raw_pass(c, d_file, ss)) return r;
  c->infl_off.resize(c->recs.size());
  c->adler.resize(c->recs.size());
  bool nested = false;
  if (c->nest_depth)
    if (int r = nest_write(c, d_file, F, ss, atz_len, nested)) return r;
  if (!nested)
    if (int r = write_impl(c, d_file, F, ss, atz_len)) return r;
  c->stats.n_streams = c->recs.size();
  for (auto& s2 : ss) c->stats.n_recomp += s2.recomp;
  c->stats.atz_bytes = *atz_len;
  c->stats.total_ms = ms_since(t0);
  if (ss_out) ss_out->swap(ss);
  return 0;
}

// ---------------------------------------------------------------------------------------------
// one-shot deflates (reconstruct / atz_deflate): trials in "full output" mode on a temporary record
// set.  Stream s lives at absolute device address addr[s] (256-byte aligned), len[s] bytes, with its
// Adler-32 in adl[s] (host) or already in c->d_adler (adl empty).  The streams go in batches whose
// match tables / symbol buffers / outputs fit the round budget; after each batch on_batch(s0, s1,
// out_addr, out_len) sees the outputs (device addresses, valid until the next batch).
static int deflate_dev(atz_ctx* c, const std::vector<uint64_t>& addr, const std::vector<uint64_t>& len,
                       const std::vector<uint32_t>& adl, const std::vector<DeflSpec>& params,
                       const std::function<int(size_t, size_t, const std::vector<uint64_t>&,
                                               const std::vector<uint64_t>&)>& on_batch) {
  c->scan_valid = false; c->shard.stage = 0;   // recs / infl_off / adler / chain_off are replaced below
  const size_t n = addr.size();
  if (!n) return 0;
  c->recs.assign(n, Rec{});
  c->infl_off = addr;
  for (size_t s = 0; s < n; s++) {
    if (len[s] >= (1ull << 31)) return ATZ_E_ARG;   // trial kernels keep 32-bit positions
    c->recs[s].infl_len = len[s];
  }
  // k_buckets_sort reports each (stream, memLevel)'s deepest bucket at 10 s + m: sized for these streams
  // (a buffer left by an earlier call on fewer streams would be overrun)
  if (int r = c->depth_pin.reserve(n * 40 + 64)) return r;
  std::memset(c->depth_pin.p, 0xff, n * 40);
  if (!adl.empty()) {
    c->adler = adl;
    if (int r = upload(c, c->d_adler, c->adler.data(), n * 4)) return r;
  }
  std::vector<StreamDev> sd(n);
  for (size_t s = 0; s < n; s++) { sd[s].orig_off = 0; sd[s].infl_off = addr[s]; sd[s].comp_len = 0; sd[s].infl_len = len[s]; }
  if (int r = upload(c, c->d_streams, sd.data(), n * sizeof(StreamDev))) return r;
  if (int r = ensure_pipes(c, 1)) return r;
  HIPCHK(hipStreamSynchronize(c->st));   // tables (context stream) before the pipe's kernels
  Pipe* p = c->pipes[0].get();
  p->mw_cap = mw_cap_for(~(size_t)0);   // the large-sweep cap (or ATZ_MW)
  if (int r = c->d_tmp.reserve(4096)) return r;   // zero-length "file" for the compare side
  const uint64_t budget = cap_bytes(ROUND_BUDGET_BYTES);
  for (size_t s0 = 0; s0 < n;) {
    // a batch: streams until the scratch estimate passes the budget (at least one)
    size_t s1 = s0;
    uint64_t bytes = 0;
    while (s1 < n && (s1 == s0 || bytes <= budget)) {
      bytes += 9 * len[s1] + 4 * sym_words(p, 1, params[s1], len[s1]) + 4096;
      s1++;
    }
    c->chain_off.assign(n, {});
    std::vector<std::pair<uint32_t, int>> need;
    for (size_t s = s0; s < s1; s++)
      if (params[s].needs_tables()) need.push_back({(uint32_t)s, params[s].table_memlevel()});
    if (int r = private_chains(c, p, need)) return r;
    TrialBatch B;
    for (size_t s = s0; s < s1; s++) {
      const auto at = B.add(p, (uint32_t)s, len[s], params[s], TM_FULL, 0);
      if (at.first) B.tr[at.first][at.second].chain_off = c->chain_off[s][params[s].table_memlevel()];
    }
    if (int r = B.reserve(p)) return r;
    SweepOpts so{0, 0, 0, 0};
    std::vector<TrialRes> rr[3];
    if (int r = run_trials(c, p, c->d_tmp.as<uint8_t>(), B.tr, so, rr)) return r;
    std::vector<uint64_t> oa(s1 - s0), ol(s1 - s0);
    const uint64_t ob = (uint64_t)(uintptr_t)p->d_out.p;
    for (int k = 0; k < 3; k++)
      for (size_t q = 0; q < B.tr[k].size(); q++) {
        if (rr[k][q].state != TR_FULL) return ATZ_E_INTERNAL;
        oa[B.tr[k][q].stream - s0] = ob + B.tr[k][q].out_off;
        ol[B.tr[k][q].stream - s0] = rr[k][q].out_len;
      }
    if (int r = on_batch(s0, s1, oa, ol)) return r;
    s0 = s1;
  }
  return 0;
}

// Host inputs (atz_deflate / atz_deflate_batch): uploaded 256-byte aligned, Adler-32 on the host.
static int deflate_many(atz_ctx* c, const std::vector<std::pair<const uint8_t*, uint64_t>>& ins,
                        const std::vector<DeflSpec>& params, std::vector<std::vector<uint8_t>>& outs) {
  c->scan_valid = false; c->shard.stage = 0;
  const size_t n = ins.size();
  outs.assign(n, {});
  if (!n) return 0;
  uint64_t tot = 0;
  std::vector<uint64_t> off(n), addr(n), len(n);
  for (size_t s = 0; s < n; s++) { off[s] = tot; tot += (ins[s].second + 255) & ~255ull; }
  std::vector<uint8_t> hb(tot + 8);
  for (size_t s = 0; s < n; s++) if (ins[s].second) std::memcpy(hb.data() + off[s], ins[s].first, ins[s].second);
  if (int r = upload(c, c->d_infl, hb.data(), hb.size(), 65536)) return r;
  std::vector<uint32_t> adl(n);
  for (size_t s = 0; s < n; s++) {
    addr[s] = (uint64_t)(uintptr_t)c->d_infl.p + off[s];
    len[s] = ins[s].second;
    uint32_t a = 1, b = 0;
    for (uint64_t k = 0; k < ins[s].second; k++) { a = (a + ins[s].first[k]) % 65521; b = (b + a) % 65521; }
    adl[s] = (b << 16) | a;
  }
  return deflate_dev(c, addr, len, adl, params,
                     [&](size_t s0, size_t s1, const std::vector<uint64_t>& oa, const std::vector<uint64_t>& ol) -> int {
                       for (size_t s = s0; s < s1; s++) {
                         outs[s].resize(ol[s - s0]);
                         if (ol[s - s0])
                           HIPCHK(hipMemcpyAsync(outs[s].data(), (const void*)(uintptr_t)oa[s - s0], ol[s - s0],
                                                 hipMemcpyDeviceToHost, c->pipes[0]->st));
                       }
                       HIPCHK(hipStreamSynchronize(c->pipes[0]->st));
                       return 0;
                     });
}

// ---------------------------------------------------------------------------------------------
// Reconstruct (-r; ATZreconstructor::reconstructATZ, main.cpp:869-950) with the ATZ1 bytes resident
// in HBM: descriptors parsed on the host (h: host copy) and the plan made there (atz_format.h: parse_atz,
// plan_layout, plan_batch), payloads gathered into an aligned slab, Adler-32 on the device, one deflate
// per stream (doDeflate, main.cpp:976-1003), diff bytes patched (main.cpp:916-926) and the original
// assembled in c->d_rec by k_gather: residue gaps, the first comp_len bytes of each deflate output
// (zero-extended, as the reference's buffer is), the tail.
// P: where the payloads lie -- in the file, or (the stripped outer of a nested file) in the inner file's original.
static int reconstruct_flat(atz_ctx* c, const uint8_t* d_atz, const uint8_t* h, uint64_t n, uint64_t* out_len,
                            const PayloadSrc& P) {
  auto t0 = std::chrono::steady_clock::now();
  std::vector<AtzDesc> d;
  uint64_t origlen = 0, residue = 0;
  if (int r = parse_atz(h, n, d, origlen, residue, P.stripped, P.plen)) return r;
  if (int r = c->d_rec.reserve(origlen + 4096)) return r;
  const size_t ns = d.size();
  RecLayout L;
  if (int r = plan_layout(h, n, d, origlen, residue, L, P)) return r;
  const std::vector<uint8_t> meta(8, 0);
  // residue gaps and the tail are plain copies; the streams' segments come from their batches
  if (!L.gaps.empty())
    if (int r = gather_segments(c, d_atz, meta, L.gaps, c->d_rec.as<uint8_t>())) return r;
  if (ns) {
    // payloads into an aligned slab (the trial kernels read 256-byte aligned streams)
    if (c->slabs.empty()) c->slabs.emplace_back(new DBuf());
    DBuf& slab = *c->slabs[0];
    if (int r = slab.reserve(L.slab + 65536)) return r;
    std::vector<uint64_t> addr(ns), len(ns);
    for (size_t j = 0; j < ns; j++) { addr[j] = (uint64_t)(uintptr_t)slab.p + L.loc[j]; len[j] = d[j].il; }
    if (!L.payloads.empty())
      if (int r = gather_segments(c, d_atz, meta, L.payloads, slab.as<uint8_t>())) return r;
    // Adler-32 of every payload on the device
    if (int r = upload(c, c->d_pos, addr.data(), ns * 8)) return r;
    if (int r = upload(c, c->d_hbase, len.data(), ns * 8)) return r;
    if (int r = c->d_adler.reserve(ns * 4 + 4096)) return r;
    kbeg(c, 3);
    hipLaunchKernelGGL(k_adler32, dim3((uint32_t)ns), dim3(64), 0, c->st, c->d_pos.as<uint64_t>(),
                       c->d_hbase.as<uint64_t>(), c->d_adler.as<uint32_t>(), (uint32_t)ns);
    kend(c);
    KCHECK("k_adler32");
    HIPCHK(hipStreamSynchronize(c->st));
    kcollect(c);
    int rc2 = deflate_dev(c, addr, len, {}, L.params,
                          [&](size_t s0, size_t s1, const std::vector<uint64_t>& oa, const std::vector<uint64_t>& ol) -> int {
      RecBatch B;
      if (int r = plan_batch(h, d, L, origlen, s0, s1, oa, ol, (uint64_t)(uintptr_t)c->d_rec.p, B)) return r;
      if (!B.segs.empty())
        if (int r = gather_segments(c, d_atz, meta, B.segs, c->d_rec.as<uint8_t>())) return r;
      if (!B.pat.empty()) {
        if (int r = upload(c, c->d_diffjobs, B.pat.data(), B.pat.size() * 8)) return r;
        if (int r = upload(c, c->d_diffval, B.pval.data(), B.pval.size())) return r;
        kbeg(c, 3);
        hipLaunchKernelGGL(k_patch, dim3((uint32_t)((B.pat.size() + 255) / 256)), dim3(256), 0, c->st,
                           c->d_diffjobs.as<uint64_t>(), c->d_diffval.as<uint8_t>(), (uint64_t)B.pat.size());
        kend(c);
        KCHECK("k_patch");
        HIPCHK(hipStreamSynchronize(c->st));
        kcollect(c);
      }
      return 0;
    });
    if (rc2) return rc2;
  }
  HIPCHK(hipStreamSynchronize(c->st));
  *out_len = origlen;
  c->stats.total_ms = ms_since(t0);
  return 0;
}

// A nested file (h at its "ATN" header, accepted by parse_nest): the child rebuilds the inner file's original, P, from
// d_atz + offset and h + offset, into its d_rec; the outer's layout and batches then run as a flat file's, their
// payload segments sourced from P where it lies.
static int reconstruct_dev(atz_ctx* c, const uint8_t* d_atz, const uint8_t* h, uint64_t n, uint64_t* out_len,
                           bool checked = false) {
  if (!is_nest(h, n)) return reconstruct_flat(c, d_atz, h, n, out_len, PayloadSrc{});
  if (!checked) {
    std::vector<NestLevel> lv;
    if (int r = parse_nest(h, n, lv)) return r;
  }
  const uint64_t outer_len = rd8(h + 12), in = NEST_HEADER + outer_len;
  atz_ctx* k = nullptr;
  if (int r = nest_child(c, &k)) return r;
  k->scan_valid = false; k->shard.stage = 0;
  uint64_t plen = 0;
  {
    NestLend lend(c, k);   // (this context's deflates come after the child's)
    if (int r = reconstruct_dev(k, d_atz + in, h + in, n - in, &plen, true)) return r;
  }
  PayloadSrc P;
  P.stripped = true; P.pbase = (uint64_t)(uintptr_t)k->d_rec.p; P.plen = plen;
  return reconstruct_flat(c, d_atz + NEST_HEADER, h + NEST_HEADER, outer_len, out_len, P);
}

// ---------------------------------------------------------------------------------------------
// Multi-GPU precompress of one file: one process, context and GPU per rank, each
// holding the whole file in HBM.  Rank r inflates the scan candidates of its contiguous chunk range
// [nch*r/world, nch*(r+1)/world) (atz_shard_scan); the ranks all-gather those results, and each
// replays the whole file's greedy selection from them (the same record list on every rank: the
// replay is cheap host work, the inflates were the cost), then sweeps and writes the ATZ1
// descriptors of the records its chunk range produced (atz_shard_sweep).  Rank 0 gathers the pieces
// (RCCL over xGMI, by the caller) and adds the header and the residue (atz_shard_assemble).  The
// result is byte-identical to a one-GPU precompress of the file.
static constexpr uint64_t SHARD_MAGIC = 0x315348535a5441ull;   // "ATZSHS1"
static constexpr size_t SHARD_HDR = 7;                          // words

static void shard_range(uint32_t nch, int rank, int world, uint32_t& ja, uint32_t& jb) {
  ja = (uint32_t)((uint64_t)nch * (uint64_t)rank / (uint64_t)world);
  jb = (uint32_t)((uint64_t)nch * (uint64_t)(rank + 1) / (uint64_t)world);
}

// The sweep's split: contiguous record ranges (so the ATZ1 pieces concatenate in file order) of equal
// estimated cost.  A stream's sweep costs about I_s x the trials it runs, and the trial count is set
// by its header class: the class's list (main.cpp:487-560) is walked until the stream's own
// parameters are reached.  Mean trials per stream measured with the oracle on C4 (uniform clevel /
// memLevel): FLEVEL 0 5.8, 1 14.7, 2 5.5, 3 10.3.  A stream that matches no entry runs the whole
// list (81-82 entries): the scan flags the likely ones (Rec::noshort, k_inflate's first-block test:
// Z_FILTERED output such as C3's PNG-like streams, which no list entry reproduces).  Every rank
// computes the same split from the same record list (the hints travel in the scan blobs).  Records
// another rank's scan decoded are inflated again here (their scan output stays in that rank's arena).
static bool split_hint_on() {   // ATZ_SPLIT_HINT=0: round 3's fixed class weights (class 3: 20), no hint
  static const int v = [] { const char* e = std::getenv("ATZ_SPLIT_HINT"); return (int)(e ? std::atoi(e) : 1); }();
  return v != 0;
}
static uint64_t shard_cost(const Rec& r) {
  static constexpr uint64_t trials_by_class[4] = {6, 15, 6, 10};
  if (!split_hint_on()) return (r.infl_len + 1024) * ((r.type & 3) == 3 ? 20 : trials_by_class[r.type & 3]);
  return (r.infl_len + 1024) * (r.noshort ? 81 : trials_by_class[(uint32_t)r.type & 3u]);
}
static void shard_records(const std::vector<Rec>& recs, int rank, int world, size_t& r0, size_t& r1) {
  const size_t n = recs.size();
  std::vector<uint64_t> cum(n + 1, 0);
  for (size_t s = 0; s < n; s++) cum[s + 1] = cum[s] + shard_cost(recs[s]);
  auto cut = [&](int q) -> size_t {   // first record whose cost starts at or after q/world of the total
    if (q <= 0) return 0;
    if (q >= world) return n;
    const uint64_t goal = (uint64_t)((unsigned __int128)cum[n] * (unsigned)q / (unsigned)world);
    return (size_t)(std::lower_bound(cum.begin(), cum.end(), goal) - cum.begin());
  };
  r0 = std::min(cut(rank), n);
  r1 = std::max(r0, std::min(cut(rank + 1), n));
}

static int shard_scan_impl(atz_ctx* c, const uint8_t* d_file, const uint8_t* h, uint64_t F, int rank, int world,
                           std::vector<uint64_t>& blob) {
  atz_ctx::Shard& sh = c->shard;
  sh = atz_ctx::Shard{};
  sh.t0 = std::chrono::steady_clock::now();
  c->scan_valid = false; c->shard.stage = 0;
  c->stats = atz_stats_t{};
  c->stats.file_bytes = F;
  c->recs.clear();
  sh.S = std::make_shared<ScanState>();
  ScanState& S = *sh.S;
  if (int r = scan_plan(c, h, d_file, F, S)) return r;
  const uint32_t nch = (uint32_t)S.chunks.size();
  shard_range(nch, rank, world, sh.ja, sh.jb);
  if (sh.jb > sh.ja)   // the arena holds this rank's candidates only
    S.arena_cap = arena_cap_for(S.chunks[sh.jb - 1].co + S.chunks[sh.jb - 1].len - S.chunks[sh.ja].co);
  if (int r = scan_inflate(c, h, d_file, S, sh.ja, sh.jb)) return r;
  const size_t k0 = S.cbeg[sh.ja], k1 = S.cbeg[sh.jb];
  blob.assign(SHARD_HDR, 0);
  blob[0] = SHARD_MAGIC; blob[1] = (uint64_t)world; blob[2] = (uint64_t)rank; blob[3] = sh.ja; blob[4] = sh.jb;
  blob[5] = k1 - k0; blob[6] = F;
  blob.reserve(SHARD_HDR + 3 * (k1 - k0) + 4 * (sh.jb - sh.ja));
  for (size_t k = k0; k < k1; k++) {
    // status, with the candidate's hints in bits 32-35 (the first block's memLevel) and 36 (INF_HINT_NOSHORT)
    blob.push_back(S.cres[k].status | ((uint64_t)(S.cres[k].err >> INF_HINT_MLEV_SHIFT) << 32));
    blob.push_back(S.cres[k].consumed); blob.push_back(S.cres[k].produced);
  }
  for (uint32_t j = sh.ja; j < sh.jb; j++) {
    blob.push_back((uint64_t)(int64_t)S.pend0[j]);
    blob.push_back(S.cont0[j].status); blob.push_back(S.cont0[j].consumed); blob.push_back(S.cont0[j].produced);
  }
  sh.rank = rank; sh.world = world; sh.F = F;
  sh.stage = 1;
  c->stats.scan_ms = ms_since(sh.t0);
  return 0;
}

static int shard_sweep_impl(atz_ctx* c, const uint8_t* d_file, const uint8_t* h, uint64_t F,
                            const uint8_t* const* blobs, const uint64_t* blob_lens, int world,
                            std::vector<uint8_t>& flags, uint64_t* n_recomp) {
  atz_ctx::Shard& sh = c->shard;
  if (sh.stage != 1 || world != sh.world || F != sh.F || !blobs || !blob_lens) return ATZ_E_ARG;
  sh.stage = 0;
  auto t1 = std::chrono::steady_clock::now();
  ScanState& S = *sh.S;
  const uint32_t nch = (uint32_t)S.chunks.size();
  // the other ranks' candidate results and continuations (their arena outputs are theirs: the
  // records this rank keeps come from its own candidates, or are inflated again from the file)
  for (int q = 0; q < world; q++) {
    if (q == sh.rank) continue;
    if (!blobs[q] || blob_lens[q] % 8 || blob_lens[q] < SHARD_HDR * 8) return ATZ_E_ARG;
    const size_t nw = blob_lens[q] / 8;
    std::vector<uint64_t> b(nw);
    std::memcpy(b.data(), blobs[q], nw * 8);
    uint32_t ja, jb;
    shard_range(nch, q, world, ja, jb);
    const size_t k0 = S.cbeg[ja], k1 = S.cbeg[jb];
    if (b[0] != SHARD_MAGIC || b[1] != (uint64_t)world || b[2] != (uint64_t)q || b[3] != ja || b[4] != jb ||
        b[5] != k1 - k0 || b[6] != F || nw != SHARD_HDR + 3 * (k1 - k0) + 4 * (size_t)(jb - ja))
      return ATZ_E_ARG;
    const uint64_t* p = b.data() + SHARD_HDR;
    for (size_t k = k0; k < k1; k++, p += 3) {
      InfRes r{};
      r.status = (uint32_t)p[0]; r.consumed = p[1]; r.produced = p[2]; r.arena_off = ARENA_NONE;
      r.err = (uint32_t)((p[0] >> 32) & 31u) << INF_HINT_MLEV_SHIFT;
      S.cres[k] = r;
    }
    for (uint32_t j = ja; j < jb; j++, p += 4) {
      S.pend0[j] = (long)(int64_t)p[0];
      InfRes r{};
      r.status = (uint32_t)p[1]; r.consumed = p[2]; r.produced = p[3]; r.arena_off = ARENA_NONE;
      S.cont0[j] = r;
    }
  }
  // the whole file's replay (the same record list on every rank), then this rank's share of it
  c->recs.clear();
  c->recs.reserve(S.max_records());
  c->hfile = h; c->flen = F;
  struct Drop { atz_ctx* c; ~Drop() { c->hfile = nullptr; } } drop{c};
  if (int r = scan_replay(c, h, S, 0, nch)) return r;
  sh.all.resize(c->recs.size());
  for (size_t s = 0; s < c->recs.size(); s++) sh.all[s] = {c->recs[s].offset, c->recs[s].comp_len};
  size_t r0, r1;
  shard_records(c->recs, sh.rank, world, r0, r1);
  c->recs.erase(c->recs.begin() + r1, c->recs.end());
  c->recs.erase(c->recs.begin(), c->recs.begin() + r0);
  const size_t n = c->recs.size();
  if (c->slabs.empty()) c->slabs.emplace_back(new DBuf());
  if (int r = inflate_records(c, d_file, F, 0, n, *c->slabs[0])) return r;
  c->stats.scan_ms += ms_since(t1);
  std::vector<StreamState> ss;
  if (int r = sweep_impl(c, d_file, ss)) return r;
  // this rank's piece: descriptors + payloads of its recompressed streams
  auto t2 = std::chrono::steady_clock::now();
  std::vector<uint8_t> meta;
  std::vector<Seg> segs;
  uint64_t out = 0;
  write_descriptors(n, write_recs(c, ss), meta, segs, out);
  if (int r = c->d_atz.reserve(out + 4096)) return r;
  if (!segs.empty())
    if (int r = gather_segments(c, d_file, meta, segs, c->d_atz.as<uint8_t>())) return r;
  sh.piece_len = out;
  flags.resize(n);
  uint64_t nr = 0;
  for (size_t s = 0; s < n; s++) { flags[s] = ss[s].recomp; nr += ss[s].recomp; }
  *n_recomp = nr;
  c->stats.n_streams = n;
  c->stats.n_recomp = nr;
  c->stats.atz_bytes = out;
  c->stats.write_ms = ms_since(t2);
  c->stats.total_ms = ms_since(sh.t0);
  sh.stage = 2;
  return 0;
}

static int shard_assemble_impl(atz_ctx* c, const uint8_t* d_file, uint64_t F, const uint8_t* flags, uint64_t n_flags,
                               uint64_t n_recomp, uint64_t pieces_len, uint8_t* d_atz, uint64_t cap, uint64_t* atz_len) {
  atz_ctx::Shard& sh = c->shard;
  if (sh.stage != 2 || sh.rank != 0 || F != sh.F || n_flags != sh.all.size() || (!flags && n_flags) || !d_atz)
    return ATZ_E_ARG;
  uint64_t nr = 0;
  for (uint64_t s = 0; s < n_flags; s++) nr += flags[s] != 0;
  if (nr != n_recomp) return ATZ_E_ARG;
  std::vector<uint8_t> meta;
  std::vector<Seg> segs;
  uint64_t out = write_header(meta, segs, F, n_recomp, 1) + pieces_len;   // the pieces are already in place
  if (int r = write_residue(sh.all, flags, F, segs, out)) return r;
  if (out > cap) return ATZ_E_ARG;
  write_length(meta, out);
  if (int r = gather_segments(c, d_file, meta, segs, d_atz)) return r;
  *atz_len = out;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// No C++ exception crosses the C ABI (std::vector growth, new): allocation failures become
// ATZ_E_NOMEM, anything else ATZ_E_INTERNAL.
template <class F>
static int guarded(F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return ATZ_E_NOMEM;
  } catch (const std::length_error&) {
    return ATZ_E_NOMEM;
  } catch (...) {
    return ATZ_E_INTERNAL;
  }
}

extern "C" {

void atz_default_opts(atz_opts_t* o) {
  o->recomp_tresh = 128; o->sizediff_tresh = 128; o->shortcut_len = 512; o->mismatch_tol = 2;
  o->chunksize = 524288; o->brute_window = 0; o->device = -1;
}

const char* atz_strerror(int e) {
  switch (e) {
    case ATZ_OK: return "ok";
    case ATZ_E_ARG: return "invalid argument";
    case ATZ_E_NODEV: return "no usable HIP device (gfx950 kernels not loadable)";
    case ATZ_E_HIP: return "HIP runtime error";
    case ATZ_E_NOMEM: return "out of memory";
    case ATZ_E_REF_ABORT: return "the reference aborts on this input (inflate/deflate failure)";
    case ATZ_E_REF_UB: return "the reference has undefined behaviour on this input";
    case ATZ_E_FORMAT: return "invalid ATZ file";
    default: return "internal error";
  }
}

void atz_free(void* p) { std::free(p); }

int atz_open(atz_ctx_t** ctx, const atz_opts_t* opts) {
  return guarded([&]() -> int {
    if (!ctx) return ATZ_E_ARG;
    *ctx = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ATZ_E_NODEV;
    atz_ctx* c = new atz_ctx();
    if (opts) c->o = *opts; else atz_default_opts(&c->o);
    c->dev = c->o.device >= 0 ? c->o.device : 0;
    if (c->o.device >= 0 && hipSetDevice(c->dev) != hipSuccess) { delete c; return ATZ_E_NODEV; }
    if (c->o.device < 0) hipGetDevice(&c->dev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->dev) != hipSuccess) { delete c; return ATZ_E_NODEV; }
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
      std::fprintf(stderr, "atz: device %d is %s, kernels are built for gfx950\n", c->dev, prop.gcnArchName);
      delete c;
      return ATZ_E_NODEV;
    }
    if (hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess) { delete c; return ATZ_E_HIP; }
    DeflTables T;
    make_tables(T);
    if (atz_upload_defl_tables(&T) != hipSuccess) { delete c; return ATZ_E_NODEV; }
    *ctx = c;
    return ATZ_OK;
  });
}

void atz_close(atz_ctx_t* c) {
  if (!c) return;
  try {
    close_ctx(c);   // (and its nesting children)
  } catch (...) {
  }
}

int atz_scan(atz_ctx_t* c, const uint8_t* file, uint64_t len, atz_cand_t** out, uint64_t* n) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || (!file && len) || !out || !n) return ATZ_E_ARG;
    c->scan_valid = false; c->shard.stage = 0;
    if (int r = upload(c, c->d_file, file, len)) return r;
    c->hfile = file; c->flen = len;
    c->stats = atz_stats_t{};
    const int rs = scan_impl(c, file, c->d_file.as<uint8_t>(), len);
    c->hfile = nullptr;   // the caller's buffer is not used after this call returns
    if (rs) return rs;
    // atz_sweep needs each stream's Adler-32 trailer: keep it, so `file` may be freed in between
    c->scan_trailer.assign(c->recs.size(), 0);
    for (size_t s = 0; s < c->recs.size(); s++) {
      const Rec& r = c->recs[s];
      if (r.comp_len < 4 || r.offset + r.hull() > len) continue;   // atz_sweep reports ATZ_E_REF_UB
      c->scan_trailer[s] = rec_trailer(r, file, c->st_off, c->st_len);
    }
    *n = c->recs.size();
    *out = (atz_cand_t*)std::malloc((c->recs.size() + 1) * sizeof(atz_cand_t));
    if (!*out) return ATZ_E_NOMEM;
    for (size_t s = 0; s < c->recs.size(); s++) {
      (*out)[s].offset = c->recs[s].offset; (*out)[s].comp_len = c->recs[s].comp_len;
      (*out)[s].infl_len = c->recs[s].infl_len; (*out)[s].type = c->recs[s].type;
      (*out)[s].flags = c->recs[s].flags | (c->recs[s].noshort ? 2u : 0u) | ((uint32_t)c->recs[s].mhint << 2) |
                        (c->recs[s].stitch != ~0ull ? 64u : 0u);
    }
    c->scan_valid = true;
    return ATZ_OK;
  });
}

int atz_sweep(atz_ctx_t* c, const atz_cand_t* cands, uint64_t n, atz_result_t* res, uint64_t** diff_off,
              uint8_t** diff_val, uint64_t* n_diffs) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    // only on the records of this context's last atz_scan (nothing in between replaced them)
    if (!c || !res || !c->scan_valid || n != c->recs.size()) return ATZ_E_ARG;
    (void)cands;
    c->scan_valid = false; c->shard.stage = 0;   // inflate_records / the sweep overwrite the scan's device state
    c->hfile = nullptr;
    if (c->slabs.empty()) c->slabs.emplace_back(new DBuf());
    if (int r = inflate_records(c, c->d_file.as<uint8_t>(), c->flen, 0, c->recs.size(), *c->slabs[0])) return r;
    std::vector<StreamState> ss;
    c->exact_idents = true;   // every stream's result is reported (elig_floor)
    const int rs = sweep_impl(c, c->d_file.as<uint8_t>(), ss);
    c->exact_idents = false;
    if (rs) return rs;
    uint64_t nd = 0;
    for (auto& s : ss) if (s.recomp) nd += s.rawdiff.size();
    uint64_t* dof = (uint64_t*)std::malloc((nd + 1) * 8);
    uint8_t* dva = (uint8_t*)std::malloc(nd + 1);
    uint64_t k = 0;
    for (size_t s = 0; s < n; s++) {
      const StreamState& st = ss[s];
      atz_result_t& r = res[s];
      r.clevel = st.c; r.window = st.w; r.memlevel = st.m; r.recomp = st.recomp;
      r.n_trials = st.trials; r.ident = st.ident; r.first_diff = st.first_diff;
      r.diff_index = k;
      r.n_diff = st.recomp ? st.rawdiff.size() : 0;
      if (st.recomp)
        for (size_t q = 0; q < st.rawdiff.size(); q++, k++) {
          dof[k] = q == 0 ? 0 : (uint64_t)st.rawdiff[q] - st.rawdiff[q - 1];
          dva[k] = st.diffval[q];
        }
    }
    *diff_off = dof; *diff_val = dva; *n_diffs = nd;
    return ATZ_OK;
  });
}

// The host ATZ1 buffer of atz_precompress.  A D2H copy into a fresh 1.5 GB malloc buffer took ~155 ms
// (first-touch page faults, the kernel zeroing every page, and the runtime's staging of pageable
// memory), against ~28 ms into pinned memory (tools/h2h_probe.py).  So while the GPU sweeps, a helper
// thread allocates a buffer of the estimated size, touches its pages and registers it with HIP; the
// ATZ1 is then copied at DMA speed and the buffer unregistered before the caller gets it (a plain
// malloc buffer, atz_free).
struct HostOut {
  static constexpr uint64_t PIECE = 64ull << 20;   // registered in pieces: no long hold of the driver's locks
  uint8_t* p = nullptr;
  uint64_t cap = 0;
  std::vector<uint64_t> reg;   // registered pieces [k * PIECE, ...), in order
  double t_reg = 0;
  int mode = 2;                // ATZ_H2H_PREP: 0 plain malloc at the end, 1 touch, 2 touch + register
  std::thread th;
  HostOut() { const char* e = std::getenv("ATZ_H2H_PREP"); if (e) mode = std::atoi(e); }
  void start(uint64_t est) {
    if (mode <= 0 || p || th.joinable()) return;
    p = (uint8_t*)std::malloc(est + 1);
    if (!p) return;
    cap = est;
    th = std::thread([this]() {
      const auto t0 = std::chrono::steady_clock::now();
      const uint64_t n = cap + 1;
      for (uint64_t a = 0; a < n; a += PIECE) {
        const uint64_t b = std::min<uint64_t>(n, a + PIECE);
        volatile uint8_t* q = p;
        for (uint64_t k = a; k < b; k += 4096) q[k] = 0;
        if (mode >= 2) {
          if (hipHostRegister(p + a, b - a, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); mode = 1; }
          else reg.push_back(a);
        }
      }
      t_reg = ms_since(t0);
    });
  }
  void join() { if (th.joinable()) th.join(); }
  uint8_t* take(uint64_t n) {   // a buffer of at least n bytes
    join();
    uint8_t* r = p;
    if (r && n > cap + 1) {
      if (timing_on())
        std::fprintf(stderr, "atz: host ATZ1 buffer: %llu bytes estimated, %llu needed (reallocated, unregistered copy)\n",
                     (unsigned long long)cap, (unsigned long long)n);
      unreg();
      uint8_t* g = (uint8_t*)std::realloc(r, n);
      if (!g) std::free(r);
      r = g;
    } else if (!r) {
      r = (uint8_t*)std::malloc(n);
    }
    p = r; cap = r ? n - 1 : 0;
    return r;
  }
  // the D2H: registered pieces one copy each (a copy never spans two registrations), the rest plain
  hipError_t copy_from(const void* d, uint64_t n, hipStream_t st) {
    uint64_t done = 0;
    for (uint64_t a : reg) {
      if (a >= n) break;
      const uint64_t b = std::min<uint64_t>(n, a + PIECE);
      const hipError_t e = hipMemcpyAsync(p + a, (const uint8_t*)d + a, b - a, hipMemcpyDeviceToHost, st);
      if (e != hipSuccess) return e;
      done = b;
    }
    if (hipError_t e = hipStreamSynchronize(st)) return e;
    return done < n ? hipMemcpy(p + done, (const uint8_t*)d + done, n - done, hipMemcpyDeviceToHost) : hipSuccess;
  }
  void unreg() { for (uint64_t a : reg) (void)hipHostUnregister(p + a); reg.clear(); }
  uint8_t* release() { unreg(); uint8_t* r = p; p = nullptr; cap = 0; return r; }
  ~HostOut() { join(); unreg(); std::free(p); }
};

int atz_precompress(atz_ctx_t* c, const uint8_t* file, uint64_t len, uint8_t** atz, uint64_t* atz_len,
                    atz_stats_t* stats) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || (!file && len) || !atz || !atz_len) return ATZ_E_ARG;
    dev_mark_call();
    const auto t0 = std::chrono::steady_clock::now();
    if (int r = upload(c, c->d_file, file, len)) return r;
    HIPCHK(hipStreamSynchronize(c->st));
    const double t_up = ms_since(t0);
    uint64_t al = 0;
    HostOut ho;
    c->on_records = [&ho](uint64_t est) { ho.start(est); };
    struct Reset { atz_ctx* c; ~Reset() { c->on_records = nullptr; } } reset{c};
    if (int r = precompress_dev(c, c->d_file.as<uint8_t>(), file, len, &al, nullptr)) return r;
    c->on_records = nullptr;
    const double t_dev = ms_since(t0);
    uint8_t* h = ho.take(al + 1);
    if (!h) return ATZ_E_NOMEM;
    const double t_take = ms_since(t0);
    HIPCHK(ho.copy_from(c->d_atz.p, al, c->st));
    const double t_d2h = ms_since(t0);
    h = ho.release();
    if (timing_on() || std::getenv("ATZ_H2H_TIMING"))
      std::fprintf(stderr, "atz: host path: upload %.1f ms, device %.1f ms, host buffer wait %.1f ms (touch + "
                   "register %.1f ms on the helper), D2H %.1f ms, unregister %.1f ms\n", t_up, t_dev - t_up,
                   t_take - t_dev, ho.t_reg, t_d2h - t_take, ms_since(t0) - t_d2h);
    *atz = h; *atz_len = al;
    c->stats.dev_bytes_peak = g_dev.peak.load(); c->stats.dev_bytes_held = g_dev.cur.load();
    if (stats) *stats = c->stats;
    return ATZ_OK;
  });
}

int atz_precompress_device(atz_ctx_t* c, const uint8_t* d_file, const uint8_t* h_file, uint64_t len,
                           const uint8_t** d_atz, uint64_t* atz_len, atz_stats_t* stats) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || !d_file || !h_file || !d_atz || !atz_len) return ATZ_E_ARG;
    dev_mark_call();
    HostProf prof;
    uint64_t al = 0;
    auto tc = std::chrono::steady_clock::now();
    if (int r = precompress_dev(c, d_file, h_file, len, &al, nullptr)) return r;
    if (timing_on())
      std::fprintf(stderr, "atz: precompress call %.2f ms (inside: %.2f ms)\n", ms_since(tc), c->stats.total_ms);
    *d_atz = c->d_atz.as<uint8_t>();
    *atz_len = al;
    c->stats.dev_bytes_peak = g_dev.peak.load(); c->stats.dev_bytes_held = g_dev.cur.load();
    if (stats) *stats = c->stats;
    return ATZ_OK;
  });
}

uint64_t atz_deflate_bound(uint64_t n, int window, int memlevel) { return bound(n, window, memlevel); }

int atz_deflate(atz_ctx_t* c, const uint8_t* in, uint64_t in_len, int clevel, int window, int memlevel,
                uint8_t* out, uint64_t out_cap, uint64_t* out_len) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || (!in && in_len) || !out_len || clevel < 0 || clevel > 9 || window < 8 || window > 15 ||
        memlevel < 1 || memlevel > 9)
      return ATZ_E_ARG;
    DeflSpec p;
    p.level = clevel; p.window = window == 8 ? 9 : window; p.memlevel = memlevel;
    std::vector<std::vector<uint8_t>> outs;
    if (int r = deflate_many(c, {{in, in_len}}, {p}, outs)) return r;
    *out_len = outs[0].size();
    if (outs[0].size() > out_cap) return ATZ_E_ARG;
    if (out && !outs[0].empty()) std::memcpy(out, outs[0].data(), outs[0].size());
    return ATZ_OK;
  });
}

// ex: atz_deflate_batch_ex's reading of the params words (valid_api, atz_params.h)
static int deflate_batch_api(atz_ctx_t* c, const uint8_t* buf, uint64_t len, const uint64_t* offs, const uint64_t* lens,
                             const uint32_t* params, uint64_t n, uint8_t* out, const uint64_t* out_offs,
                             const uint64_t* out_caps, uint64_t* out_lens, bool ex) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || (!buf && len) || !out_lens) return ATZ_E_ARG;
    std::vector<std::pair<const uint8_t*, uint64_t>> ins(n);
    std::vector<DeflSpec> ps(n);
    for (uint64_t k = 0; k < n; k++) {
      if (offs[k] + lens[k] > len || !valid_api(params[k], ex, &ps[k])) return ATZ_E_ARG;
      ins[k] = {buf + offs[k], lens[k]};
    }
    std::vector<std::vector<uint8_t>> outs;
    if (int r = deflate_many(c, ins, ps, outs)) return r;
    for (uint64_t k = 0; k < n; k++) {
      out_lens[k] = outs[k].size();
      if (outs[k].size() > out_caps[k]) return ATZ_E_ARG;
      if (!outs[k].empty()) std::memcpy(out + out_offs[k], outs[k].data(), outs[k].size());
    }
    return ATZ_OK;
  });
}

int atz_deflate_batch(atz_ctx_t* c, const uint8_t* buf, uint64_t len, const uint64_t* offs, const uint64_t* lens,
                      const uint32_t* params, uint64_t n, uint8_t* out, const uint64_t* out_offs,
                      const uint64_t* out_caps, uint64_t* out_lens) {
  return deflate_batch_api(c, buf, len, offs, lens, params, n, out, out_offs, out_caps, out_lens, false);
}

int atz_deflate_batch_ex(atz_ctx_t* c, const uint8_t* buf, uint64_t len, const uint64_t* offs, const uint64_t* lens,
                         const uint32_t* params, uint64_t n, uint8_t* out, const uint64_t* out_offs,
                         const uint64_t* out_caps, uint64_t* out_lens) {
  return deflate_batch_api(c, buf, len, offs, lens, params, n, out, out_offs, out_caps, out_lens, true);
}

int atz_set_strategies(atz_ctx_t* c, uint32_t mask) {
  if (!c || (mask & ~14u)) return ATZ_E_ARG;   // bits 1..3: Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE
  c->strat_mask = mask;
  return ATZ_OK;
}

int atz_set_containers(atz_ctx_t* c, uint32_t mask) {
  if (!c || (mask & ~3u)) return ATZ_E_ARG;   // bit 0: ZIP local file headers, bit 1: gzip members
  c->cont_mask = mask;
  c->scan_valid = false;
  return ATZ_OK;
}

int atz_container_anchors(atz_ctx_t* c, const uint8_t* file, uint64_t len, uint32_t mask, uint64_t** out, uint64_t* n) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || (!file && len) || !out || !n || (mask & ~3u)) return ATZ_E_ARG;
    c->scan_valid = false; c->shard.stage = 0;   // d_file is replaced
    if (int r = upload(c, c->d_file, file, len)) return r;
    std::vector<uint64_t> a;
    if (int r = anchors_dev(c, c->d_file.as<uint8_t>(), len, mask, a)) return r;
    *out = (uint64_t*)std::malloc((a.size() + 1) * 8);
    if (!*out) return ATZ_E_NOMEM;
    if (!a.empty()) std::memcpy(*out, a.data(), a.size() * 8);
    *n = a.size();
    return ATZ_OK;
  });
}

int atz_set_stitch(atz_ctx_t* c, uint32_t mask) {
  if (!c || (mask & ~1u)) return ATZ_E_ARG;   // bit 0: PNG IDAT chains
  c->stitch_mask = mask;
  c->scan_valid = false;
  return ATZ_OK;
}

int atz_stitch_anchors(atz_ctx_t* c, const uint8_t* file, uint64_t len, uint32_t mask, uint64_t** out, uint64_t* n) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || (!file && len) || !out || !n || (mask & ~1u)) return ATZ_E_ARG;
    c->scan_valid = false; c->shard.stage = 0;   // d_file is replaced
    if (int r = upload(c, c->d_file, file, len)) return r;
    std::vector<uint64_t> a;
    if (int r = anchors_dev(c, c->d_file.as<uint8_t>(), len, (mask & 1u) ? 4u : 0u, a)) return r;
    *out = (uint64_t*)std::malloc((a.size() + 1) * 8);
    if (!*out) return ATZ_E_NOMEM;
    if (!a.empty()) std::memcpy(*out, a.data(), a.size() * 8);
    *n = a.size();
    return ATZ_OK;
  });
}

int atz_set_probe(atz_ctx_t* c, uint32_t mask) {
  if (!c || (mask & ~1u)) return ATZ_E_ARG;   // bit 0: raw deflate starts whose first block is dynamic
  c->probe_mask = mask;
  c->scan_valid = false;
  return ATZ_OK;
}

int atz_set_deflaters(atz_ctx_t* c, uint32_t mask) {
  if (!c || (mask & ~1u)) return ATZ_E_ARG;   // bit 0: GNU gzip's and Info-ZIP's deflater, for raw records
  c->defl_mask = mask;
  return ATZ_OK;
}

int atz_set_segments(atz_ctx_t* c, uint32_t mask) {
  if (!c || (mask & ~1u)) return ATZ_E_ARG;   // bit 0: full-flush points
  c->seg_mask = mask;
  c->scan_valid = false;
  return ATZ_OK;
}

int atz_set_nesting(atz_ctx_t* c, int depth) {
  if (!c || depth < 0 || depth > 4) return ATZ_E_ARG;
  c->nest_depth = depth;
  c->nest_ran = false;
  return ATZ_OK;
}

int atz_nest_stats(atz_ctx_t* c, int level, atz_stats_t* stats) {
  if (!c || !stats || level < 0 || level > 4) return ATZ_E_ARG;
  const atz_ctx* k = c;
  for (int l = 0; l < level; l++) {   // level l + 1 ran in level l's last precompress
    if (!k->nest_depth || !k->nest_ran || !k->nest_child) return ATZ_E_ARG;
    k = k->nest_child;
  }
  *stats = k->stats;
  return ATZ_OK;
}

int atz_flush_markers(atz_ctx_t* c, const uint8_t* file, uint64_t len, uint64_t** out, uint64_t* n) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || (!file && len) || !out || !n) return ATZ_E_ARG;
    c->scan_valid = false; c->shard.stage = 0;   // d_file is replaced
    if (int r = upload(c, c->d_file, file, len)) return r;
    MarkerList ml;
    if (int r = markers_dev(c, c->d_file.as<uint8_t>(), len, ml)) return r;
    if (timing_on())
      std::fprintf(stderr, "atz: k_marker_ordered: %zu markers, kernels %.3f ms (both passes)\n", ml.pos.size(), ml.kernel_ms);
    *out = (uint64_t*)std::malloc((ml.pos.size() + 1) * 8);
    if (!*out) return ATZ_E_NOMEM;
    if (!ml.pos.empty()) std::memcpy(*out, ml.pos.data(), ml.pos.size() * 8);
    *n = ml.pos.size();
    return ATZ_OK;
  });
}

int atz_probe_positions(atz_ctx_t* c, const uint8_t* file, uint64_t len, uint64_t** out, uint64_t* n) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || (!file && len) || !out || !n) return ATZ_E_ARG;
    c->scan_valid = false; c->shard.stage = 0;   // d_file is replaced
    if (int r = upload(c, c->d_file, file, len)) return r;
    ProbeList pl;
    if (int r = probe_dev(c, c->d_file.as<uint8_t>(), len, pl)) return r;
    *out = (uint64_t*)std::malloc((pl.pos.size() + 1) * 8);
    if (!*out) return ATZ_E_NOMEM;
    if (!pl.pos.empty()) std::memcpy(*out, pl.pos.data(), pl.pos.size() * 8);
    *n = pl.pos.size();
    return ATZ_OK;
  });
}

int atz_stitch_pieces(atz_ctx_t* c, uint64_t record, uint64_t** offs, uint64_t** lens, uint64_t* k) {
  return guarded([&]() -> int {
    if (!c || !offs || !lens || !k || !c->scan_valid || record >= c->recs.size()) return ATZ_E_ARG;
    const Rec& r = c->recs[record];
    const uint64_t n = r.stitch != ~0ull ? r.pk : 0;
    *offs = (uint64_t*)std::malloc((n + 1) * 8);
    *lens = (uint64_t*)std::malloc((n + 1) * 8);
    if (!*offs || !*lens) { std::free(*offs); std::free(*lens); return ATZ_E_NOMEM; }
    for (uint64_t q = 0; q < n; q++) { (*offs)[q] = c->st_off[r.p0 + q]; (*lens)[q] = c->st_len[r.p0 + q]; }
    *k = n;
    return ATZ_OK;
  });
}

// seg: k_inflate's SEG variant on raw bodies (atz_inflate_segments); at_marker[k]: job k ended at a flush marker
static int inflate_batch_api(atz_ctx_t* c, const uint8_t* buf, uint64_t len, const uint64_t* offs, const uint64_t* lens,
                             uint64_t n, uint32_t* status, uint64_t* consumed, uint64_t* produced, bool seg,
                             uint8_t* at_marker) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || (!buf && len) || (seg && !at_marker)) return ATZ_E_ARG;
    c->scan_valid = false; c->shard.stage = 0;   // the arena holds the last scan's kept outputs
    if (int r = upload(c, c->d_tmp, buf, len)) return r;
    std::vector<InfJob> jobs(n);
    for (uint64_t k = 0; k < n; k++) {
      if (offs[k] + lens[k] > len) return ATZ_E_ARG;
      // the scan's configuration: output into arena slots (small-ring decoder, 32 KiB-ring reruns)
      jobs[k].in_off = offs[k]; jobs[k].in_len = lens[k]; jobs[k].out_off = ARENA_OUT; jobs[k].out_cap = ARENA_SLOT;
    }
    std::vector<InfRes> res;
    const uint64_t arena_cap = cap_bytes(std::min<uint64_t>(64ull << 30, std::max<uint64_t>(256ull << 20, n * ARENA_SLOT)));
    if (int r = run_inflate_jobs(c, c->d_tmp.as<uint8_t>(), nullptr, jobs, res, arena_cap, false, true, seg ? INF_SEG : 0)) return r;
    for (uint64_t k = 0; k < n; k++) {
      status[k] = res[k].status; consumed[k] = res[k].consumed; produced[k] = res[k].produced;
      if (seg) at_marker[k] = res[k].status == INF_END && (res[k].err & INF_AT_MARKER) ? 1 : 0;
    }
    return ATZ_OK;
  });
}

int atz_inflate_batch(atz_ctx_t* c, const uint8_t* buf, uint64_t len, const uint64_t* offs, const uint64_t* lens,
                      uint64_t n, uint32_t* status, uint64_t* consumed, uint64_t* produced) {
  return inflate_batch_api(c, buf, len, offs, lens, n, status, consumed, produced, false, nullptr);
}

int atz_inflate_segments(atz_ctx_t* c, const uint8_t* buf, uint64_t len, const uint64_t* offs, const uint64_t* lens,
                         uint64_t n, uint32_t* status, uint64_t* consumed, uint64_t* produced, uint8_t* at_marker) {
  return inflate_batch_api(c, buf, len, offs, lens, n, status, consumed, produced, true, at_marker);
}

int atz_shard_scan(atz_ctx_t* c, const uint8_t* d_file, const uint8_t* h_file, uint64_t len, int rank, int world,
                   uint8_t** blob, uint64_t* blob_len) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || !d_file || !h_file || !blob || !blob_len || world < 1 || rank < 0 || rank >= world) return ATZ_E_ARG;
    if (c->strat_mask || c->cont_mask || c->stitch_mask || c->probe_mask || c->defl_mask || c->seg_mask || c->nest_depth) return ATZ_E_ARG;   // the extensions have no multi-GPU split
    dev_mark_call();   // (the peak runs on through atz_shard_sweep, whose stats report it)
    std::vector<uint64_t> b;
    if (int r = shard_scan_impl(c, d_file, h_file, len, rank, world, b)) { c->shard.stage = 0; return r; }
    uint8_t* p = (uint8_t*)std::malloc(b.size() * 8 + 1);
    if (!p) return ATZ_E_NOMEM;
    std::memcpy(p, b.data(), b.size() * 8);
    *blob = p; *blob_len = b.size() * 8;
    return ATZ_OK;
  });
}

int atz_shard_sweep(atz_ctx_t* c, const uint8_t* d_file, const uint8_t* h_file, uint64_t len,
                    const uint8_t* const* blobs, const uint64_t* blob_lens, int world, uint64_t* piece_len,
                    uint8_t** recomp_flags, uint64_t* n_flags, uint64_t* n_recomp, atz_stats_t* stats) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || !d_file || !h_file || !piece_len || !recomp_flags || !n_flags || !n_recomp) return ATZ_E_ARG;
    if (c->strat_mask || c->cont_mask || c->stitch_mask || c->probe_mask || c->defl_mask || c->seg_mask || c->nest_depth) return ATZ_E_ARG;
    std::vector<uint8_t> f;
    if (int r = shard_sweep_impl(c, d_file, h_file, len, blobs, blob_lens, world, f, n_recomp)) {
      c->shard.stage = 0;
      return r;
    }
    uint8_t* p = (uint8_t*)std::malloc(f.size() + 1);
    if (!p) return ATZ_E_NOMEM;
    if (!f.empty()) std::memcpy(p, f.data(), f.size());
    *recomp_flags = p; *n_flags = f.size();
    *piece_len = c->shard.piece_len;
    c->stats.dev_bytes_peak = g_dev.peak.load(); c->stats.dev_bytes_held = g_dev.cur.load();
    if (stats) *stats = c->stats;
    return ATZ_OK;
  });
}

int atz_shard_piece(atz_ctx_t* c, uint8_t* d_dst) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || c->nest_depth || c->shard.stage != 2 || (!d_dst && c->shard.piece_len)) return ATZ_E_ARG;
    if (c->shard.piece_len)
      HIPCHK(hipMemcpyAsync(d_dst, c->d_atz.p, c->shard.piece_len, hipMemcpyDeviceToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return ATZ_OK;
  });
}

int atz_shard_assemble(atz_ctx_t* c, const uint8_t* d_file, uint64_t len, const uint8_t* recomp_flags,
                       uint64_t n_flags, uint64_t n_recomp, uint64_t pieces_len, uint8_t* d_atz, uint64_t cap,
                       uint64_t* atz_len) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || !d_file || !atz_len || c->nest_depth) return ATZ_E_ARG;
    return shard_assemble_impl(c, d_file, len, recomp_flags, n_flags, n_recomp, pieces_len, d_atz, cap, atz_len);
  });
}


int atz_reconstruct(atz_ctx_t* c, const uint8_t* atz, uint64_t n, uint8_t** out, uint64_t* out_len) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || !atz || !out || !out_len) return ATZ_E_ARG;
    c->scan_valid = false; c->shard.stage = 0;
    if (int r = upload(c, c->d_atzin, atz, n)) return r;
    uint64_t L = 0;
    if (int r = reconstruct_dev(c, c->d_atzin.as<uint8_t>(), atz, n, &L)) return r;
    uint8_t* h = (uint8_t*)std::malloc(L + 1);
    if (!h) return ATZ_E_NOMEM;
    if (L) {
      const hipError_t e = hipMemcpy(h, c->d_rec.p, L, hipMemcpyDeviceToHost);
      if (e != hipSuccess) { std::free(h); return ATZ_E_HIP; }
    }
    *out = h; *out_len = L;
    return ATZ_OK;
  });
}

int atz_reconstruct_device(atz_ctx_t* c, const uint8_t* d_atz, const uint8_t* h_atz, uint64_t len,
                           const uint8_t** d_out, uint64_t* out_len) {
  return guarded([&]() -> int {
    (void)hipGetLastError();
    if (!c || !d_atz || !h_atz || !d_out || !out_len) return ATZ_E_ARG;
    c->scan_valid = false; c->shard.stage = 0;
    uint64_t L = 0;
    if (int r = reconstruct_dev(c, d_atz, h_atz, len, &L)) return r;
    *d_out = c->d_rec.as<uint8_t>();
    *out_len = L;
    return ATZ_OK;
  });
}

}  // extern "C"
