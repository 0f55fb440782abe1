// mhx_core — drop-in for `megahit_core count | read2sdbg | seq2sdbg` (reference
// src/main_sdbg_build.cpp:35-224, dispatched from src/main.cpp:68-110): same flags, same on-disk
// inputs and outputs, the sorting engines replaced by libmhx (HIP, gfx950) through its C ABI.
//
// Sub-programs outside the SdBG-construction path (buildlib, assemble, iterate, local, ...) are not
// implemented here; when MHX_REF_CORE names a reference `megahit_core` binary they are forwarded to
// it unchanged, so the unmodified `megahit` orchestrator can run with this binary in place.
#include <atomic>
#include <chrono>
#include <cmath>
#include <unistd.h>
#include <fcntl.h>
#include <poll.h>
#include <signal.h>
#include <sys/prctl.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <sys/un.h>
#include <sys/wait.h>
#include <cerrno>

#include <algorithm>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../bgzf_scan.h"
#include "formats.h"
#include "mhx.h"

// how much room the store of the sorted edges gets for mercy edges: the reference reserves 25 % more than the edges, or
// MEGAHIT_NUM_MERCY_FACTOR times more when that is set (SeqToSdbg::Initialize, src/sorting/seq_to_sdbg.cpp:370-378)
static long long mercy_reserve_permille() {
  if (const char *f = getenv("MEGAHIT_NUM_MERCY_FACTOR")) {
    char *end = nullptr;
    const double v = strtod(f, &end);
    if (end != f && v >= 0) return (long long)std::min(100000.0, 1000.0 * (1.0 + v));
  }
  return 1250;
}

extern char **environ;

using mhxio::fatal;
using mhxio::info;

namespace {

struct Timer {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double lap() {
    auto t1 = std::chrono::steady_clock::now();
    double s = std::chrono::duration<double>(t1 - t0).count();
    t0 = t1;
    return s;
  }
};

// OptionsDescription (reference src/utils/options_description.cpp:33-96): long options take their
// value as the next argument (or --name=value), bool options take none, unknown options are errors.
struct Options {
  struct Opt {
    std::string long_name, short_name;
    bool is_flag;
    std::string value;
    bool seen = false;
  };
  std::vector<Opt> opts;
  void add(const char *l, const char *s, bool flag, const char *def) { opts.push_back({l, s, flag, def}); }
  void parse(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
      std::string a = argv[i], name, val;
      bool has_val = false;
      Opt *o = nullptr;
      if (a.rfind("--", 0) == 0) {
        size_t eq = a.find('=');
        name = a.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
        if (eq != std::string::npos) { val = a.substr(eq + 1); has_val = true; }
        for (auto &x : opts) if (x.long_name == name) o = &x;
      } else if (a.size() >= 2 && a[0] == '-') {
        name = a.substr(1, 1);
        if (a.size() > 2) { val = a.substr(2); has_val = true; }
        for (auto &x : opts) if (!x.short_name.empty() && x.short_name == name) o = &x;
      } else {
        continue;  // positional arguments are ignored, as getopt_long permutes them away
      }
      if (!o) throw std::string("Invalid option ") + a;
      o->seen = true;
      if (o->is_flag) { o->value = "1"; continue; }
      if (!has_val) {
        if (i + 1 >= argc) throw std::string("Option ") + a + " requires an argument";
        val = argv[++i];
      }
      o->value = val;
    }
  }
  const std::string &get(const char *l) const {
    for (auto &x : opts) if (x.long_name == l) return x.value;
    static std::string empty;
    return empty;
  }
  void usage() const {
    for (auto &x : opts)
      fprintf(stderr, "  %s--%s %s\n", x.short_name.empty() ? "" : ("-" + x.short_name + ", ").c_str(), x.long_name.c_str(),
              x.is_flag ? "" : "<arg>");
  }
};

int num_threads_or_all(int n) {
  if (n > 0) return n;
  unsigned hc = std::thread::hardware_concurrency();
  return hc ? (int)hc : 1;
}

// `mhx_core --serve <socket>`: this process stays, holds one handle and its device buffers, and runs the sub-programs that
// clients (mhx_core started with MHX_SERVER=<socket>) send it, one after the other — see serve() below.
bool g_serving = false;
mhx_ctx *g_served_ctx = nullptr;
// leave a sub-program early (usage errors): the process, or only the request when serving
[[noreturn]] void quit(int status) {
  if (g_serving) throw mhxio::Fatal{};
  exit(status);
}

mhx_ctx *open_gpu() {
  int dev = 0;
  if (const char *e = getenv("MHX_DEVICE")) dev = atoi(e);
  mhx_ctx *c = nullptr;
  if (g_serving && g_served_ctx) {
    c = g_served_ctx;
    if (mhx_reset(c) != 0) fatal("%s", mhx_last_error());
  } else {
    c = mhx_create(dev);
    if (!c) fatal("%s", mhx_last_error());
    if (g_serving) g_served_ctx = c;
  }
  mhx_profile_enable(c, getenv("MHX_PROFILE") ? 1 : 0);  // per-kernel HIP-event times, printed by finish()
  return c;
}
// The chained-scan sort gives up (and says so) when a unit waits seconds for a predecessor — a wedged or heavily shared
// GPU.  Its remedy is the classic histogram + scan + scatter passes (MHX_SORT=classic: slower, no inter-workgroup waiting).
// The worker process tells the front process (main) to start the sub-program again that way instead of failing the caller.
extern int g_done_fd;
constexpr unsigned char kRetryClassicSort = 75;
struct RetryClassic {};  // served request: run it once more with the classic sort passes
[[noreturn]] void fail_call(const char *msg) {
  if (g_serving) {
    if (!getenv("MHX_SORT") && strstr(msg, "chained scan timed out")) {
      mhxio::info("%s: running the request again with MHX_SORT=classic", msg);
      throw RetryClassic{};
    }
    fprintf(stderr, "FATAL %s\n", msg);
    throw mhxio::Fatal{};
  }
  if (g_done_fd >= 0 && !getenv("MHX_SORT") && strstr(msg, "chained scan timed out")) {
    mhxio::info("%s: running the sub-program again with MHX_SORT=classic", msg);
    fflush(nullptr);
    const unsigned char st = kRetryClassicSort;
    if (write(g_done_fd, &st, 1) == 1) _exit(kRetryClassicSort);
  }
  // (not exit(): with rank threads still running, static destructors and the HIP runtime's atexit handlers can hang)
  fprintf(stderr, "FATAL %s\n", msg);
  fflush(nullptr);
  _exit(1);
}
#define CK(call)                                  \
  do {                                            \
    if ((call) != 0) fail_call(mhx_last_error()); \
  } while (0)

// ---- multi-GPU: `mhx_core --gpus N <sub-program> ...` or MHX_NUM_GPUS=N.  One host thread per GPU in this process (no
// launcher): reads are sharded contiguously over the ranks, lv1 buckets over their owners, the items cross the node
// through the communicator of include/mhx.h (RCCL over xGMI; the in-process transport when ranks share a device, i.e.
// MHX_GPU_MAP="0,0" on a 1-GPU box) — what base_engine.cpp:213-223,318-327 does with OpenMP threads.
int g_num_gpus = 1;
struct RankSet {
  int n = 1;
  std::vector<int> dev;
  bool local = false;
};
RankSet rank_set() {
  RankSet rs;
  rs.n = g_num_gpus;
  if (const char *e = getenv("MHX_GPU_MAP")) {
    for (const char *p = e; *p;) {
      rs.dev.push_back(atoi(p));
      while (*p && *p != ',') ++p;
      if (*p == ',') ++p;
    }
  }
  for (int r = (int)rs.dev.size(); r < rs.n; ++r) rs.dev.push_back(r);
  rs.dev.resize(rs.n);
  for (int a = 0; a < rs.n; ++a)
    for (int b = a + 1; b < rs.n; ++b)
      if (rs.dev[a] == rs.dev[b]) rs.local = true;  // RCCL refuses two ranks on one device
  if (const char *e = getenv("MHX_COMM")) rs.local = !strcmp(e, "local");
  return rs;
}
// body(rank, ctx, comm) on one thread per rank; any failure ends the process with the rank's message
template <class Body>
void run_ranks(const RankSet &rs, Body body) {
  std::vector<mhx_ctx *> ctx(rs.n, nullptr);
  for (int r = 0; r < rs.n; ++r) {
    ctx[r] = mhx_create(rs.dev[r]);
    if (!ctx[r]) fatal("rank %d (device %d): %s", r, rs.dev[r], mhx_last_error());
    mhx_profile_enable(ctx[r], getenv("MHX_PROFILE") ? 1 : 0);
  }
  std::vector<mhx_comm *> comm(rs.n, nullptr);
  unsigned char id[MHX_COMM_ID_BYTES];
  if (rs.local) {
    if (mhx_comm_local_group(rs.n, ctx.data(), comm.data()) != 0) fatal("%s", mhx_last_error());
  } else if (mhx_comm_unique_id(id) != 0) {
    fatal("%s", mhx_last_error());
  }
  info("%d ranks on devices %s over %s", rs.n, [&] { std::string d; for (int v : rs.dev) d += std::to_string(v) + " "; return d; }().c_str(),
       rs.local ? "the in-process transport" : "RCCL");
  // A rank that fails must take the whole process down at once, from its own thread: the other ranks sit in a barrier of
  // the in-process transport or in an RCCL collective that this rank will never enter, so joining them would hang.
  // fail_rank -> fail_call: tells the front process (classic-sort retry or failure) and leaves with _exit, no teardown.
  auto fail_rank = [](int r, const std::string &what) {
    static std::mutex once;
    std::lock_guard<std::mutex> lk(once);  // the first failing rank reports; a second one waits here until the process is gone
    fail_call(("rank " + std::to_string(r) + ": " + (what.empty() ? "failed" : what)).c_str());
  };
  std::vector<std::thread> th;
  for (int r = 0; r < rs.n; ++r)
    th.emplace_back([&, r] {
      try {
        if (getenv("MHX_TEST_RANK_FAIL") && atoi(getenv("MHX_TEST_RANK_FAIL")) == r) throw std::string("test hook: this rank fails before its first collective");
        if (!rs.local) {
          comm[r] = mhx_comm_init_rank(ctx[r], id, r, rs.n);  // collective: returns when every rank has joined
          if (!comm[r]) throw std::string(mhx_last_error());
        }
        body(r, ctx[r], comm[r]);
      } catch (const std::string &e) {
        fail_rank(r, e);
      } catch (const std::exception &e) {  // std::bad_alloc from a fetch, std::system_error, ...
        fail_rank(r, e.what());
      } catch (...) {
        fail_rank(r, "unknown exception");
      }
    });
  for (auto &t : th) t.join();
  if (getenv("MHX_PROFILE")) {  // per-kernel HIP-event times of every rank (the ranks run side by side: the job's time per kernel is the slowest rank's)
    std::map<std::string, mhx_kernel_stat> worst;
    std::vector<std::vector<mhx_kernel_stat>> per_rank(rs.n);
    for (int r = 0; r < rs.n; ++r) {
      std::vector<mhx_kernel_stat> ks(64);
      const int n = mhx_profile_get(ctx[r], ks.data(), (int)ks.size());
      ks.resize(n < 0 ? 0 : std::min<size_t>((size_t)n, ks.size()));
      for (const mhx_kernel_stat &k : ks) {
        auto it = worst.find(k.name);
        if (it == worst.end() || k.total_ms > it->second.total_ms) worst[k.name] = k;
      }
      per_rank[r] = ks;
    }
    std::vector<mhx_kernel_stat> ws;
    for (auto &kv : worst) ws.push_back(kv.second);
    std::sort(ws.begin(), ws.end(), [](const mhx_kernel_stat &a, const mhx_kernel_stat &b) { return a.total_ms > b.total_ms; });
    for (const mhx_kernel_stat &k : ws) info("profile %-24s %6u launches %12.3f ms %14.0f algorithmic bytes (slowest of %d ranks)", k.name, k.launches, k.total_ms, k.algo_bytes, rs.n);
    if (const char *path = getenv("MHX_PROFILE_JSON")) {
      if (FILE *f = fopen(path, "w")) {
        auto put = [&](const std::vector<mhx_kernel_stat> &ks) {
          fprintf(f, "{");
          for (size_t i = 0; i < ks.size(); ++i)
            fprintf(f, "%s\"%s\": {\"launches\": %u, \"ms\": %.4f, \"bytes\": %.0f}", i ? ", " : "", ks[i].name, ks[i].launches, ks[i].total_ms, ks[i].algo_bytes);
          fprintf(f, "}");
        };
        fprintf(f, "{\"kernels\": ");
        put(ws);
        fprintf(f, ", \"what\": \"per kernel the slowest of %d ranks\", \"ranks\": [", rs.n);
        for (int r = 0; r < rs.n; ++r) {
          if (r) fprintf(f, ", ");
          put(per_rank[r]);
        }
        fprintf(f, "]}\n");
        fclose(f);
      }
    }
  }
  for (int r = 0; r < rs.n; ++r) {
    mhx_comm_destroy(comm[r]);
    mhx_destroy(ctx[r]);
  }
}
#define CKT(call)                                             \
  do {                                                        \
    if ((call) != 0) throw std::string(mhx_last_error());     \
  } while (0)
// contiguous shards of the reads with about equal numbers of record words
std::vector<uint64_t> shard_reads(const mhxio::BinFile &bin, int n) {
  std::vector<uint64_t> first(n + 1, bin.n_reads);
  first[0] = 0;
  for (int r = 1; r < n; ++r) {
    const uint64_t target = bin.n_words / n * r;
    if (bin.fixed_rw) first[r] = std::min<uint64_t>(bin.n_reads, (target + bin.fixed_rw - 1) / bin.fixed_rw);
    else first[r] = std::lower_bound(bin.off.begin(), bin.off.end(), target) - bin.off.begin();
  }
  return first;
}

// The outputs are on disk and closed: release the device memory and leave without running the HIP runtime's own teardown.
int g_done_fd = -1;  // write end of the pipe to the front process (main): set in the process that does the work
// test hook (tests/test_front_process.py): the first worker pretends the chained scan timed out
void maybe_pretend_scan_timeout() {
  if (getenv("MHX_TEST_SCAN_TIMEOUT_ONCE") && !getenv("MHX_SORT")) fail_call("radix sort: chained scan timed out waiting for a predecessor unit (test hook)");
}
std::atomic<uint64_t> g_d2h_ns{0}, g_d2h_bytes{0};  // (D2hClock, below)
int finish(mhx_ctx *c) {
  if (getenv("MHX_PROFILE")) {
    std::vector<mhx_kernel_stat> ks(256);
    const int n = mhx_profile_get(c, ks.data(), (int)ks.size());
    ks.resize(n < 0 ? 0 : std::min<size_t>((size_t)n, ks.size()));
    std::sort(ks.begin(), ks.end(), [](const mhx_kernel_stat &a, const mhx_kernel_stat &b) { return a.total_ms > b.total_ms; });
    for (const mhx_kernel_stat &s : ks) info("profile %-24s %6u launches %12.3f ms %14.0f algorithmic bytes", s.name, s.launches, s.total_ms, s.algo_bytes);
    if (const char *path = getenv("MHX_PROFILE_JSON")) {  // the same, machine-readable (tools/config_bench.py)
      if (FILE *f = fopen(path, "w")) {
        fprintf(f, "{\"kernels\": {");
        for (size_t i = 0; i < ks.size(); ++i)
          fprintf(f, "%s\"%s\": {\"launches\": %u, \"ms\": %.4f, \"bytes\": %.0f}", i ? ", " : "", ks[i].name, ks[i].launches, ks[i].total_ms, ks[i].algo_bytes);
        fprintf(f, "}}\n");
        fclose(f);
      }
    }
  }
  // Default: give the device memory back HERE, synchronously (hipFree of every buffer), before the caller is told that we
  // are done.  Leaving it to process exit is faster for this call (MHX_EARLY_EXIT=1: the front process returns while the
  // driver still reclaims tens of GB in the background) but the next GPU process of a pipeline then starts on a device
  // that is busy unmapping: its hipMalloc calls wait and hipMemGetInfo under-reports (the reference's orchestrator runs
  // count -> seq2sdbg -> assemble -> iterate -> seq2sdbg back to back).
  if (!g_serving && (!getenv("MHX_EARLY_EXIT") || getenv("MHX_CLEAN_EXIT"))) mhx_destroy(c);
  {
    double ms = 0, fs = 0;
    uint64_t bytes = 0, calls = 0;
    mhx_alloc_stats(&ms, &fs, &bytes, &calls);
    info("Device memory: %llu allocations, %.2f GB, %.4f s in hipMalloc, %.4f s in hipFree%s", (unsigned long long)calls, (double)bytes / 1e9, ms, fs,
         g_serving ? " (server: totals since its start, buffers kept)" : "");
    info("Device to host: %.2f GB in %.4f s%s", (double)g_d2h_bytes.load() / 1e9, (double)g_d2h_ns.load() * 1e-9, g_serving ? " (server: totals since its start)" : "");
  }
  if (g_serving) {  // the handle and its buffers stay for the next request
    fflush(nullptr);
    return 0;
  }
  fflush(nullptr);
  if (g_done_fd >= 0) {
    // Everything the caller waits for exists and is closed: tell the front process.  The standard streams are closed so
    // that a caller reading our stderr through a pipe sees its end when the front process exits.
    const unsigned char ok = 0;
    if (write(g_done_fd, &ok, 1) != 1) _exit(1);
    close(g_done_fd);
    close(0);
    close(1);
    close(2);
  }
  _exit(0);
}

// what leaves the device for the output files: seconds and bytes, reported with the memory line (where the wall time of a large job goes
// besides its kernels: VERDICT r5 weak #5)
struct D2hClock {
  uint64_t bytes;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit D2hClock(uint64_t b) : bytes(b) {}
  ~D2hClock() {
    g_d2h_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    g_d2h_bytes += bytes;
  }
};
template <class T>
std::vector<T> fetch_t(mhx_ctx *c, int which) {  // the throwing flavour for rank threads
  uint64_t bytes = mhx_buffer_bytes(c, which);
  D2hClock clk(bytes);
  std::vector<T> v(bytes / sizeof(T));
  if (bytes) CKT(mhx_fetch(c, which, v.data(), 0, bytes));
  return v;
}

template <class T>
std::vector<T> fetch(mhx_ctx *c, int which) {
  uint64_t bytes = mhx_buffer_bytes(c, which);
  D2hClock clk(bytes);
  std::vector<T> v(bytes / sizeof(T));
  if (bytes) CK(mhx_fetch(c, which, v.data(), 0, bytes));
  return v;
}

int out_files(int n_threads) {
  if (const char *e = getenv("MHX_NUM_OUT_FILES")) return std::max(1, std::min(atoi(e), n_threads));
  return 1;
}

// ---- memory plan (the reference's --host_mem / lv1 passes, base_engine.cpp:54-141): when the items of a stage do not
// fit the free HBM (or MHX_MAX_ITEMS caps them), the stage runs once per contiguous range of lv1 buckets.
struct BucketRange {
  uint32_t lo, hi;
  uint64_t n_items;
};
// What a planned stage held on the device (mhx_alloc_peak): the bytes held when its plan was made, the peak until its last pass was
// done, and the free bytes the plan was made with — the budget the plan is held to (tests/test_gpu_memory_plan.py).
struct PlanMemory {
  uint64_t held = 0;
  double budget = 0;
} g_plan_memory;
void note_plan_memory(double free_bytes) {
  mhx_alloc_peak(&g_plan_memory.held, nullptr, 1);
  g_plan_memory.budget = free_bytes;
}
// The staging of a stage that extracts over batches of reads (the lv1 histogram of such a stage, and its filtered passes: one batch of
// items and its keep/drop split) is sized by the budget too: a 32nd of the free bytes each, 1 GiB at the most — 1/15 of the free bytes
// with the allocator's headroom, out of the fifth the plan leaves free.
uint64_t plan_batch_bytes() { return (uint64_t)std::min(std::max(g_plan_memory.budget / 32.0, 1048576.0), 1073741824.0); }
const char *stage_name(int stage) {
  switch (stage) {
    case MHX_STAGE_S1: return "stage 1";
    case MHX_STAGE_S1_MERCY: return "stage 1 (mercy)";
    case MHX_STAGE_S2: return "stage 2";
    case MHX_STAGE_COUNT: return "count";
    case MHX_STAGE_SEQ2SDBG: return "seq2sdbg";
  }
  return "stage";
}
void report_plan_memory(int stage) {
  uint64_t peak = 0;
  mhx_alloc_peak(nullptr, &peak, 0);
  info("Device memory of %s: %llu bytes held when planned, peak %llu bytes, budget %.0f", stage_name(stage), (unsigned long long)g_plan_memory.held,
       (unsigned long long)peak, g_plan_memory.budget);
}
// the same for the stages of a rank driver call (mhx_dist_plan_memory: the ranks of this process together)
void report_rank_memory(mhx_comm *cm) {
  int stage = 0;
  uint64_t held = 0, peak = 0, budget = 0;
  const int n = mhx_dist_plan_memory(cm, -1, nullptr, nullptr, nullptr, nullptr, 0);
  for (int i = 0; i < n; ++i) {
    mhx_dist_plan_memory(cm, i, &stage, &held, &peak, &budget, i + 1 == n);
    info("Device memory of %s: %llu bytes held when planned, peak %llu bytes, budget %llu", stage_name(stage), (unsigned long long)held,
         (unsigned long long)peak, (unsigned long long)budget);
  }
}
// Plan by TIME as well as by space: -> the passes P that minimise P * t_scan + working_set / P * rate (0: by space alone), logged.
// (see plan_ranges; MHX_PLAN_BY_TIME=0 switches it off, MHX_ALLOC_S_PER_GB sets the rate: tests)
int plan_passes_by_time(mhx_ctx *c, double working_set) {
  if (getenv("MHX_PLAN_BY_TIME") && atoi(getenv("MHX_PLAN_BY_TIME")) == 0) return 0;
  double malloc_s = 0;
  uint64_t abytes = 0;
  mhx_alloc_stats(&malloc_s, nullptr, &abytes, nullptr);
  // (seconds per byte.  The first few GB of a process come fast whatever the box — at 100 M reads the 4.6 GB of the read store
  //  took 0.1 s, the 239 GB behind them 6.1 s — so what has been seen so far is only a lower bound: a working set of more than
  //  64 GB is planned with at least 5 ms per GB — the boxes of this pool showed 0.03 (one box), 2-4, 17 and 25 ms per GB for the
  //  same 239 GB: a plan for 5 costs a fast box 0.25 s of extra read scans and saves a slow one 2-3 s.  A resident server keeps
  //  its buffers between requests: nothing to plan for there.)
  double rate = abytes >= (1ull << 30) ? malloc_s / (double)abytes : 0.0;
  if (working_set > 64e9 && !g_serving) rate = std::max(rate, 5e-12);
  if (g_serving) rate = 0;
  if (const char *e = getenv("MHX_ALLOC_S_PER_GB")) rate = atof(e) * 1e-9;
  const double t_scan = 6.5e-12 * (double)mhx_num_bases(c);
  if (!(rate > 0 && t_scan > 0)) return 0;
  const int p = (int)std::min(16.0, std::floor(std::sqrt(working_set * rate / t_scan) + 0.5));
  if (p < 2) return 0;
  info("Memory plan by time: hipMalloc ran at %.1f ms per GB so far; %d passes of ~%.1f GB each instead of one working set of %.1f GB", rate * 1e12, p,
       working_set / p / 1e9, working_set / 1e9);
  return p;
}
// Stage 2 from a count of the (k+1)-mers whose one run does not fit: its count in passes over the count's OWN lv1 bucket ranges (include/mhx.h:
// s2_count_pass_items, mhx_s2_from_count_bytes) — the largest pass whose figure, with the allocator's headroom, fits `avail`, fewer records
// where the plan by time says so.  At the 40 M-read shard under a budget that fails the once-fit by one per cent: 558 ms of kernels in 4 count
// passes against 890 ms for the per-occurrence lv1 passes (profiles/r18_s2_count_passes.json).  MHX_S2_COUNT_PASSES=0 switches it off.
// -> the passes planned, with the options set and s2_agg_from_count = 3 (a give-up fails the call); 0: not planned, nothing set
struct S2CountPlan {
  bool allowed = true;  // in: false once the route gave this job up
  size_t passes = 0;    // out: the count passes planned, 0: the lv1 plan stands
};
size_t plan_s2_count_passes(mhx_ctx *c, uint32_t k, uint32_t m, double est_items, double avail) {
  const char *sw = getenv("MHX_S2_COUNT_PASSES");
  if (sw && atoi(sw) == 0) return 0;
  const double headroom = 17.0 / 16.0;
  const uint64_t est = (uint64_t)est_items;
  if (!mhx_s2_from_count_bytes(c, k, m, est, 1) || (double)mhx_s2_from_count_bytes(c, k, m, est, 1) * headroom > avail) return 0;
  std::vector<uint64_t> hist(MHX_NUM_BUCKETS);
  CK(mhx_set_bucket_filter(c, nullptr, 0, plan_batch_bytes(), 0));  // (no filter: the batch size alone, for a histogram taken over batches)
  CK(mhx_bucket_histogram(c, MHX_STAGE_COUNT, k, m, hist.data()));
  uint64_t records = 0;
  for (uint64_t v : hist) records += v;
  if (!records) return 0;
  uint64_t lo = 1, hi = records;  // the largest pass that fits (the figure grows with the pass)
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if ((double)mhx_s2_from_count_bytes(c, k, m, est, mid) * headroom <= avail) lo = mid;
    else hi = mid - 1;
  }
  uint64_t pass = lo;
  const double working_set = (double)mhx_s2_from_count_bytes(c, k, m, est, records) - (double)mhx_s2_from_count_bytes(c, k, m, est, 1);
  if (const int p = plan_passes_by_time(c, working_set)) pass = std::min<uint64_t>(pass, (uint64_t)((double)records / p * 1.02));
  pass = std::max<uint64_t>(pass, 1);
  size_t n_passes = 1;  // as the library cuts them (s2.hip s2_count_ranges)
  uint64_t acc = 0;
  for (uint64_t v : hist) {
    if (acc && acc + v > pass) {
      ++n_passes;
      acc = 0;
    }
    acc += v;
  }
  if (n_passes < 2 || n_passes > 64) return 0;  // (more than the library's cap: it would decline)
  CK(mhx_set_option(c, "s2_count_pass_items", (long long)pass));
  CK(mhx_set_option(c, "s2_count_budget_mb", (long long)std::max(1.0, std::floor(avail / 1048576.0))));
  CK(mhx_set_option(c, "s2_agg_from_count", 3));
  info("Memory plan: stage 2 from a count in %zu passes over its own bucket ranges (at most %llu records each)", n_passes, (unsigned long long)pass);
  return n_passes;
}
// fixed_bytes: device state of the stage that does not shrink with the bucket range (stage 1: the 1 B/base mark map, the
// bitmap and the aggregated stage-2 items; count: first_0_out / last_0_in; all: sort status words ~ items / 3)
std::vector<BucketRange> plan_ranges(mhx_ctx *c, int stage, uint32_t k, uint32_t m, size_t item_bytes, double items_upper_bound,
                                     double fixed_bytes = 0, S2CountPlan *s2_count = nullptr) {
  uint64_t max_items = 0;
  double free_bytes = (double)mhx_device_free_bytes(c);
  if (const char *e = getenv("MHX_FREE_BYTES")) free_bytes = atof(e);  // tests: make the automatic plan fire on a small input
  note_plan_memory(free_bytes);
  if (const char *e = getenv("MHX_MAX_ITEMS")) max_items = strtoull(e, nullptr, 10);
  else {
    // What the figures leave out is taken off here: the part of the library's figure that does not grow with the items (status words
    // over all item slots, the giant buckets' tables: its answer for no items), the staging of the batched extraction (one batch of items
    // and its split) and the allocator's headroom (DevBuf::reserve: bytes + bytes / 16) on both and on every item buffer below.
    const double lib_fixed = (double)mhx_stage_pass_bytes(c, stage, k, m, 0);
    const double headroom = 17.0 / 16.0;
    if (free_bytes * 0.8 - fixed_bytes <= 0)
      fatal("not enough free device memory for the fixed state of this stage (%.1f GB free, %.1f GB needed)", free_bytes / 1e9, fixed_bytes / 1e9);
    double avail = free_bytes * 0.8 - fixed_bytes - (lib_fixed + 2.0 * (double)plan_batch_bytes()) * headroom;
    // (tables of a fixed size — tens of MB — against a free memory of a few MB, as the tests fake it: the passes are planned with a
    //  twelfth of it, and the stage will hold more than was free)
    if (avail < free_bytes / 12.0) {
      info("WARNING: the workspaces of a fixed size of this stage (%.0f MB) leave less than a twelfth of the free device memory (%.0f MB) for its items: planning with that twelfth",
           lib_fixed * headroom / 1e6, free_bytes / 1e6);
      avail = free_bytes / 12.0;
    }
    // A route that serves only the whole job at once decides only whether one run fits: a plan of several passes sets the bucket
    // filter, which switches such a route off, so its ranges are sized with the figure of a filtered pass below.
    const uint64_t once_bytes = mhx_stage_once_bytes(c, stage, k, m, (uint64_t)items_upper_bound);
    if (once_bytes && (double)once_bytes * headroom <= avail) return {{0, MHX_NUM_BUCKETS, 0}};
    // ... unless that route cuts its own count into passes: then the single unfiltered range again
    if (once_bytes && stage == MHX_STAGE_S2 && s2_count && s2_count->allowed) {
      s2_count->passes = plan_s2_count_passes(c, k, m, items_upper_bound, avail);
      if (s2_count->passes) return {{0, MHX_NUM_BUCKETS, 0}};
    }
    // 2 sort buffers + filtered copy (+ status words); the library knows better where a stage has a leaner path
    const uint64_t probe = 1ull << 30, lib_bytes = mhx_stage_pass_bytes(c, stage, k, m, probe);
    const double per_item = headroom * (lib_bytes ? ((double)lib_bytes - lib_fixed) / (double)probe : 3.0 * (double)item_bytes + 1.0);
    const double fit = avail / per_item;
    // Plan by TIME as well as by space (round 6).  On this driver hipMalloc costs per BYTE mapped, not per call (tools/micro/alloc_probe:
    // 200 GB in one call 3.4 s, in 40 calls 4.4 s; between 3 and 30 ms per GB from box to box and process to process), while one more
    // bucket-range pass costs one more scan of the reads by the histogram pre-pass and the generating pass (~6.5 ps per base: 0.1 s at
    // 100 M reads) where the stage has that lean form (lib_bytes: the library says so).  The rate this very process has seen so far —
    // the read store it has just allocated — decides: P passes minimise P * t_scan + bytes(P) * rate.  MHX_PLAN_BY_TIME=0 switches it off.
    double time_cap = 0;
    if (lib_bytes && (stage == MHX_STAGE_S1 || stage == MHX_STAGE_COUNT))
      if (const int p = plan_passes_by_time(c, per_item * items_upper_bound)) time_cap = items_upper_bound / p * 1.02;
    if (items_upper_bound <= fit && time_cap == 0) return {{0, MHX_NUM_BUCKETS, 0}};
    max_items = (uint64_t)(time_cap > 0 ? std::min(fit, time_cap) : fit);
  }
  if (!max_items) return {{0, MHX_NUM_BUCKETS, 0}};
  std::vector<uint64_t> hist(MHX_NUM_BUCKETS);
  CK(mhx_set_bucket_filter(c, nullptr, 0, plan_batch_bytes(), 0));  // (no filter: the batch size alone)
  CK(mhx_bucket_histogram(c, stage, k, m, hist.data()));
  std::vector<BucketRange> out;
  uint32_t lo = 0;
  uint64_t acc = 0;
  for (uint32_t b = 0; b < MHX_NUM_BUCKETS; ++b) {
    if (acc && acc + hist[b] > max_items) {
      out.push_back({lo, b, acc});
      lo = b;
      acc = 0;
    }
    acc += hist[b];
  }
  out.push_back({lo, MHX_NUM_BUCKETS, acc});
  for (const BucketRange &r : out)
    if (r.hi - r.lo == 1 && r.n_items > max_items)  // the reference gives up here (base_engine.cpp:96-99); we try, the allocation may fail
      info("WARNING: lv1 bucket %u alone holds %llu items, more than the %llu that fit: trying it as a pass of its own", r.lo,
           (unsigned long long)r.n_items, (unsigned long long)max_items);
  if (out.size() > 1) info("Memory plan: %zu passes over lv1 bucket ranges (at most %llu items each)", out.size(), (unsigned long long)max_items);
  return out;
}
void set_range(mhx_ctx *c, const std::vector<BucketRange> &ranges, size_t i, bool accumulate) {
  if (ranges.size() == 1) return;  // everything at once: no filter
  std::vector<uint8_t> keep(MHX_NUM_BUCKETS, 0);
  for (uint32_t b = ranges[i].lo; b < ranges[i].hi; ++b) keep[b] = 1;
  CK(mhx_set_bucket_filter(c, keep.data(), ranges[i].n_items, plan_batch_bytes(), accumulate && i > 0 ? 1 : 0));
}
void clear_range(mhx_ctx *c, const std::vector<BucketRange> &ranges) {
  if (ranges.size() > 1) CK(mhx_set_bucket_filter(c, nullptr, 0, 0, 0));
}

// SdBG output collected over the passes (bucket order = pass order)
struct SdbgAcc {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> off = std::vector<uint64_t>(MHX_NUM_BUCKETS, 0), items = off, tips = off, large = off;
  uint64_t wc[10] = {0};
  mhx_sdbg_result r{};
  void add(mhx_ctx *c, const mhx_sdbg_result &pr) {
    add(fetch<uint8_t>(c, MHX_BUF_SDBG_BYTES), fetch<uint64_t>(c, MHX_BUF_BUCKET_OFFSET), fetch<uint64_t>(c, MHX_BUF_BUCKET_COUNT),
        fetch<uint64_t>(c, MHX_BUF_BUCKET_TIPS), fetch<uint64_t>(c, MHX_BUF_BUCKET_LARGE), fetch<uint64_t>(c, MHX_BUF_W_COUNT), pr);
  }
  void add(const SdbgAcc &o) { add(o.bytes, o.off, o.items, o.tips, o.large, std::vector<uint64_t>(o.wc, o.wc + 10), o.r); }
  void add(std::vector<uint8_t> b, const std::vector<uint64_t> &o, const std::vector<uint64_t> &it, const std::vector<uint64_t> &tp,
           const std::vector<uint64_t> &lg, const std::vector<uint64_t> &w, const mhx_sdbg_result &pr) {
    for (int i = 0; i < MHX_NUM_BUCKETS; ++i) {
      if (it[i]) off[i] = o[i] + bytes.size();
      items[i] += it[i];
      tips[i] += tp[i];
      large[i] += lg[i];
    }
    for (int i = 0; i < 10; ++i) wc[i] += w[i];
    if (bytes.empty()) bytes = std::move(b);  // the usual single pass: no second copy of the byte stream
    else bytes.insert(bytes.end(), b.begin(), b.end());
    r.n_items += pr.n_items;
    r.n_sdbg += pr.n_sdbg;
    r.n_tips += pr.n_tips;
    r.n_large += pr.n_large;
    r.sdbg_bytes += pr.sdbg_bytes;
    r.words_per_tip_label = pr.words_per_tip_label;
    r.item_words = pr.item_words;
  }
  void write(const std::string &out, uint32_t k, int n_files) const {
    mhxio::write_sdbg(out, k, r.words_per_tip_label, bytes.data(), bytes.size(), off.data(), items.data(), tips.data(), large.data(), n_files);
    info("Number of $ A C G T A- C- G- T-:");
    fprintf(stderr, "INFO  ");
    for (int i = 0; i < 9; ++i) fprintf(stderr, "%llu ", (unsigned long long)wc[i]);
    fprintf(stderr, "\n");
    info("Total number of edges: %llu", (unsigned long long)r.n_sdbg);
    info("Total number of ONEs: %llu", (unsigned long long)wc[9]);
    info("Total number of $v edges: %llu", (unsigned long long)r.n_tips);
  }
};

// The read library's record stream, mapped (no host copy), loaded into the GPU store reversed (kmer_counter.cpp:61).
// When every read has the same length — the first record's size divides the stream and the device finds that length in
// every record header — no per-read table is ever built on the host.
mhxio::BinFile load_read_lib(mhx_ctx *c, const std::string &prefix) {
  int64_t bases, reads;
  mhxio::read_lib_info(prefix, &bases, &reads);
  mhxio::BinFile bin = mhxio::open_bin_file(prefix + ".bin");
  if (bin.fixed_rw) {
    CK(mhx_load_bin_records(c, bin.data, bin.n_words, bin.n_reads, 1));
    if (bin.n_reads && mhx_fixed_length(c) != bin.data[0]) {  // lengths differ after all: index the records and load again
      bin.build_index();
      CK(mhx_load_bin_records(c, bin.data, bin.n_words, bin.n_reads, 1));
    }
  } else {
    CK(mhx_load_bin_records(c, bin.data, bin.n_words, bin.n_reads, 1));
  }
  if ((int64_t)bin.n_reads != reads) info("lib_info says %lld reads, .bin holds %llu", (long long)reads, (unsigned long long)bin.n_reads);
  return bin;
}
// the multi-GPU paths shard the records on the host: they need the true record offsets
mhxio::BinFile open_indexed(const std::string &prefix) {
  mhxio::BinFile bin = mhxio::open_bin_file(prefix + ".bin");
  if (bin.fixed_rw) {  // confirm the arithmetic index on the host (one header word per record)
    const uint32_t L = bin.data[0];
    bool ok = true;
    for (uint64_t i = 0; i < bin.n_reads && ok; ++i) ok = bin.data[i * bin.fixed_rw] == L;
    if (!ok) bin.build_index();
  }
  return bin;
}

// ---------------------------------------------------------------------------
int main_kmer_count(int argc, char **argv) {
  Options o;
  o.add("kmer_k", "k", false, "21");
  o.add("min_kmer_frequency", "m", false, "2");
  o.add("host_mem", "", false, "0");
  o.add("num_cpu_threads", "", false, "0");
  o.add("read_lib_file", "", false, "");
  o.add("output_prefix", "", false, "out");
  o.add("mem_flag", "", false, "1");
  try {
    o.parse(argc, argv);
    if (o.get("read_lib_file").empty()) throw std::string("No read library configuration file!");
    if (atof(o.get("host_mem").c_str()) == 0) throw std::string("Please specify the host memory!");
  } catch (std::string &e) {
    fprintf(stderr, "%s\nUsage: sdbg_builder count --input_file fastx_file -o out\nOptions:\n", e.c_str());
    o.usage();
    quit(1);
  }
  const uint32_t k = (uint32_t)atoi(o.get("kmer_k").c_str()), m = (uint32_t)atoi(o.get("min_kmer_frequency").c_str());
  const int n_threads = num_threads_or_all(atoi(o.get("num_cpu_threads").c_str()));
  const std::string out = o.get("output_prefix");
  Timer t;
  if (g_num_gpus > 1) {
    const RankSet rs = rank_set();
    info("Preparing data...");
    mhxio::BinFile lib = open_indexed(o.get("read_lib_file"));
    const std::vector<uint64_t> first = shard_reads(lib, rs.n);
    info("%llu reads; Preparing data... Done. Time elapsed: %.4f", (unsigned long long)lib.n_reads, t.lap());
    std::vector<std::vector<uint32_t>> edges(rs.n), f0(rs.n), l0(rs.n);
    std::vector<std::vector<uint64_t>> bc(rs.n);
    std::vector<std::vector<int64_t>> hist(rs.n);
    std::vector<mhx_count_result> res(rs.n);
    std::string plan_text;
    run_ranks(rs, [&](int r, mhx_ctx *c, mhx_comm *cm) {
      const uint64_t lo = first[r], hi = first[r + 1];
      const uint64_t w0 = lib.end_offset(lo), w1 = lib.end_offset(hi);
      CKT(mhx_load_bin_records(c, lib.data + w0, w1 - w0, hi - lo, 1));
      CKT(mhx_dist_setup(c, cm, MHX_STAGE_COUNT, k, m));
      CKT(mhx_dist_count(c, cm, k, m, &res[r]));
      if (r == 0) report_rank_memory(cm);
      if (r == 0) plan_text = mhx_last_s1_plan(c);
      edges[r] = fetch_t<uint32_t>(c, MHX_BUF_EDGES);
      bc[r] = fetch_t<uint64_t>(c, MHX_BUF_BUCKET_COUNT);
      hist[r] = fetch_t<int64_t>(c, MHX_BUF_MUL_HIST);
      f0[r] = fetch_t<uint32_t>(c, MHX_BUF_FIRST_0_OUT);
      l0[r] = fetch_t<uint32_t>(c, MHX_BUF_LAST_0_IN);
    });
    mhx_count_result r{};
    std::vector<uint32_t> all_edges, first_out, last_in;
    std::vector<uint64_t> bcount(MHX_NUM_BUCKETS, 0);
    std::vector<int64_t> h(MHX_MAX_MUL + 1, 0);
    for (int q = 0; q < rs.n; ++q) {  // ranks own ascending bucket ranges and hold ascending read ranges
      all_edges.insert(all_edges.end(), edges[q].begin(), edges[q].end());
      first_out.insert(first_out.end(), f0[q].begin(), f0[q].end());
      last_in.insert(last_in.end(), l0[q].begin(), l0[q].end());
      for (int b = 0; b < MHX_NUM_BUCKETS; ++b) bcount[b] += bc[q][b];
      for (int i = 0; i <= MHX_MAX_MUL; ++i) h[i] += hist[q][i];
      r.n_items += res[q].n_items;
      r.n_distinct += res[q].n_distinct;
      r.n_edges += res[q].n_edges;
      r.words_per_edge = res[q].words_per_edge;
    }
    info("GPU count: %llu items, %llu distinct, %llu solid. Time elapsed: %.4f", (unsigned long long)r.n_items,
         (unsigned long long)r.n_distinct, (unsigned long long)r.n_edges, t.lap());
    info("Count plan: %s", plan_text.c_str());
    mhxio::write_edges(out, k, r.words_per_edge, all_edges.data(), r.n_edges, bcount.data(), std::max(out_files(n_threads), std::min(rs.n, n_threads)));
    int64_t n_cand = 0, n_tips = 0;
    mhxio::write_cand(out, lib, first_out.data(), last_in.data(), &n_cand, &n_tips);
    mhxio::write_counting(out, h.data());
    info("Total number of candidate reads: %lld (%lld)", (long long)n_cand, (long long)n_tips);
    info("Total number of solid edges: %llu", (unsigned long long)r.n_edges);
    info("Postprocess done. Time elapsed: %.4f", t.lap());
    return 0;
  }
  mhx_ctx *c = open_gpu();
  info("Device ready. Time elapsed: %.4f", t.lap());
  info("Preparing data...");
  mhxio::BinFile lib = load_read_lib(c, o.get("read_lib_file"));
  info("%llu reads; Preparing data... Done. Time elapsed: %.4f", (unsigned long long)mhx_num_sequences(c), t.lap());
  const size_t count_item_bytes = (size_t)(((2 * (k + 1) + 31) / 32 + 2 + 1) / 2 * 2) * 4;
  // count on super-k-mer records plans its own passes (include/mhx.h: mhx_count_self_planned): asked first, unless the environment dictates
  // a plan; a job it gives up on fails the call and the lv1 bucket plan takes over
  std::vector<BucketRange> ranges;
  bool self_planned = false;
  const long long skm_before = mhx_get_option(c, "count_skm", 1);
  if (!getenv("MHX_MAX_ITEMS") && !getenv("MHX_FREE_BYTES") && mhx_count_self_planned(c, k, m) == 1) {
    self_planned = true;
    mhx_set_option(c, "count_skm", 3);
    ranges = {{0, MHX_NUM_BUCKETS, 0}};
    note_plan_memory((double)mhx_device_free_bytes(c));
  } else {
    ranges = plan_ranges(c, MHX_STAGE_COUNT, k, m, count_item_bytes, (double)mhx_num_bases(c), 12.0 * (double)mhx_num_sequences(c));
  }
  mhx_count_result r{};
  std::vector<uint32_t> edges;
  std::vector<uint64_t> bcount(MHX_NUM_BUCKETS, 0);
  for (size_t i = 0; i < ranges.size(); ++i) {
    set_range(c, ranges, i, true);
    mhx_count_result pr;
    if (self_planned) {
      const bool ok = mhx_count(c, k, m, &pr) == 0;
      mhx_set_option(c, "count_skm", ok ? skm_before : 0);
      self_planned = false;
      if (!ok) {  // (nothing taken yet: plan the lv1 bucket ranges and start over)
        info("count on super-k-mer records: %s; planning lv1 bucket ranges instead", mhx_last_error());
        ranges = plan_ranges(c, MHX_STAGE_COUNT, k, m, count_item_bytes, (double)mhx_num_bases(c), 12.0 * (double)mhx_num_sequences(c));
        i = (size_t)-1;
        continue;
      }
    } else {
      CK(mhx_count(c, k, m, &pr));
    }
    {  // this pass's solid edges straight behind the earlier passes' (no second host copy)
      const uint64_t eb = mhx_buffer_bytes(c, MHX_BUF_EDGES);
      const size_t at = edges.size();
      if (i == 0 && ranges.size() > 1) edges.reserve((size_t)(eb / 4) * ranges.size() * 5 / 4);
      D2hClock clk(eb);
      edges.resize(at + eb / 4);
      if (eb) CK(mhx_fetch(c, MHX_BUF_EDGES, edges.data() + at, 0, eb));
    }
    auto bc = fetch<uint64_t>(c, MHX_BUF_BUCKET_COUNT);
    for (int b = 0; b < MHX_NUM_BUCKETS; ++b) bcount[b] += bc[b];
    r.n_items += pr.n_items;
    r.n_distinct += pr.n_distinct;
    r.n_edges += pr.n_edges;
    r.words_per_edge = pr.words_per_edge;
  }
  clear_range(c, ranges);
  report_plan_memory(MHX_STAGE_COUNT);
  info("GPU count: %llu items, %llu distinct, %llu solid. Time elapsed: %.4f", (unsigned long long)r.n_items,
       (unsigned long long)r.n_distinct, (unsigned long long)r.n_edges, t.lap());
  info("Count plan: %s", mhx_last_s1_plan(c));
  auto first = fetch<uint32_t>(c, MHX_BUF_FIRST_0_OUT), last = fetch<uint32_t>(c, MHX_BUF_LAST_0_IN);
  auto hist = fetch<int64_t>(c, MHX_BUF_MUL_HIST);
  mhxio::write_edges(out, k, r.words_per_edge, edges.data(), r.n_edges, bcount.data(), out_files(n_threads));
  int64_t n_cand = 0, n_tips = 0;
  mhxio::write_cand(out, lib, first.data(), last.data(), &n_cand, &n_tips);
  mhxio::write_counting(out, hist.data());
  info("Total number of candidate reads: %lld (%lld)", (long long)n_cand, (long long)n_tips);
  info("Total number of solid edges: %llu", (unsigned long long)r.n_edges);
  info("Postprocess done. Time elapsed: %.4f", t.lap());
  return finish(c);
}

int main_read2sdbg(int argc, char **argv) {
  Options o;
  o.add("kmer_k", "k", false, "21");
  o.add("min_kmer_frequency", "m", false, "2");
  o.add("host_mem", "", false, "0");
  o.add("num_cpu_threads", "", false, "0");
  o.add("read_lib_file", "", false, "");
  o.add("output_prefix", "", false, "out");
  o.add("mem_flag", "", false, "1");
  o.add("need_mercy", "", true, "");
  try {
    o.parse(argc, argv);
    if (o.get("read_lib_file").empty()) throw std::string("No input file!");
    if (atof(o.get("host_mem").c_str()) == 0) throw std::string("Please specify the host memory!");
  } catch (std::string &e) {
    fprintf(stderr, "%s\nUsage: sdbg_builder read2sdbg --read_lib_file fastx_file -o out\nOptions:\n", e.c_str());
    o.usage();
    quit(1);
  }
  const uint32_t k = (uint32_t)atoi(o.get("kmer_k").c_str()), m = (uint32_t)atoi(o.get("min_kmer_frequency").c_str());
  const int n_threads = num_threads_or_all(atoi(o.get("num_cpu_threads").c_str()));
  const bool need_mercy = !o.get("need_mercy").empty();
  const std::string out = o.get("output_prefix");
  Timer t;
  if (g_num_gpus > 1) {
    const RankSet rs = rank_set();
    info("Preparing data...");
    mhxio::BinFile lib = open_indexed(o.get("read_lib_file"));
    const std::vector<uint64_t> first = shard_reads(lib, rs.n);
    info("%llu reads; Preparing data... Done. Time elapsed: %.4f", (unsigned long long)lib.n_reads, t.lap());
    const int mercy_mode = !need_mercy ? 0 : (getenv("MHX_STABLE_TIES") ? 1 : 2);
    std::vector<SdbgAcc> part(rs.n);
    std::vector<std::vector<int64_t>> hist(rs.n);
    std::vector<mhx_s1_result> r1(rs.n);
    std::vector<uint64_t> nm(rs.n, 0);
    std::string plan_text;
    run_ranks(rs, [&](int r, mhx_ctx *c, mhx_comm *cm) {
      const uint64_t lo = first[r], hi = first[r + 1];
      const uint64_t w0 = lib.end_offset(lo), w1 = lib.end_offset(hi);
      CKT(mhx_load_bin_records(c, lib.data + w0, w1 - w0, hi - lo, 1));
      CKT(mhx_dist_setup(c, cm, m > 1 ? (mercy_mode ? MHX_STAGE_S1_MERCY : MHX_STAGE_S1) : MHX_STAGE_S2, k, m));
      mhx_sdbg_result r2{};
      CKT(mhx_dist_read2sdbg(c, cm, k, m, mercy_mode, &r1[r], &r2, &nm[r]));
      if (r == 0) report_rank_memory(cm);
      if (m > 1) hist[r] = fetch_t<int64_t>(c, MHX_BUF_MUL_HIST);
      if (r == 0) plan_text = mhx_last_s1_plan(c);
      part[r].add(fetch_t<uint8_t>(c, MHX_BUF_SDBG_BYTES), fetch_t<uint64_t>(c, MHX_BUF_BUCKET_OFFSET), fetch_t<uint64_t>(c, MHX_BUF_BUCKET_COUNT),
                  fetch_t<uint64_t>(c, MHX_BUF_BUCKET_TIPS), fetch_t<uint64_t>(c, MHX_BUF_BUCKET_LARGE), fetch_t<uint64_t>(c, MHX_BUF_W_COUNT), r2);
    });
    if (m > 1) {
      std::vector<int64_t> h(MHX_MAX_MUL + 1, 0);
      uint64_t n1 = 0, ns = 0, mercy_total = 0;
      for (int q = 0; q < rs.n; ++q) {
        for (int i = 0; i <= MHX_MAX_MUL; ++i) h[i] += hist[q][i];
        n1 += r1[q].n_items;
        ns += r1[q].n_solid;
        mercy_total += nm[q];
      }
      int64_t n_solid_edges = 0;
      for (uint32_t i = m; i <= 65535; ++i) n_solid_edges += h[i];
      info("Total number of solid edges: %lld", (long long)n_solid_edges);
      mhxio::write_counting(out, h.data());
      info("Stage 1 done (%llu items, %llu solid occurrences).", (unsigned long long)n1, (unsigned long long)ns);
      info("Stage 1 plan: %s", plan_text.c_str());
      if (need_mercy) info("Number mercy: %llu", (unsigned long long)mercy_total);
    }
    SdbgAcc acc;
    for (int q = 0; q < rs.n; ++q) acc.add(part[q]);  // ranks own ascending bucket ranges: concatenation = bucket order
    info("Stage 2 done (%llu items). Time elapsed: %.4f", (unsigned long long)acc.r.n_items, t.lap());
    acc.write(out, k, std::max(out_files(n_threads), std::min(rs.n, n_threads)));
    info("Postprocess done. Time elapsed: %.4f", t.lap());
    return 0;
  }
  mhx_ctx *c = open_gpu();
  info("Device ready. Time elapsed: %.4f", t.lap());
  info("Preparing data...");
  load_read_lib(c, o.get("read_lib_file"));
  info("%llu reads, %llu total bases; Preparing data... Done. Time elapsed: %.4f", (unsigned long long)mhx_num_sequences(c),
       (unsigned long long)mhx_num_bases(c), t.lap());
  if (m > 1) {  // stage 1 is skipped when every edge is solid (main_sdbg_build.cpp:139-147)
    mhx_s1_result r1;
    // --need_mercy: reproduce the reference's kmsort tie order (bit-identical mercy edges); MHX_STABLE_TIES=1
    // selects the faster stable order instead (DESIGN.md "H1")
    const int mercy_mode = !need_mercy ? 0 : (getenv("MHX_STABLE_TIES") ? 1 : 2);
    const size_t s1_item_bytes = 16 + (k > 30 ? (size_t)((2 * (k - 1) + 6 + 31) / 32 - 2 + 1) / 2 * 8 : 0);
    // fixed: 1 B/base mark map + bitmap + the aggregated stage-2 items kept for stage 2 (k <= 22, and k = 23..27 with s1_agg_wide: <= 8 B
    // per base, typically 1)
    const bool s1_items = k <= 22 || (k <= 27 && !need_mercy && mhx_get_option(c, "s1_agg_wide", 0) != 0);
    // Stage 1 on super-k-mer records plans its own passes (include/mhx.h: mhx_s1_self_planned): asked first, unless the environment
    // dictates a plan (MHX_MAX_ITEMS / MHX_FREE_BYTES: tests of the lv1 bucket plan).  If the input turns out not to be served —
    // low-complexity reads — the call fails and the lv1 bucket plan takes over.
    bool s1_done = false;
    if (!getenv("MHX_MAX_ITEMS") && !getenv("MHX_FREE_BYTES") && mhx_s1_self_planned(c, k, m, mercy_mode) == 1) {
      const long long before = mhx_get_option(c, "s1_skm", 1);
      mhx_set_option(c, "s1_skm", 3);
      note_plan_memory((double)mhx_device_free_bytes(c));
      s1_done = mhx_read2sdbg_s1(c, k, m, mercy_mode, &r1) == 0;
      if (!s1_done) info("Stage 1 on super-k-mer records: %s; planning lv1 bucket ranges instead", mhx_last_error());
      mhx_set_option(c, "s1_skm", s1_done ? before : 0);
    }
    if (!s1_done) {
      const auto ranges = plan_ranges(c, mercy_mode ? MHX_STAGE_S1_MERCY : MHX_STAGE_S1, k, m, s1_item_bytes,
                                      (double)mhx_num_bases(c) + 4.0 * (double)mhx_num_sequences(c),
                                      (double)mhx_num_bases(c) * (1.0 + 0.125 + (s1_items ? 1.0 : 0.0)));
      uint64_t n1 = 0;
      for (size_t i = 0; i < ranges.size(); ++i) {
        set_range(c, ranges, i, true);
        CK(mhx_read2sdbg_s1(c, k, m, mercy_mode, &r1));
        n1 += r1.n_items;
      }
      clear_range(c, ranges);
      r1.n_items = n1;
    }
    report_plan_memory(mercy_mode ? MHX_STAGE_S1_MERCY : MHX_STAGE_S1);
    auto hist = fetch<int64_t>(c, MHX_BUF_MUL_HIST);
    int64_t n_solid_edges = 0;
    for (uint32_t i = m; i <= 65535; ++i) n_solid_edges += hist[i];
    info("Total number of solid edges: %lld", (long long)n_solid_edges);
    mhxio::write_counting(out, hist.data());
    info("Stage 1 done (%llu items, %llu solid occurrences). Time elapsed: %.4f", (unsigned long long)r1.n_items,
         (unsigned long long)r1.n_solid, t.lap());
    info("Stage 1 plan: %s", mhx_last_s1_plan(c));
    if (need_mercy) {
      info("Adding mercy edges...");
      uint64_t nm = 0;
      CK(mhx_read2sdbg_add_mercy(c, k, &nm));
      info("Adding mercy Done. Time elapsed: %.4f", t.lap());
      info("Number mercy: %llu", (unsigned long long)nm);
    }
  }
  const size_t s2_item_bytes = (size_t)(((2 * k + 4 + 31) / 32 + 1) / 2 * 2) * 4;
  // per-occurrence path: up to 2 + 4/(solid run) items per base position; the aggregated path (k <= 22, and wherever the handle says
  // stage 1 left the items) is far smaller
  const bool s2_items = m > 1 && (k <= 22 || mhx_s1_left_items(c, k, m) == 1);
  const double s2_items_bound = (s2_items ? 0.5 : 2.2) * (double)mhx_num_bases(c);
  S2CountPlan s2_count;
  const long long from_count_before = mhx_get_option(c, "s2_agg_from_count", 1);
  auto ranges2 = plan_ranges(c, MHX_STAGE_S2, k, m, s2_item_bytes, s2_items_bound, 0, &s2_count);
  SdbgAcc acc;
  bool s2_done = false;
  if (s2_count.passes) {
    // Stage 2 from a count in passes over its own bucket ranges (plan_s2_count_passes): one unfiltered call.  A job the route gives up on — an
    // edge region overflowed, the items exceed the budget — fails the call with that message and nothing published: the lv1 bucket plan
    // with the per-occurrence figure takes over.  Any other failure is an error.
    mhx_sdbg_result pr;
    s2_done = mhx_read2sdbg_s2(c, k, m, &pr) == 0;
    mhx_set_option(c, "s2_count_pass_items", 0);
    mhx_set_option(c, "s2_count_budget_mb", 0);
    mhx_set_option(c, "s2_agg_from_count", from_count_before);
    if (s2_done) acc.add(c, pr);
    else {
      const std::string why = mhx_last_error();
      if (why.find("stage 2 from a count given up") == std::string::npos) fatal("%s", why.c_str());
      info("%s; planning lv1 bucket ranges instead", why.c_str());
      ranges2 = plan_ranges(c, MHX_STAGE_S2, k, m, s2_item_bytes, s2_items_bound);  // (without the route)
    }
  }
  for (size_t i = 0; i < ranges2.size() && !s2_done; ++i) {
    set_range(c, ranges2, i, false);
    mhx_sdbg_result pr;
    CK(mhx_read2sdbg_s2(c, k, m, &pr));
    acc.add(c, pr);
  }
  clear_range(c, ranges2);
  report_plan_memory(MHX_STAGE_S2);
  info("Stage 2 done (%llu items). Time elapsed: %.4f", (unsigned long long)acc.r.n_items, t.lap());
  acc.write(out, k, out_files(n_threads));
  info("Postprocess done. Time elapsed: %.4f", t.lap());
  return finish(c);
}

int main_seq2sdbg(int argc, char **argv) {
  Options o;
  o.add("host_mem", "", false, "0");
  o.add("kmer_size", "k", false, "0");
  o.add("kmer_from", "", false, "0");
  o.add("num_cpu_threads", "t", false, "0");
  o.add("contig", "", false, "");
  o.add("bubble", "", false, "");
  o.add("addi_contig", "", false, "");
  o.add("local_contig", "", false, "");
  o.add("input_prefix", "", false, "");
  o.add("output_prefix", "o", false, "");
  o.add("need_mercy", "", true, "");
  o.add("mem_flag", "", false, "1");
  try {
    o.parse(argc, argv);
    if (o.get("input_prefix").empty() && o.get("contig").empty() && o.get("addi_contig").empty()) throw std::string("No input files!");
    if (atoi(o.get("kmer_size").c_str()) < 9) throw std::string("kmer size must be >= 9!");
    if (atof(o.get("host_mem").c_str()) == 0) throw std::string("Please specify the host memory!");
  } catch (std::string &e) {
    fprintf(stderr,
            "%s\nUsage: sdbg_builder seq2sdbg -k kmer_size --contig contigs.fa [--addi_contig add.fa] [--input_prefix input] -o out\nOptions:\n",
            e.c_str());
    o.usage();
    quit(1);
  }
  const uint32_t k = (uint32_t)atoi(o.get("kmer_size").c_str()), k_from = (uint32_t)atoi(o.get("kmer_from").c_str());
  const int n_threads = num_threads_or_all(atoi(o.get("num_cpu_threads").c_str()));
  const bool need_mercy = !o.get("need_mercy").empty();
  const std::string in = o.get("input_prefix"), out = o.get("output_prefix");
  if (need_mercy && in.empty())  // GenMercyEdges reads <input_prefix>.cand and the sorted edges (seq_to_sdbg.cpp:171-189,435)
    fatal("--need_mercy needs --input_prefix (its .cand file and the sorted edges to search)");
  Timer t;
  if (g_num_gpus > 1) {
    // edges are sharded contiguously over the ranks (their items carry no positions, so any split works); the contigs,
    // a small share of the input, are loaded by rank 0; sorting and emission are balanced by the bucket partition
    const RankSet rs = rank_set();
    mhxio::EdgeSet es;
    if (!in.empty()) {
      es = mhxio::read_edges(in);
      info("Number edges: %llu", (unsigned long long)es.n_edges());
    }
    mhxio::PackedSeqs contigs;
    std::vector<uint16_t> cmult;
    auto read_one = [&](const std::string &f, unsigned kf, unsigned kt) {
      if (f.empty()) return;
      int64_t n = mhxio::read_contigs(f, &contigs, &cmult, k + 1, kf, kt, true);
      info("Read %lld contigs from %s.", (long long)n, f.c_str());
    };
    if (!o.get("contig").empty()) {
      read_one(o.get("contig"), k_from, k);
      read_one(o.get("bubble"), 0, 0);
    }
    read_one(o.get("addi_contig"), 0, 0);
    read_one(o.get("local_contig"), 0, 0);
    // --need_mercy: every rank gets all candidate reads; the search runs against the rank's slice of the sorted edges and
    // the per-position answers are OR-ed over the ranks (mhx_dist_gen_mercy_edges)
    mhxio::PackedSeqs cand;
    if (need_mercy) {
      std::vector<uint32_t> rec = mhxio::read_bin_file(in + ".cand");
      std::vector<uint64_t> off = mhxio::index_bin_records(rec);
      for (size_t i = 0; i < off.size(); ++i) cand.append_packed(&rec[off[i] + 1], rec[off[i]], false);
      info("Adding mercy edges...");
    }
    std::vector<uint64_t> n_mercy(rs.n, 0);
    std::vector<SdbgAcc> part(rs.n);
    run_ranks(rs, [&](int r, mhx_ctx *c, mhx_comm *cm) {
      const uint64_t ne = es.n_edges(), lo = ne * r / rs.n, hi = ne * (r + 1) / rs.n;
      bool loaded = false;
      if (hi > lo) {
        if (need_mercy) mhx_set_option(c, "edges_reserve_permille", mercy_reserve_permille());
        CKT(mhx_load_edges(c, es.data + lo * es.words_per_edge, hi - lo, es.k, es.words_per_edge));
        if (need_mercy) mhx_set_option(c, "edges_reserve_permille", 1000);
        loaded = true;
      }
      if (need_mercy) {
        CKT(mhx_dist_gen_mercy_edges(c, cm, k, cand.words.data(), cand.words.size(), cand.n_seqs(), cand.start.data(), &n_mercy[r]));
        loaded = loaded || mhx_num_sequences(c) > 0;
      }
      if (r == 0 && contigs.n_seqs()) {
        if (loaded)
          CKT(mhx_append_sequences(c, contigs.words.data(), contigs.words.size(), contigs.n_seqs(), 0, contigs.start.data(), cmult.data()));
        else {
          CKT(mhx_load_sequences(c, contigs.words.data(), contigs.words.size(), contigs.n_seqs(), 0, contigs.start.data()));
          CKT(mhx_load_multiplicity(c, cmult.data(), cmult.size()));
        }
        loaded = true;
      }
      if (!loaded) {
        uint64_t zero = 0;
        uint32_t w = 0;
        uint16_t mz = 0;
        CKT(mhx_load_sequences(c, &w, 0, 0, 0, &zero));
        CKT(mhx_load_multiplicity(c, &mz, 0));
      }
      CKT(mhx_dist_setup(c, cm, MHX_STAGE_SEQ2SDBG, k, 0));
      mhx_sdbg_result r2{};
      CKT(mhx_dist_seq2sdbg(c, cm, k, &r2));
      if (r == 0) report_rank_memory(cm);
      part[r].add(fetch_t<uint8_t>(c, MHX_BUF_SDBG_BYTES), fetch_t<uint64_t>(c, MHX_BUF_BUCKET_OFFSET), fetch_t<uint64_t>(c, MHX_BUF_BUCKET_COUNT),
                  fetch_t<uint64_t>(c, MHX_BUF_BUCKET_TIPS), fetch_t<uint64_t>(c, MHX_BUF_BUCKET_LARGE), fetch_t<uint64_t>(c, MHX_BUF_W_COUNT), r2);
    });
    if (need_mercy) info("Number of reads: %llu, Number of mercy edges: %llu", (unsigned long long)cand.n_seqs(), (unsigned long long)n_mercy[0]);
    SdbgAcc acc;
    for (int q = 0; q < rs.n; ++q) acc.add(part[q]);
    info("GPU seq2sdbg done (%llu items). Time elapsed: %.4f", (unsigned long long)acc.r.n_items, t.lap());
    acc.write(out, k, std::max(out_files(n_threads), std::min(rs.n, n_threads)));
    info("Postprocess done. Time elapsed: %.4f", t.lap());
    return 0;
  }
  mhx_ctx *c = open_gpu();
  bool loaded = false;
  if (!in.empty()) {
    mhxio::EdgeSet es = mhxio::read_edges(in);
    info("Number edges: %llu", (unsigned long long)es.n_edges());
    // edges -> gap-free (k+1)-mer store + multiplicities (EdgeReader::ReadSorted/ReadUnsorted, edge_reader.h:24-52): on the GPU
    if (need_mercy) mhx_set_option(c, "edges_reserve_permille", mercy_reserve_permille());
    CK(mhx_load_edges(c, es.data, es.n_edges(), es.k, es.words_per_edge));
    if (need_mercy) mhx_set_option(c, "edges_reserve_permille", 1000);
    loaded = true;
    info("Read %llu edges. Time elapsed: %.4f", (unsigned long long)es.n_edges(), t.lap());
    if (need_mercy) {
      info("Adding mercy edges...");
      std::vector<uint32_t> rec = mhxio::read_bin_file(in + ".cand");
      std::vector<uint64_t> off = mhxio::index_bin_records(rec);
      mhxio::PackedSeqs cand;
      for (size_t i = 0; i < off.size(); ++i) cand.append_packed(&rec[off[i] + 1], rec[off[i]], false);
      uint64_t nm = 0;
      CK(mhx_gen_mercy_edges(c, k, cand.words.data(), cand.words.size(), cand.n_seqs(), cand.start.data(), &nm));
      info("Number of reads: %llu, Number of mercy edges: %llu", (unsigned long long)cand.n_seqs(), (unsigned long long)nm);
      info("Done. Time elapsed: %.4f", t.lap());
    }
  }
  // contigs (reversed; loop contigs extended k_from -> k), bubble, addi, local: seq_to_sdbg.cpp:449-503.  Every file is parsed and packed
  // by a thread of its own (round 6: the sequential parse was most of this sub-program's wall time) and appended on the device in the
  // reference's order
  struct CtgFile {
    std::string path;
    unsigned kf, kt;
    mhxio::PackedSeqs seqs;
    std::vector<uint16_t> mult;
    int64_t n = 0;
  };
  std::vector<CtgFile> files;
  auto want = [&](const std::string &f, unsigned kf, unsigned kt) {
    if (!f.empty()) files.push_back(CtgFile{f, kf, kt, {}, {}, 0});
  };
  if (!o.get("contig").empty()) {
    want(o.get("contig"), k_from, k);
    want(o.get("bubble"), 0, 0);
  }
  want(o.get("addi_contig"), 0, 0);
  want(o.get("local_contig"), 0, 0);
  {
    std::vector<std::thread> th;
    for (const CtgFile &cf : files)  // (a missing file is reported from this thread, as every other failure of the sub-program)
      if (access(cf.path.c_str(), R_OK) != 0) fatal("Cannot open %s", cf.path.c_str());
    for (size_t i = 1; i < files.size(); ++i)
      th.emplace_back([&files, i, k]() { files[i].n = mhxio::read_contigs(files[i].path, &files[i].seqs, &files[i].mult, k + 1, files[i].kf, files[i].kt, true); });
    if (!files.empty()) files[0].n = mhxio::read_contigs(files[0].path, &files[0].seqs, &files[0].mult, k + 1, files[0].kf, files[0].kt, true);
    for (std::thread &t_ : th) t_.join();
  }
  for (CtgFile &cf : files) {
    info("Read %lld contigs from %s.", (long long)cf.n, cf.path.c_str());
    if (!cf.seqs.n_seqs()) continue;
    if (loaded)
      CK(mhx_append_sequences(c, cf.seqs.words.data(), cf.seqs.words.size(), cf.seqs.n_seqs(), 0, cf.seqs.start.data(), cf.mult.data()));
    else {
      CK(mhx_load_sequences(c, cf.seqs.words.data(), cf.seqs.words.size(), cf.seqs.n_seqs(), 0, cf.seqs.start.data()));
      CK(mhx_load_multiplicity(c, cf.mult.data(), cf.mult.size()));
    }
    loaded = true;
  }
  if (!loaded) {
    uint64_t zero = 0;
    uint32_t w = 0;
    CK(mhx_load_sequences(c, &w, 0, 0, 0, &zero));
    uint16_t mz = 0;
    CK(mhx_load_multiplicity(c, &mz, 0));
  }
  info("Finally, %llu sequences, %llu bases. Time elapsed: %.4f", (unsigned long long)mhx_num_sequences(c),
       (unsigned long long)mhx_num_bases(c), t.lap());
  const size_t seq_item_bytes = (size_t)(((2 * k + 20 + 31) / 32 + 1) / 2 * 2) * 4;
  const auto ranges = plan_ranges(c, MHX_STAGE_SEQ2SDBG, k, 0, seq_item_bytes, 2.0 * (double)mhx_num_bases(c) + 4.0 * (double)mhx_num_sequences(c));
  SdbgAcc acc;
  for (size_t i = 0; i < ranges.size(); ++i) {
    set_range(c, ranges, i, false);
    mhx_sdbg_result pr;
    CK(mhx_seq2sdbg(c, k, &pr));
    acc.add(c, pr);
  }
  clear_range(c, ranges);
  report_plan_memory(MHX_STAGE_SEQ2SDBG);
  info("GPU seq2sdbg done (%llu items). Time elapsed: %.4f", (unsigned long long)acc.r.n_items, t.lap());
  acc.write(out, k, out_files(n_threads));
  info("Postprocess done. Time elapsed: %.4f", t.lap());
  return finish(c);
}

// ---------------------------------------------------------------------------
// buildlib (reference src/main_buildlib.cpp + SequenceLibCollection::Build, sequence_lib.cpp:8-91): read-library
// description -> <out>.bin + <out>.lib_info.  The texts are parsed and packed on the GPU (mhx_fastx_to_records);
// a text the GPU parser declines goes through the sequential kseq-compatible parser.  MHX_BUILDLIB_HOST=1 forces that.
// MHX_BUILDLIB_BGZF=1: a library whose files are BGZF throughout is mapped as it is and inflated on the GPU
// (mhx_fastx_bgzf_to_records); any other gzip file, and a BGZF file the GPU declines, is inflated by zlib as ever.
int main_buildlib(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "Usage %s <read_lib_file> <out_prefix>\n", argv[0]);
    quit(1);
  }
  const std::string lib_file = argv[1], out = argv[2];
  Timer t;
  FILE *cfg = fopen(lib_file.c_str(), "r");
  if (!cfg) fatal("File to open read_lib file: %s", lib_file.c_str());
  std::vector<char> cfg_text;
  for (int ch; (ch = fgetc(cfg)) != EOF;) cfg_text.push_back((char)ch);
  fclose(cfg);
  FILE *bin = fopen((out + ".bin").c_str(), "wb");
  if (!bin) fatal("Cannot open %s.bin", out.c_str());
  const bool host_only = getenv("MHX_BUILDLIB_HOST") != nullptr;
  const char *bgzf_env = getenv("MHX_BUILDLIB_BGZF");
  const bool bgzf_route = !host_only && bgzf_env && *bgzf_env && strcmp(bgzf_env, "0") != 0;
  mhx_ctx *c = nullptr;
  struct Lib {
    std::string meta;
    int64_t begin, end;
    unsigned max_len;
    bool paired;
  };
  std::vector<Lib> libs;
  int64_t total_reads = 0, total_bases = 0;
  // the description: per library one free-text line, then "<type> <file> [<file2>]" (sequence_lib.cpp:29-44)
  size_t pos = 0;
  auto next_line = [&](std::string *dst) -> bool {
    if (pos >= cfg_text.size()) return false;
    size_t e = pos;
    while (e < cfg_text.size() && cfg_text[e] != '\n') ++e;
    dst->assign(cfg_text.data() + pos, e - pos);
    pos = e < cfg_text.size() ? e + 1 : e;
    return true;
  };
  std::string meta, spec;
  while (next_line(&meta)) {
    if (!next_line(&spec)) break;
    char type[64] = {0}, f1[4096] = {0}, f2[4096] = {0};
    const int got = sscanf(spec.c_str(), "%63s %4095s %4095s", type, f1, f2);
    const std::string ty = type;
    if (got < 2 || (ty != "pe" && ty != "se" && ty != "interleaved") || (ty == "pe" && got < 3)) {
      fprintf(stderr, "Cannot identify read library type %s\n", type);
      fatal("Valid types: pe, se, interleaved");
    }
    const int64_t begin = total_reads;
    unsigned max_len = 0;
    bool done = false;
    auto write_records = [&](const mhx_fastx_result &r) {
      std::vector<uint32_t> rec(r.n_words);
      if (r.n_words) CK(mhx_fetch(c, MHX_BUF_LIB_RECORDS, rec.data(), 0, r.n_words * 4));
      if (r.n_words && fwrite(rec.data(), 4, rec.size(), bin) != rec.size()) fatal("write error on %s.bin", out.c_str());
      total_reads += (int64_t)r.n_reads;
      total_bases += (int64_t)r.n_bases;
      max_len = r.max_len;
      done = true;
    };
    if (bgzf_route) {
      // the compressed files as they are; both mates must be BGZF throughout, or the whole library is inflated by zlib below
      mhxio::TextFile g1 = mhxio::map_gzip_file(f1), g2;
      if (ty == "pe") g2 = mhxio::map_gzip_file(f2);
      uint64_t n_blocks = 0;
      bool all = g1.data != nullptr && (ty != "pe" || g2.data != nullptr);
      for (const mhxio::TextFile *g : {&g1, &g2}) {
        if (!all || !g->data) continue;
        const mhx::BgzfScan scan = mhx::bgzf_scan(g->data, g->size);
        all = scan.reason == mhx::kBgzfOk;
        n_blocks += scan.blocks.size();
      }
      if (all) {
        if (!c) c = open_gpu();
        mhx_fastx_result r{};
        CK(mhx_fastx_bgzf_to_records(c, g1.data, g1.size, ty == "pe" ? g2.data : nullptr, g2.size, &r));
        if (r.status == 0) {
          info("%s: BGZF, %llu blocks inflated on the GPU", f1, (unsigned long long)n_blocks);
          write_records(r);
        }
      }
      g1.close();
      g2.close();
    }
    mhxio::TextFile t1, t2;
    if (!done) {
      t1 = mhxio::open_text_file(f1);
      if (ty == "pe") t2 = mhxio::open_text_file(f2);
    }
    if (!done && !host_only) {
      if (!c) c = open_gpu();
      mhx_fastx_result r{};
      CK(mhx_fastx_to_records(c, t1.data, t1.size, ty == "pe" ? t2.data : nullptr, t2.size, &r));
      if (r.status == 0) {
        write_records(r);
      } else {
        info("%s: not plain FASTA / four-line FASTQ, using the sequential parser", f1);
      }
    }
    if (!done) {
      std::vector<uint32_t> rec;
      auto add = [&](const char *s, size_t len) {
        const uint32_t L = mhxio::append_bin_record(&rec, s, len);
        total_bases += L;
        ++total_reads;
        max_len = std::max(max_len, L);
      };
      if (ty == "pe") mhxio::parse_fastx_sequential(t1.data, t1.size, add, t2.data ? t2.data : "", t2.size);
      else mhxio::parse_fastx_sequential(t1.data, t1.size, add);
      if (!rec.empty() && fwrite(rec.data(), 4, rec.size(), bin) != rec.size()) fatal("write error on %s.bin", out.c_str());
    }
    t1.close();
    t2.close();
    if (ty != "se" && (total_reads - begin) % 2 != 0) {
      fprintf(stderr, "PE library number of reads is odd: %lld!\n", (long long)(total_reads - begin));
      fatal("File(s): %s", meta.c_str());
    }
    info("Lib %zu (%s): %s, %lld reads, %u max length", libs.size(), meta.c_str(), type, (long long)(total_reads - begin), max_len);
    libs.push_back({meta, begin, total_reads, max_len, ty != "se"});
  }
  if (fclose(bin) != 0) fatal("write error on %s.bin", out.c_str());
  FILE *li = fopen((out + ".lib_info").c_str(), "w");
  if (!li) fatal("Cannot open %s.lib_info", out.c_str());
  fprintf(li, "%lld %lld\n", (long long)total_bases, (long long)total_reads);
  for (const Lib &l : libs) fprintf(li, "%s\n%lld %lld %u %d\n", l.meta.c_str(), (long long)l.begin, (long long)l.end, l.max_len, l.paired ? 1 : 0);
  if (fclose(li) != 0) fatal("write error on %s.lib_info", out.c_str());
  info("buildlib done: %lld reads, %lld bases. Time elapsed: %.4f", (long long)total_reads, (long long)total_bases, t.lap());
  if (c) return finish(c);
  return 0;
}

// ---------------------------------------------------------------------------
// iterate (reference src/main_iterate.cpp): contigs + bubbles of round k and the reads -> <o>.edges.0 / .edges.info, the
// unsorted (k+step+1)-mer edges that feed seq2sdbg of round k+step.  SURVEY section 8f N2.
int main_iterate(int argc, char **argv) {
  Options o;
  o.add("contig_file", "c", false, "");
  o.add("bubble_file", "b", false, "");
  o.add("read_file", "r", false, "");
  o.add("num_cpu_threads", "t", false, "0");
  o.add("kmer_k", "k", false, "0");
  o.add("step", "s", false, "0");
  o.add("output_prefix", "o", false, "");
  int k = 0, step = 0;
  try {
    o.parse(argc, argv);
    k = atoi(o.get("kmer_k").c_str());
    step = atoi(o.get("step").c_str());
    if (k + step >= MHX_MAX_K + 1) throw std::string("kmer_k + step must less than ") + std::to_string(MHX_MAX_K + 1);
    if (o.get("contig_file").empty()) throw std::string("No contig file!");
    if (o.get("bubble_file").empty()) throw std::string("No bubble file!");
    if (o.get("read_file").empty()) throw std::string("No reads file!");
    if (k <= 0) throw std::string("Invalid kmer size!");
    if (step <= 0 || step > 28 || step % 2 == 1) throw std::string("Invalid step size!");
    if (o.get("output_prefix").empty()) throw std::string("No output prefix!");
  } catch (std::string &e) {
    fprintf(stderr, "%s\nUsage: %s [opt]\nopt with (*) are must\nopt:\n", e.c_str(), argv[0]);
    o.usage();
    quit(1);
  }
  Timer t;
  mhx_ctx *c = open_gpu();
  // contigs and bubbles, forward, loop and standalone contigs dropped (async_sequence_reader.h:80)
  mhxio::PackedSeqs ctg;
  std::vector<uint16_t> unused_mult;
  for (const std::string &f : {o.get("contig_file"), o.get("bubble_file")}) {
    const int64_t n = mhxio::read_contigs(f, &ctg, &unused_mult, 0, 0, 0, false, 1u | 2u);
    info("Read %lld contigs", (long long)n);
  }
  mhxio::BinFile bin = mhxio::open_bin_file(o.get("read_file"));
  if (bin.fixed_rw) {
    CK(mhx_load_bin_records(c, bin.data, bin.n_words, bin.n_reads, 0));
    if (bin.n_reads && mhx_fixed_length(c) != bin.data[0]) {
      bin.build_index();
      CK(mhx_load_bin_records(c, bin.data, bin.n_words, bin.n_reads, 0));
    }
  } else {
    CK(mhx_load_bin_records(c, bin.data, bin.n_words, bin.n_reads, 0));
  }
  mhx_iterate_result r{};
  CK(mhx_iterate(c, (uint32_t)k, (uint32_t)step, ctg.words.data(), ctg.words.size(), ctg.n_seqs(), ctg.start.data(), &r));
  info("Number of flank kmers: %llu", (unsigned long long)r.n_flanks);
  std::vector<uint32_t> edges((size_t)r.n_edges * r.words_per_edge);
  if (!edges.empty()) CK(mhx_fetch(c, MHX_BUF_EDGES, edges.data(), 0, edges.size() * 4));
  mhxio::write_edges_unsorted(o.get("output_prefix"), (uint32_t)(k + step), r.words_per_edge, edges.data(), r.n_edges);
  info("Total: %llu. Iterative edges: %llu. Time elapsed: %.4f", (unsigned long long)bin.n_reads, (unsigned long long)r.n_edges, t.lap());
  return finish(c);
}



// ---------------------------------------------------------------------------
// assemble (reference src/main_assemble.cpp) when its options ask for nothing beyond tip trimming, the unitig graph and
// contig output: --bubble_level 0 --prune_level 0 --cleaning_rounds 0 — and, with MHX_ASSEMBLE_CLEAN=1 in the environment,
// with --cleaning_rounds N >= 1 as well: the rounds of RemoveTips and DisconnectWeakLinks on the unitig graph
// (main_assemble.cpp:182-249 at bubble level 0 and prune level 0) — and, with MHX_ASSEMBLE_PRUNE=1, at --prune_level 1 or 2
// (the --min_depth given and > 0, or — with the variable at 2 — inferred on the device: mhx_sdbg_infer_min_depth): RemoveLocalLowDepth inside the rounds (level 2), the
// IterateLocalLowDepth after them and the .addi.fa of the changed contigs (main_assemble.cpp:238-301) — and, with
// MHX_ASSEMBLE_BUBBLE=1 (which implies the other two), at --bubble_level 0..2 and --prune_level 0..3: the naive and complex
// PopBubbles of the rounds, RemoveLowDepth and its pops at prune level 3, the final complex pop after the iteration and the
// --careful_bubble records in .bubble_seq.fa, when --merge_len / --merge_similar fit the similarity kernel's cap at k =
// MHX_MAX_K (include/mhx.h: MHX_SIM_MAX_LEN, MHX_SIM_MAX_INDEL).  Every other option set goes to the reference.
// The SdBG files are read back into HBM, indexed (mhx_sdbg_build_index), trimmed (mhx_sdbg_remove_tips), turned into the
// unitig graph and its contig text (mhx_sdbg_unitigs), cleaned in place (mhx_unitig_*); the host folds palindromes and
// writes the ContigWriter files.  The cleaned result is the reference's at -t 1 whatever -t says.
void add_assemble_options(Options &o) {  // main_assemble.cpp:66-101
  o.add("sdbg_name", "s", false, "");
  o.add("output_prefix", "o", false, "out");
  o.add("num_cpu_threads", "t", false, "0");
  o.add("max_tip_len", "", false, "-1");
  o.add("min_standalone", "", false, "200");
  o.add("bubble_level", "", false, "2");
  o.add("merge_len", "", false, "20");
  o.add("merge_similar", "", false, "0.98");
  o.add("prune_level", "", false, "2");
  o.add("disconnect_ratio", "", false, "0.1");
  o.add("low_local_ratio", "", false, "0.2");
  o.add("cleaning_rounds", "", false, "5");
  o.add("min_depth", "", false, "-1");
  o.add("is_final_round", "", true, "");
  o.add("output_standalone", "", true, "");
  o.add("careful_bubble", "", true, "");
}
// ComplexBubbleRemover::PopBubbles' max_len (bubble_remover.cpp:155-157): unsigned product, double quotient
uint32_t complex_max_len(int merge_len, uint32_t k, double sim) { return (uint32_t)lround((uint32_t)merge_len * k / sim); }
// decided from argv alone, before anything touches HIP (forwarding is an execv)
// value of an opt-in variable: 0 off, 1 the route, 2 the route and, at a prune level >= 1 without a --min_depth > 0, InferMinDepth on
// the device (at 1 such a command line is forwarded, as it always was)
int opt_in_level(const char *name) { return getenv(name) ? atoi(getenv(name)) : 0; }
bool assemble_on_gpu(int argc, char **argv) {
  if (getenv("MHX_ASSEMBLE_REF") && atoi(getenv("MHX_ASSEMBLE_REF")) != 0) return false;
  Options o;
  add_assemble_options(o);
  try {
    o.parse(argc - 1, argv + 1);
  } catch (std::string &) {
    return false;  // the reference reports it
  }
  if (o.get("sdbg_name").empty()) return false;
  const int prune_level = atoi(o.get("prune_level").c_str()), rounds = atoi(o.get("cleaning_rounds").c_str());
  if (getenv("MHX_ASSEMBLE_BUBBLE") && atoi(getenv("MHX_ASSEMBLE_BUBBLE")) != 0) {  // bubble popping and prune level 3 on the GPU: opt-in
    const int bubble_level = atoi(o.get("bubble_level").c_str()), merge_len = atoi(o.get("merge_len").c_str());
    const double sim = atof(o.get("merge_similar").c_str());
    if (bubble_level < 0 || bubble_level > 2 || prune_level < 0 || prune_level > 3 || rounds < 0) return false;
    if (prune_level >= 1 && !(atof(o.get("min_depth").c_str()) > 0) && opt_in_level("MHX_ASSEMBLE_BUBBLE") < 2) return false;  // no depth: inferred only at 2
    if (bubble_level >= 2) {
      // the similarity kernel's cap, at the largest k there is: k is not known before the graph is read
      if (merge_len < 0 || !(sim > 0 && sim <= 1)) return false;
      const double longest = (double)complex_max_len(merge_len, MHX_MAX_K, sim) + MHX_MAX_K;
      if (longest > MHX_SIM_MAX_LEN || longest * (1 - sim) >= MHX_SIM_MAX_INDEL + 1) return false;
    }
    return true;
  }
  if (atoi(o.get("bubble_level").c_str()) != 0) return false;
  const bool prune = getenv("MHX_ASSEMBLE_PRUNE") && atoi(getenv("MHX_ASSEMBLE_PRUNE")) != 0;  // low-depth pruning on the GPU: opt-in
  if (prune_level != 0)  // levels 1 and 2 with a given minimum depth (at 2: or an inferred one); the variable implies the cleaning rounds
    return prune && (prune_level == 1 || prune_level == 2) && (atof(o.get("min_depth").c_str()) > 0 || opt_in_level("MHX_ASSEMBLE_PRUNE") >= 2) && rounds >= 0;
  if (rounds <= 0) return rounds == 0;
  return prune || (getenv("MHX_ASSEMBLE_CLEAN") && atoi(getenv("MHX_ASSEMBLE_CLEAN")) != 0);  // the cleaning rounds on the GPU: opt-in
}
void revcomp_ascii(std::string &s) {  // contig_output.cpp:12-42
  auto comp = [](char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; };
  std::reverse(s.begin(), s.end());
  for (char &c : s) c = comp(c);
}
void fold_palindrome(std::string &s, unsigned k, bool is_loop) {  // contig_output.cpp:43-60
  if (is_loop) {
    for (unsigned i = 1; i + k <= s.length(); ++i) {
      std::string rc = s.substr(i, k);
      revcomp_ascii(rc);
      if (rc == s.substr(i - 1, k)) {
        s = s.substr(i, s.length() / 2);
        break;
      }
    }
  } else {
    const long num_edges = (long)s.length() - (long)k;
    s.resize((size_t)((num_edges - 1) / 2 + k + 1));
  }
}
int main_assemble(int argc, char **argv) {
  Options o;
  add_assemble_options(o);
  try {
    o.parse(argc, argv);
    if (o.get("sdbg_name").empty()) throw std::string("no succinct de Bruijn graph name!");
  } catch (std::string &e) {
    fprintf(stderr, "%s\nUsage: %s -s sdbg_name -o output_prefix\noptions:\n", e.c_str(), argv[0]);
    o.usage();
    quit(1);
  }
  const std::string prefix = o.get("output_prefix");
  const int n_threads = num_threads_or_all(atoi(o.get("num_cpu_threads").c_str()));
  const int min_standalone = atoi(o.get("min_standalone").c_str());
  const bool output_standalone = o.get("output_standalone") == "1";
  Timer t;
  info("Loading succinct de Bruijn graph: %s", o.get("sdbg_name").c_str());
  const mhxio::SdbgFiles f = mhxio::read_sdbg(o.get("sdbg_name"));
  mhx_ctx *c = open_gpu();
  CK(mhx_sdbg_load_bytes(c, f.bytes.data(), f.bytes.size(), f.offset.data(), f.items.data(), f.tips.data(), f.large.data()));
  mhx_sdbg_index_info ix{};
  CK(mhx_sdbg_build_index(c, f.k, &ix));
  info("Done. Time elapsed: %.4f", t.lap());
  info("Number of Edges: %llu; K value: %u", (unsigned long long)ix.n_items, f.k);
  info("Number of CPU threads: %d", n_threads);
  int max_tip_len = atoi(o.get("max_tip_len").c_str());
  if (max_tip_len == -1) max_tip_len = (int)f.k * 2;
  // InferMinDepth on the graph as loaded (main_assemble.cpp:146-150; assemble_on_gpu lets such a command line in only at opt-in
  // level 2).  Prune level 0 never reads the value: nothing is inferred or logged there
  double min_depth = atof(o.get("min_depth").c_str());
  if (atoi(o.get("prune_level").c_str()) >= 1 && !(min_depth > 0)) {
    int converged = 1;
    CK(mhx_sdbg_infer_min_depth(c, &ix, &min_depth, &converged));
    if (!converged) fprintf(stderr, "WARN  Cannot detect min depth: unconverged\n");
    info("min depth set to %.3f", min_depth);
  }
  if (max_tip_len > 0) {
    uint64_t n_tips = 0;
    CK(mhx_sdbg_remove_tips(c, &ix, max_tip_len, &n_tips));
    info("Removing tips with length less than %d; Accumulated tips removed: %llu", max_tip_len, (unsigned long long)n_tips);
    info("Tips removal done! Time elapsed(sec): %.3f", t.lap());
  }
  mhx_unitig_result ur{};
  CK(mhx_sdbg_unitigs(c, &ix, &ur));
  info("Graph size without loops: %llu, palindrome: %llu", (unsigned long long)(ur.n_vertices - ur.n_loops), (unsigned long long)ur.n_palindromes);
  info("unitig graph size: %llu, time for building: %.3f", (unsigned long long)ur.n_vertices, t.lap());
  // CalcAndPrintStat (contig_stat.h:15-47): contig lengths = length + k; std::map order of the names
  auto print_stat = [&](const std::vector<mhx_unitig_vertex> &vtx) {
    std::map<uint64_t, uint64_t> hist;
    uint64_t total = 0, n_looped = 0, n_isolated = 0;
    for (const mhx_unitig_vertex &v : vtx) {
      ++hist[v.length + f.k];
      total += v.length + f.k;
      n_looped += (v.flags & MHX_UNITIG_LOOP) != 0;
      n_isolated += (v.flags & MHX_UNITIG_STANDALONE) != 0;
    }
    uint64_t n50 = 0;
    double acc = 0;
    for (auto it = hist.rbegin(); it != hist.rend(); ++it) {
      acc += (double)it->second * (double)it->first;
      if (acc >= 0.5 * (double)total) {
        n50 = it->first;
        break;
      }
    }
    info("Max: %llu, Min: %llu, N50: %llu, number contigs: %llu, number isolated: %llu, number looped: %llu, total size: %llu, ",
         (unsigned long long)(hist.empty() ? 0 : hist.rbegin()->first), (unsigned long long)(hist.empty() ? 0 : hist.begin()->first),
         (unsigned long long)n50, (unsigned long long)vtx.size(), (unsigned long long)n_isolated, (unsigned long long)n_looped, (unsigned long long)total);
  };
  // graph cleaning (main_assemble.cpp:170-249)
  const int cleaning_rounds = atoi(o.get("cleaning_rounds").c_str()), prune_level = atoi(o.get("prune_level").c_str());
  const int bubble_level = atoi(o.get("bubble_level").c_str()), merge_len = atoi(o.get("merge_len").c_str());
  const bool is_final_round = o.get("is_final_round") == "1", careful_bubble = o.get("careful_bubble") == "1";
  const double low_local_ratio = atof(o.get("low_local_ratio").c_str());
  const double merge_similar = atof(o.get("merge_similar").c_str());
  const uint32_t local_width = 1000;  // AssemblerOptions::local_width: no command-line option sets it
  // the --careful_bubble records of every pass, in call order: ContigWriter records with id 0, flag 0 and the average depth
  std::deque<std::string> bubble_text;
  std::vector<mhxio::ContigRecord> bubble_recs;
  uint64_t n_finishes = 0;  // mid-run finishes the pops needed for their text
  // one PopBubbles call; with_writer: the remover still holds the bubble writer
  auto pop_bubbles = [&](bool complex_mode, bool mark_changed, bool with_writer) {
    uint64_t n_removed = 0, n_records = 0;
    const uint32_t max_len = complex_mode ? complex_max_len(merge_len, f.k, merge_similar) : f.k + 2;
    CK(mhx_unitig_pop_bubbles(c, &ix, max_len, complex_mode ? merge_similar : 0.0, careful_bubble && with_writer ? 0.2 : -1.0, mark_changed ? 1 : 0,
                              &n_removed, &n_records));
    uint64_t st[4] = {0, 0, 0, 0};
    CK(mhx_unitig_bubble_stats(c, st));
    n_finishes += st[3];
    if (complex_mode)  // (not a line of the reference's)
      info("Complex bubble candidates: %llu, similarity passed: %llu, failed: %llu", (unsigned long long)st[0], (unsigned long long)st[1],
           (unsigned long long)st[2]);
    if (n_records) {
      const std::vector<mhx_bubble_record> recs = fetch<mhx_bubble_record>(c, MHX_BUF_UNITIG_BUBBLE_REC);
      const std::vector<char> text = fetch<char>(c, MHX_BUF_UNITIG_BUBBLE_SEQ);
      for (const mhx_bubble_record &r : recs) {
        bubble_text.emplace_back(text.data() + r.offset, r.length);
        bubble_recs.push_back(mhxio::ContigRecord{0, 0, r.avg_depth, bubble_text.back().data(), bubble_text.back().size()});
      }
    }
    return n_removed;
  };
  if (cleaning_rounds > 0) {
    print_stat(fetch<mhx_unitig_vertex>(c, MHX_BUF_UNITIG_VERTICES));
    const double disconnect_ratio = atof(o.get("disconnect_ratio").c_str());
    for (int round = 1; round <= cleaning_rounds; ++round) {
      info("Graph cleaning round %d", round);
      bool changed = false;
      if (round > 1) {
        uint64_t n_tips = 0;
        CK(mhx_unitig_remove_tips(c, &ix, (uint32_t)max_tip_len, &n_tips));
        changed |= n_tips > 0;
        info("Tips removed: %llu, time: %.3f", (unsigned long long)n_tips, t.lap());
      }
      if (bubble_level >= 1) {
        const uint64_t n_bubbles = pop_bubbles(false, false, true);
        info("Number of bubbles removed: %llu, Time elapsed(sec): %.3f", (unsigned long long)n_bubbles, t.lap());
        changed |= n_bubbles > 0;
      }
      if (bubble_level >= 2) {
        const uint64_t n_bubbles = pop_bubbles(true, false, true);
        info("Number of complex bubbles removed: %llu, Time elapsed(sec): %.4f", (unsigned long long)n_bubbles, t.lap());
        changed |= n_bubbles > 0;
      }
      uint64_t n_disconnected = 0;
      CK(mhx_unitig_disconnect_weak_links(c, &ix, disconnect_ratio, &n_disconnected));
      info("Number unitigs disconnected: %llu, time: %.3f", (unsigned long long)n_disconnected, t.lap());
      changed |= n_disconnected > 0;
      if (prune_level >= 3) {  // more-excessive pruning: permanent; its count does not feed `changed`
        uint64_t n_pruned = 0;
        CK(mhx_unitig_remove_low_depth(c, &ix, min_depth, &n_pruned));
        n_pruned += pop_bubbles(false, false, true);
        if (bubble_level >= 2 && merge_len > 0) n_pruned += pop_bubbles(true, false, true);
        info("Unitigs removed in (more-)excessive pruning: %llu, time: %.3f", (unsigned long long)n_pruned, t.lap());
      } else if (prune_level >= 2) {  // excessive pruning: permanent (no marks); its count does not feed `changed`
        uint64_t n_pruned = 0;
        CK(mhx_unitig_remove_local_low_depth(c, &ix, min_depth, (uint32_t)max_tip_len, local_width, std::min(low_local_ratio, 0.1), 0, &n_pruned,
                                             nullptr));
        info("Unitigs removed in excessive pruning: %llu, time: %.3f", (unsigned long long)n_pruned, t.lap());
      }
      if (!changed) break;
    }
    CK(mhx_unitig_finish(c, &ix, &ur));
  }
  std::vector<mhx_unitig_vertex> vtx;
  std::vector<char> seq;
  std::vector<uint64_t> off;
  auto fetch_graph = [&]() {
    vtx = fetch<mhx_unitig_vertex>(c, MHX_BUF_UNITIG_VERTICES);
    seq = fetch<char>(c, MHX_BUF_UNITIG_SEQ);
    off = fetch<uint64_t>(c, MHX_BUF_UNITIG_OFFSET);
    print_stat(vtx);
  };
  // OutputContigs (contig_output.cpp:62-119) with ContigWriter's record format; change_only: the MHX_UNITIG_CHANGED vertices
  // with multiplicity 1 and no split into final contigs, to `path`
  auto output_contigs = [&](bool change_only, const std::string &path) {
    std::vector<mhxio::ContigRecord> main_recs, final_recs;
    std::deque<std::string> folded;
    for (uint64_t i = 0; i < vtx.size(); ++i) {
      const mhx_unitig_vertex &v = vtx[i];
      if (change_only && !(v.flags & MHX_UNITIG_CHANGED)) continue;
      const double multi = change_only ? 1.0 : std::min(65535.0, (double)v.total_depth / v.length);  // kMaxMul
      mhxio::ContigRecord r{i, 0, multi, seq.data() + off[i], (size_t)(off[i + 1] - off[i])};
      const bool loop = v.flags & MHX_UNITIG_LOOP, pal = v.flags & MHX_UNITIG_PALINDROME;
      if (loop || (v.flags & MHX_UNITIG_STANDALONE)) {
        r.flag = loop && !pal ? 3 : 1;  // kLoop | kStandalone, or kStandalone
        if (pal) {
          folded.emplace_back(r.seq, r.len);
          fold_palindrome(folded.back(), f.k, loop);
          r.seq = folded.back().data();
          r.len = folded.back().size();
        }
        if (output_standalone && !change_only) {
          if (r.len >= (size_t)std::max(0, min_standalone)) final_recs.push_back(r);
          continue;
        }
      }
      main_recs.push_back(r);
    }
    mhxio::write_contigs(path, f.k, main_recs, n_threads);
    if (!change_only) mhxio::write_contigs(prefix + ".final.contigs.fa", f.k, final_recs, n_threads);
  };
  fetch_graph();
  if (!(is_final_round && prune_level >= 1)) {  // otherwise output after local low depth pruning
    output_contigs(false, prefix + ".contigs.fa");
    info("Time to output: %.4f", t.lap());
  }
  // remove local low depth & output as contigs (main_assemble.cpp:270-301)
  if (prune_level >= 1) {
    uint64_t n_removed = 0;
    CK(mhx_unitig_iterate_local_low_depth(c, &ix, min_depth, (uint32_t)max_tip_len, local_width, low_local_ratio, is_final_round ? 0 : 1, &n_removed));
    uint64_t n_bubbles = 0;  // the complex remover has lost its writer by now (main_assemble.cpp:282)
    if (bubble_level >= 2 && merge_len > 0) n_bubbles = pop_bubbles(true, true, false);
    info("Number of local low depth unitigs removed: %llu, complex bubbles removed: %llu, time: %.4f", (unsigned long long)n_removed,
         (unsigned long long)n_bubbles, t.lap());
    CK(mhx_unitig_finish(c, &ix, &ur));
    fetch_graph();
    if (!is_final_round) {
      output_contigs(true, prefix + ".addi.fa");
    } else {
      output_contigs(false, prefix + ".contigs.fa");
      mhxio::write_contigs(prefix + ".addi.fa", f.k, {}, 1);  // the writer is opened at every prune level >= 1
    }
    // (the reference computes the changed-only statistics here without printing them: CalcAndPrintStat(graph, false, true))
  }
  mhxio::write_contigs(prefix + ".bubble_seq.fa", f.k, bubble_recs, 1);
  if (bubble_level >= 1) info("Bubble records: %llu, mid-run finishes for their text and the similarity: %llu", (unsigned long long)bubble_recs.size(), (unsigned long long)n_finishes);
  return finish(c);
}

// route one sub-program (argv[0] = program name, argv[1] = sub-program); only the ones this binary implements
int dispatch(int argc, char **argv) {
  const std::string sub = argv[1];
  maybe_pretend_scan_timeout();
  if (sub == "count") return main_kmer_count(argc - 1, argv + 1);
  if (sub == "read2sdbg") return main_read2sdbg(argc - 1, argv + 1);
  if (sub == "seq2sdbg") return main_seq2sdbg(argc - 1, argv + 1);
  if (sub == "buildlib") return main_buildlib(argc - 1, argv + 1);
  if (sub == "iterate") return main_iterate(argc - 1, argv + 1);
  if (sub == "assemble") return main_assemble(argc - 1, argv + 1);
  fatal("sub-program '%s' is not served", sub.c_str());
}

// ---------------------------------------------------------------------------
// Resident server.  Every GPU process pays for device initialisation, for hipMalloc of its working set and — in bursts,
// whenever the driver has to scrub the memory earlier processes gave back before it can hand it out again — seconds of
// waiting inside hipMalloc (profiles/r03_process_churn.json: 1-3 s every third or fourth process at 40 GB each), more
// than the sub-programs' own work.  The reference's orchestrator starts ~4 GPU-path processes per k.
//   mhx_core --serve <socket>          stays, holds ONE handle with its (grow-only) device buffers, runs the requests it
//                                      receives one after the other, leaves after MHX_SERVE_IDLE_S (120) idle seconds
//   MHX_SERVER=<socket> mhx_core ...   sends its command line, working directory, MHX_* environment and its stderr
//                                      (descriptor passing) to the server and exits with the status it gets back;
//                                      with MHX_SERVER_AUTOSTART=1 it starts the server when none listens; if no server
//                                      can be reached it does the work itself, as without MHX_SERVER
//   mhx_core --serve-stop <socket>     asks the server to leave now
// Request: u32 argc, {u32 len, bytes}*, u32 n_env, {u32 len, bytes "NAME=value"}*, u32 len + cwd, then one byte carrying
// the client's stderr as SCM_RIGHTS.  Reply: one status byte.
namespace serve_io {
bool write_all(int fd, const void *p, size_t n) {
  const char *c = static_cast<const char *>(p);
  while (n) {
    const ssize_t w = write(fd, c, n);
    if (w < 0 && errno == EINTR) continue;
    if (w <= 0) return false;
    c += w;
    n -= (size_t)w;
  }
  return true;
}
bool read_all(int fd, void *p, size_t n) {
  char *c = static_cast<char *>(p);
  while (n) {
    const ssize_t r = read(fd, c, n);
    if (r < 0 && errno == EINTR) continue;
    if (r <= 0) return false;
    c += r;
    n -= (size_t)r;
  }
  return true;
}
bool put_str(int fd, const std::string &v) {
  const uint32_t n = (uint32_t)v.size();
  return write_all(fd, &n, 4) && write_all(fd, v.data(), n);
}
bool get_str(int fd, std::string *v) {
  uint32_t n = 0;
  if (!read_all(fd, &n, 4) || n > (1u << 20)) return false;
  v->resize(n);
  return n == 0 || read_all(fd, &(*v)[0], n);
}
bool send_fd(int sock, int fd) {
  char byte = 'F', ctrl[CMSG_SPACE(sizeof(int))];
  memset(ctrl, 0, sizeof ctrl);
  iovec iov{&byte, 1};
  msghdr msg{};
  msg.msg_iov = &iov;
  msg.msg_iovlen = 1;
  msg.msg_control = ctrl;
  msg.msg_controllen = sizeof ctrl;
  cmsghdr *cm = CMSG_FIRSTHDR(&msg);
  cm->cmsg_level = SOL_SOCKET;
  cm->cmsg_type = SCM_RIGHTS;
  cm->cmsg_len = CMSG_LEN(sizeof(int));
  memcpy(CMSG_DATA(cm), &fd, sizeof(int));
  return sendmsg(sock, &msg, 0) == 1;
}
int recv_fd(int sock) {
  char byte = 0, ctrl[CMSG_SPACE(sizeof(int))];
  iovec iov{&byte, 1};
  msghdr msg{};
  msg.msg_iov = &iov;
  msg.msg_iovlen = 1;
  msg.msg_control = ctrl;
  msg.msg_controllen = sizeof ctrl;
  if (recvmsg(sock, &msg, 0) != 1) return -1;
  for (cmsghdr *cm = CMSG_FIRSTHDR(&msg); cm; cm = CMSG_NXTHDR(&msg, cm))
    if (cm->cmsg_level == SOL_SOCKET && cm->cmsg_type == SCM_RIGHTS) {
      int fd = -1;
      memcpy(&fd, CMSG_DATA(cm), sizeof(int));
      return fd;
    }
  return -1;
}
int connect_to(const char *path) {
  sockaddr_un a{};
  a.sun_family = AF_UNIX;
  if (strlen(path) >= sizeof a.sun_path) return -1;
  strcpy(a.sun_path, path);
  const int fd = socket(AF_UNIX, SOCK_STREAM, 0);
  if (fd < 0) return -1;
  if (connect(fd, reinterpret_cast<sockaddr *>(&a), sizeof a) != 0) {
    close(fd);
    return -1;
  }
  return fd;
}
}  // namespace serve_io

int serve(const char *path) {
  using namespace serve_io;
  signal(SIGPIPE, SIG_IGN);
  sockaddr_un a{};
  a.sun_family = AF_UNIX;
  if (strlen(path) >= sizeof a.sun_path) fatal("socket path too long: %s", path);
  strcpy(a.sun_path, path);
  const int ls = socket(AF_UNIX, SOCK_STREAM, 0);
  if (ls < 0) fatal("socket: %s", strerror(errno));
  if (connect_to(path) >= 0) fatal("a server already listens on %s", path);
  unlink(path);
  // the socket is this user's alone: a request carries argv, a working directory and environment settings, i.e. whoever may
  // connect may write files as the server's user
  const mode_t old_mask = umask(0177);
  const bool bound = bind(ls, reinterpret_cast<sockaddr *>(&a), sizeof a) == 0;
  umask(old_mask);
  if (!bound || chmod(path, 0600) != 0 || listen(ls, 16) != 0) fatal("cannot listen on %s: %s", path, strerror(errno));
  const int idle_s = getenv("MHX_SERVE_IDLE_S") ? std::max(1, atoi(getenv("MHX_SERVE_IDLE_S"))) : 120;
  g_serving = true;
  mhxio::g_fatal_throws = true;
  info("serving on %s (leaves after %d idle seconds)", path, idle_s);
  uint64_t served = 0;
  for (;;) {
    pollfd pf{ls, POLLIN, 0};
    const int pr = poll(&pf, 1, idle_s * 1000);
    if (pr < 0 && errno == EINTR) continue;
    if (pr <= 0) break;  // idle
    const int fd = accept(ls, nullptr, nullptr);
    if (fd < 0) continue;
    {  // same user only, and a client that stalls in the middle of its request does not hold the server for the others
      ucred cr{};
      socklen_t cl = sizeof cr;
      if (getsockopt(fd, SOL_SOCKET, SO_PEERCRED, &cr, &cl) != 0 || cr.uid != geteuid()) {
        close(fd);
        continue;
      }
      timeval tv{10, 0};
      setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
    }
    uint32_t argc = 0, n_env = 0;
    std::vector<std::string> args, envs;
    std::string cwd;
    bool ok = read_all(fd, &argc, 4) && argc >= 1 && argc < 4096;
    for (uint32_t i = 0; ok && i < argc; ++i) {
      args.emplace_back();
      ok = get_str(fd, &args.back());
    }
    ok = ok && read_all(fd, &n_env, 4) && n_env < 4096;
    for (uint32_t i = 0; ok && i < n_env; ++i) {
      envs.emplace_back();
      ok = get_str(fd, &envs.back());
    }
    ok = ok && get_str(fd, &cwd);
    const int err_fd = ok ? recv_fd(fd) : -1;
    if (!ok || err_fd < 0) {
      if (err_fd >= 0) close(err_fd);
      close(fd);
      continue;
    }
    if (args[0] == "--serve-stop") {
      const unsigned char st = 0;
      (void)write_all(fd, &st, 1);
      close(err_fd);
      close(fd);
      break;
    }
    // the request's world: its stderr, its working directory, its MHX_* settings
    fflush(nullptr);
    const int saved_err = dup(2);
    dup2(err_fd, 2);
    close(err_fd);
    char old_cwd[4096] = "";
    if (!getcwd(old_cwd, sizeof old_cwd)) old_cwd[0] = 0;
    std::vector<std::pair<std::string, std::string>> restore;  // (name, previous value or "\x01" for unset)
    std::vector<std::string> drop;                             // MHX_* of the server that the client does not have
    for (char **e = environ; *e; ++e)
      if ((!strncmp(*e, "MHX_", 4) && strncmp(*e, "MHX_SERVE", 9)) || !strncmp(*e, "MEGAHIT_NUM_MERCY_FACTOR=", 25)) {
        const std::string kv = *e, name = kv.substr(0, kv.find('='));
        bool sent = false;
        for (const std::string &x : envs) sent = sent || x.compare(0, name.size() + 1, name + "=") == 0;
        if (!sent) drop.push_back(kv);
      }
    for (const std::string &kv : drop) {
      const std::string name = kv.substr(0, kv.find('='));
      restore.push_back({name, kv.substr(name.size() + 1)});
      unsetenv(name.c_str());
    }
    for (const std::string &kv : envs) {
      const size_t eq = kv.find('=');
      if (eq == std::string::npos) continue;
      const std::string name = kv.substr(0, eq);
      const char *prev = getenv(name.c_str());
      restore.push_back({name, prev ? std::string(prev) : std::string("\x01")});
      setenv(name.c_str(), kv.c_str() + eq + 1, 1);
    }
    unsigned char status = 1;
    if (chdir(cwd.c_str()) != 0) {
      fprintf(stderr, "FATAL cannot enter %s\n", cwd.c_str());
    } else {
      std::vector<char *> argv;
      static char prog[] = "mhx_core";
      argv.push_back(prog);
      for (std::string &x : args) argv.push_back(&x[0]);
      argv.push_back(nullptr);
      try {
        try {
          status = (unsigned char)dispatch((int)argv.size() - 1, argv.data());
        } catch (const RetryClassic &) {  // as the front process does for a worker (main): once more, without the chained scan
          setenv("MHX_SORT", "classic", 1);
          restore.emplace_back("MHX_SORT", "\x01");
          status = (unsigned char)dispatch((int)argv.size() - 1, argv.data());
        }
      } catch (const RetryClassic &) {
        status = 1;
      } catch (const mhxio::Fatal &) {
        status = 1;
      } catch (const std::string &e) {
        fprintf(stderr, "%s\n", e.c_str());
        status = 1;
      } catch (const std::exception &e) {
        fprintf(stderr, "FATAL %s\n", e.what());
        status = 1;
      }
    }
    fflush(nullptr);
    dup2(saved_err, 2);
    close(saved_err);
    if (old_cwd[0] && chdir(old_cwd) != 0) {
    }
    for (auto it = restore.rbegin(); it != restore.rend(); ++it) {
      if (it->second == "\x01") unsetenv(it->first.c_str());
      else setenv(it->first.c_str(), it->second.c_str(), 1);
    }
    (void)write_all(fd, &status, 1);
    close(fd);
    ++served;
  }
  info("server on %s leaves after %llu requests", path, (unsigned long long)served);
  if (g_served_ctx) mhx_destroy(g_served_ctx);
  close(ls);
  unlink(path);
  fflush(nullptr);
  _exit(0);
}

// the client side: -1 = not served (do the work here), else the exit status the server reported
int try_server(int argc, char **argv) {
  using namespace serve_io;
  const char *path = getenv("MHX_SERVER");
  if (!path || !*path || !strcmp(path, "off") || !strcmp(path, "0")) return -1;
  int fd = connect_to(path);
  if (fd < 0 && getenv("MHX_SERVER_AUTOSTART")) {
    const pid_t pid = fork();
    if (pid == 0) {  // detach: the server must survive this client and must not hold its pipes
      setsid();
      const int nul = open("/dev/null", O_RDWR);
      const char *logp = getenv("MHX_SERVER_LOG");
      const int lg = logp ? open(logp, O_WRONLY | O_CREAT | O_APPEND, 0644) : -1;
      dup2(nul, 0);
      dup2(nul, 1);
      dup2(lg >= 0 ? lg : nul, 2);
      for (int f = 3; f < 256; ++f) close(f);
      if (fork() != 0) _exit(0);
      char self[4096];
      const ssize_t n = readlink("/proc/self/exe", self, sizeof self - 1);
      if (n <= 0) _exit(1);
      self[n] = 0;
      execl(self, self, "--serve", path, (char *)nullptr);
      _exit(1);
    }
    if (pid > 0) {
      int ws = 0;
      while (waitpid(pid, &ws, 0) < 0 && errno == EINTR) {
      }
      for (int i = 0; i < 200 && fd < 0; ++i) {  // up to 10 s for the socket to appear
        usleep(50000);
        fd = connect_to(path);
      }
    }
  }
  if (fd < 0) return -1;
  {  // the listener has to be this user's: a request hands over argv, the working directory, MHX_* settings and this process's
     // stderr, and the answer decides whether the pipeline goes on — never to a socket somebody else bound under that name
    ucred cr{};
    socklen_t cl = sizeof cr;
    if (getsockopt(fd, SOL_SOCKET, SO_PEERCRED, &cr, &cl) != 0 || cr.uid != geteuid()) {
      close(fd);
      return -1;
    }
  }
  bool ok = true;
  const uint32_t n = (uint32_t)(argc - 1);
  ok = write_all(fd, &n, 4);
  for (int i = 1; ok && i < argc; ++i) ok = put_str(fd, argv[i]);
  std::vector<std::string> envs;
  for (char **e = environ; *e; ++e)
    if ((!strncmp(*e, "MHX_", 4) && strncmp(*e, "MHX_SERVE", 9)) || !strncmp(*e, "MEGAHIT_NUM_MERCY_FACTOR=", 25)) envs.push_back(*e);
  const uint32_t ne = (uint32_t)envs.size();
  ok = ok && write_all(fd, &ne, 4);
  for (const std::string &x : envs) ok = ok && put_str(fd, x);
  char cwd[4096] = ".";
  if (!getcwd(cwd, sizeof cwd)) strcpy(cwd, ".");
  ok = ok && put_str(fd, cwd) && send_fd(fd, 2);
  if (!ok) {  // nothing has run yet: do the work here
    close(fd);
    return -1;
  }
  unsigned char st = 1;
  if (!read_all(fd, &st, 1)) st = 1;  // the server went away in the middle of the request
  close(fd);
  return st;
}

}  // namespace

// where the default server of this user, device and set of visible devices listens ("" = nowhere safe: no server by default)
static std::string default_server_socket() {
  const char *dir = getenv("XDG_RUNTIME_DIR");
  const char *dev = getenv("MHX_DEVICE");
  // one server per user, device AND set of visible devices: "device 0" of a job that a scheduler gave another GPU
  // (HIP_/ROCR_/CUDA_VISIBLE_DEVICES) is not the device 0 a server started by an earlier job holds
  std::string vis;
  for (const char *vn : {"HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "GPU_DEVICE_ORDINAL"})
    if (const char *v = getenv(vn)) vis += std::string(vn) + "=" + v + ";";
  char vtag[24] = "";
  if (!vis.empty()) {
    uint64_t h = 1469598103934665603ull;  // FNV-1a
    for (unsigned char ch : vis) h = (h ^ ch) * 1099511628211ull;
    snprintf(vtag, sizeof vtag, "-v%010llx", (unsigned long long)(h & 0xFFFFFFFFFFull));
  }
  const std::string name = "/mhx-core-" + std::to_string((unsigned)geteuid()) + "-dev" + (dev ? dev : "0") + vtag + ".sock";
  std::string path = std::string(dir && *dir ? dir : "") + name;
  if (!(dir && *dir) || path.size() >= sizeof(sockaddr_un{}.sun_path)) {
    // no runtime directory (batch jobs), or an address too long for a socket (~107 characters): a directory of this
    // user's own under /tmp, mode 0700, checked — in /tmp itself any local user could bind the name first
    const std::string own = "/tmp/mhx-" + std::to_string((unsigned)geteuid());
    struct stat sb{};
    const bool made = mkdir(own.c_str(), 0700) == 0 || errno == EEXIST;
    if (made && lstat(own.c_str(), &sb) == 0 && S_ISDIR(sb.st_mode) && sb.st_uid == geteuid() && (sb.st_mode & 077) == 0) path = own + name;
    else path.clear();  // no safe place: every sub-program is a process of its own, as under mhx_core's own name
  }
  return !path.empty() && path.size() < sizeof(sockaddr_un{}.sun_path) ? path : std::string();
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "Usage: %s <sub_program> [sub options]\n    sub-programs: buildlib count read2sdbg seq2sdbg iterate (GPU); others via MHX_REF_CORE\n"
            "    %s --serve <socket> | --serve-stop <socket>   (resident server, see MHX_SERVER)\n", argv[0], argv[0]);
    return 1;
  }
  if (!strcmp(argv[1], "--serve") && argc >= 3) return serve(argv[2]);
  if (!strcmp(argv[1], "--default-socket")) {  // (for scripts that want to stop or watch the default server: tests, bench.py)
    printf("%s\n", default_server_socket().c_str());
    return 0;
  }
  if (!strcmp(argv[1], "--serve-stop") && argc >= 3) {
    setenv("MHX_SERVER", argv[2], 1);
    unsetenv("MHX_SERVER_AUTOSTART");
    const int st = try_server(argc, argv);
    return st < 0 ? 1 : st;
  }
  // `mhx_core --gpus N <sub-program> ...` (or MHX_NUM_GPUS): our only addition to the reference's command line; it sits
  // before the sub-program so that the sub-programs' own option sets stay the reference's
  if (const char *e = getenv("MHX_NUM_GPUS")) g_num_gpus = std::max(1, atoi(e));
  if (!strcmp(argv[1], "--gpus") && argc >= 4) {
    g_num_gpus = std::max(1, atoi(argv[2]));
    argv[2] = argv[0];
    argv += 2;
    argc -= 2;
  }
  // Started under the reference's own name (a link megahit_core -> mhx_core, which is how an unmodified orchestrator finds
  // us: INTEGRATION.md §1) the sub-programs of a pipeline run one behind the other, and each new process would pay for the
  // device memory the one before it gave back (the driver scrubs returned memory: 1-4 s per process at 40-240 GB).  So under
  // that name the resident server is the default: one per user and device, started on first use, gone after two idle minutes.
  // MHX_SERVER=off (or any explicit MHX_SERVER) overrides; if no server can be reached the work is done here as ever.
  {
    const char *base = strrchr(argv[0], '/');
    base = base ? base + 1 : argv[0];
    if (!strcmp(base, "megahit_core") && !getenv("MHX_SERVER")) {
      const std::string path = default_server_socket();
      if (!path.empty()) {
        setenv("MHX_SERVER", path.c_str(), 1);
        setenv("MHX_SERVER_AUTOSTART", "1", 0);
      }
    }
  }
  const std::string sub = argv[1];
  const bool ours = sub == "count" || sub == "read2sdbg" || sub == "seq2sdbg" || (sub == "buildlib" && !getenv("MHX_BUILDLIB_REF")) ||
                    (sub == "iterate" && !getenv("MHX_ITERATE_REF")) || (sub == "assemble" && assemble_on_gpu(argc, argv));
  if (ours && g_num_gpus == 1) {
    const int st = try_server(argc, argv);
    if (st >= 0) return st;
  }
  if (ours && !getenv("MHX_NO_FORK") && !getenv("MHX_CLEAN_EXIT")) {
    // the work runs in a child (forked before anything touches the HIP runtime); this front process only waits for the
    // child's "outputs are complete" byte (finish()) or, failing that, for its exit status
    for (int attempt = 0; attempt < 2; ++attempt) {
      int fds[2];
      if (pipe(fds) != 0) break;
      fflush(nullptr);
      const pid_t pid = fork();
      if (pid == 0) {
        close(fds[0]);
        (void)fcntl(fds[1], F_SETFD, FD_CLOEXEC);
        (void)prctl(PR_SET_PDEATHSIG, SIGKILL);  // no orphan if the front process is killed
        g_done_fd = fds[1];
        break;  // the worker: on to the sub-program
      }
      if (pid < 0) {
        close(fds[0]);
        close(fds[1]);
        break;  // no child: do the work here
      }
      close(fds[1]);
      unsigned char st = 0;
      ssize_t got;
      do got = read(fds[0], &st, 1);
      while (got < 0 && errno == EINTR);
      close(fds[0]);
      // MHX_EARLY_EXIT=1: return as soon as the outputs are complete, while the worker still gives its device memory back
      // (a caller that starts the next GPU process right away then waits in hipMalloc and sees less free memory than
      // there will be: the reference's orchestrator runs its sub-programs back to back).  Default: wait for the worker.
      if (got == 1 && st != kRetryClassicSort && getenv("MHX_EARLY_EXIT")) _exit(st);
      int ws = 0;
      while (waitpid(pid, &ws, 0) < 0 && errno == EINTR) {
      }
      if (got == 1 && st == kRetryClassicSort && attempt == 0) {  // once more, without the chained scan
        setenv("MHX_SORT", "classic", 1);
        continue;
      }
      if (got == 1 && st != kRetryClassicSort) return st;  // "outputs complete" (0): the worker's own exit is teardown only
      return WIFEXITED(ws) ? WEXITSTATUS(ws) : 128 + WTERMSIG(ws);
    }
  }
  if (g_num_gpus > 1) {
    const int have = mhx_device_count();
    if (!getenv("MHX_GPU_MAP") && have > 0 && g_num_gpus > have) {
      info("--gpus %d but only %d device(s) visible: using %d", g_num_gpus, have, have);
      g_num_gpus = have;
    }
  }
  if (ours) return dispatch(argc, argv);
  if (sub == "kmax") { printf("%d\n", MHX_MAX_K); return 0; }
  if (const char *ref = getenv("MHX_REF_CORE")) {
    execv(ref, argv);  // buildlib / assemble / iterate / local / ... : not on this path
    perror("execv MHX_REF_CORE");
    return 1;
  }
  fprintf(stderr, "sub-program '%s' is outside the SdBG-construction path; set MHX_REF_CORE to a reference megahit_core to forward it\n",
          sub.c_str());
  return 1;
}
