// CPU check of megahit_amd/csrc/skm_giant.h: the rounds of a bin of the group-by on super-k-mer records from a chosen start (sub0, rj0) —
// the good rounds reached partition exactly the hashes of that start, for every start of a depth they partition all hashes, (0, 0) is the
// rule the kernels had before, step by step, a round that stays bad gives up at depth 31 — and the plan that gives every giant bin its
// depth: the cap, the list, the work budget, a forced count, bins of different size.  Prints "ok"; a failed check says where.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "skm_giant.h"

using namespace mhx;

static int fails = 0;
#define CHECK(cond, ...)                              \
  do {                                                \
    if (!(cond)) {                                    \
      if (++fails <= 20) {                            \
        fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);                 \
        fprintf(stderr, "\n");                        \
      }                                               \
    }                                                 \
  } while (0)

// the rule of k_s1_skm / k_count_skm before the header: a whole bin, from (0, 0)
static void old_next(uint32_t sub, uint32_t rj, bool bad, uint32_t *nsub_o, uint32_t *nrj_o, bool *done_o, bool *give_up_o) {
  uint32_t nsub = sub, nrj = rj;
  bool done = false, give_up = false;
  if (bad) {
    if (sub >= 31) {
      give_up = true;
      done = true;
    } else {
      nsub = sub + 1;
      nrj = rj << 1;
    }
  } else {
    nrj = rj + 1;
    while (nsub > 0 && (nrj & 1u) == 0) {
      --nsub;
      nrj >>= 1;
    }
    done = nsub == 0 && nrj == 1u;
  }
  *nsub_o = nsub, *nrj_o = nrj, *done_o = done, *give_up_o = give_up;
}

static uint32_t in_round_count(const std::vector<uint32_t> &h, uint32_t sub, uint32_t rj) {
  uint32_t n = 0;
  for (uint32_t v : h) n += skm_in_round(v, sub, rj) ? 1u : 0u;
  return n;
}

// the traversal from (sub0, rj0) with rounds of more than `thr` hashes bad: taken[i] += 1 for every hash of a good round.  -> gave up?
static bool traverse(const std::vector<uint32_t> &h, uint32_t thr, uint32_t sub0, uint32_t rj0, std::vector<uint32_t> &taken, bool against_old) {
  uint32_t sub = sub0, rj = rj0;
  for (long step = 0;; ++step) {
    if (step > 40L * (long)h.size() + 4096) {
      CHECK(false, "no end from (%u, %u)", sub0, rj0);
      return true;
    }
    CHECK(sub >= sub0 && sub <= 31 && (sub == 0 ? rj == 0 : (uint64_t)rj < (1ull << sub)) && (rj >> (sub - sub0)) == rj0, "round (%u, %u) is not below (%u, %u)", sub,
          rj, sub0, rj0);
    const bool bad = in_round_count(h, sub, rj) > thr;
    if (!bad)
      for (size_t i = 0; i < h.size(); ++i)
        if (skm_in_round(h[i], sub, rj)) ++taken[i];
    uint32_t nsub, nrj;
    bool done, give_up;
    skm_next_round(sub, rj, bad, sub0, rj0, &nsub, &nrj, &done, &give_up);
    if (against_old) {
      uint32_t osub, orj;
      bool odone, ogive;
      old_next(sub, rj, bad, &osub, &orj, &odone, &ogive);
      CHECK(osub == nsub && orj == nrj && odone == done && ogive == give_up, "(%u, %u) bad %d: (%u, %u) done %d, before (%u, %u) done %d", sub, rj, (int)bad, nsub,
            nrj, (int)done, osub, orj, (int)odone);
    }
    if (give_up) {
      CHECK(done && sub == 31 && bad, "gives up at (%u, %u)", sub, rj);
      return true;
    }
    if (done) {
      CHECK(nsub == sub0 && nrj == rj0 + 1, "done at (%u, %u), not at (%u, %u)", nsub, nrj, sub0, rj0 + 1);
      return false;
    }
    sub = nsub;
    rj = nrj;
  }
}

static void check_traversal() {
  std::mt19937 rng(20261020);
  CHECK(skm_in_round(0u, 0, 0) && skm_in_round(~0u, 0, 0) && skm_in_round(0x80000000u, 1, 1) && !skm_in_round(0x7FFFFFFFu, 1, 1) && skm_in_round(~0u, 31, 0x7FFFFFFFu) &&
            skm_in_round(0xFFFFFFFEu, 31, 0x7FFFFFFFu) && !skm_in_round(0xFFFFFFFDu, 31, 0x7FFFFFFFu),
        "skm_in_round");
  for (int trial = 0; trial < 12; ++trial) {
    const size_t n = trial == 0 ? 0 : (trial == 1 ? 1 : 1 + rng() % 1500);
    std::vector<uint32_t> h(n);
    for (auto &v : h) v = rng();
    if (trial % 3 == 2)  // hashes crowded into a few subtrees: deep recursion below some starts, empty slices elsewhere
      for (auto &v : h) v = (v >> 7) | ((rng() % 3) << 29);
    {  // (distinct: equal hashes stay together down to depth 31)
      std::vector<uint32_t> s = h;
      std::sort(s.begin(), s.end());
      s.erase(std::unique(s.begin(), s.end()), s.end());
      h = s;
      std::shuffle(h.begin(), h.end(), rng);
    }
    const uint32_t thrs[4] = {1, 3, 40, (uint32_t)(1 + rng() % 600)};
    for (uint32_t thr : thrs) {
      for (uint32_t sub0 : {0u, 1u, 5u, 10u}) {
        std::vector<uint32_t> all(h.size(), 0);
        for (uint32_t rj0 = 0; rj0 < (1u << sub0); ++rj0) {  // (every start of the depth, also at depth 10: their union is checked below)
          std::vector<uint32_t> taken(h.size(), 0);
          const bool gave_up = traverse(h, thr, sub0, rj0, taken, sub0 == 0);
          CHECK(!gave_up, "gave up from (%u, %u), threshold %u", sub0, rj0, thr);
          for (size_t i = 0; i < h.size(); ++i) {
            CHECK(taken[i] == (skm_in_round(h[i], sub0, rj0) ? 1u : 0u), "hash %08x taken %u times from (%u, %u), threshold %u", h[i], taken[i], sub0, rj0, thr);
            all[i] += taken[i];
          }
        }
        for (size_t i = 0; i < h.size(); ++i) CHECK(all[i] == 1, "hash %08x taken %u times over the starts of depth %u", h[i], all[i], sub0);
      }
    }
  }
  // a round that is bad whatever its depth (one key more often than the table holds): given up at depth 31, from any start
  std::vector<uint32_t> same(50, 0xDEADBEEFu);
  for (uint32_t sub0 : {0u, 1u, 5u, 10u}) {
    std::vector<uint32_t> taken(same.size(), 0);
    const uint32_t rj0 = sub0 ? 0xDEADBEEFu >> (32 - sub0) : 0u;
    CHECK(traverse(same, 7, sub0, rj0, taken, sub0 == 0), "no give-up from depth %u", sub0);
    for (uint32_t t : taken) CHECK(t == 0, "a hash of a bad round was taken");
  }
}

static SkmGiantVerdict plan(const std::vector<uint64_t> &recs, uint64_t n, double wpr, const SkmGiantKnobs &kn, std::vector<uint8_t> &d) {
  d.assign(recs.size() + 1, 0xEE);
  return skm_giant_plan(recs.data(), (int)recs.size(), n, wpr, kn, d.data());
}

static void check_plan() {
  const SkmGiantKnobs def;
  CHECK(def.max_records == (1ull << 21) && def.keys == 4096 && def.work_pct == 25 && def.slices == 0, "defaults");
  std::vector<uint8_t> d;
  const uint64_t big = 1ull << 40;
  // the cap
  CHECK(plan({def.max_records + 1}, big, 3.5, def, d) == kSkmGiantCap, "a bin over the cap");
  CHECK(plan({70000, def.max_records + 1, 80000}, big, 3.5, def, d) == kSkmGiantCap, "a bin over the cap among others");
  CHECK(plan({def.max_records}, big, 3.5, def, d) == kSkmGiantServed && d[0] == 10, "a bin at the cap: depth %u", d[0]);  // 3.5 x 2^20 / 4096 = 896 -> 1024
  // the list
  CHECK(plan(std::vector<uint64_t>(1025, 70000), big, 3.5, def, d) == kSkmGiantList, "1025 bins");
  CHECK(plan(std::vector<uint64_t>(1024, 70000), big, 3.5, def, d) == kSkmGiantServed, "1024 bins");
  for (int g = 0; g < 1024; ++g) CHECK(d[g] == 6, "bin %d of 1024: depth %u", g, d[g]);  // 245 000 / 4096 = 59.8 -> 64
  CHECK(plan({}, 1000, 3.5, def, d) == kSkmGiantServed, "no bin");
  // wanted slices: estimated windows / keys, up to a power of two, at most 2^10; each bin its own
  CHECK(plan({100000, 20000}, big, 3.5, def, d) == kSkmGiantServed && d[0] == 7 && d[1] == 5, "two sizes: %u %u", d[0], d[1]);  // 85.4 -> 128, 17.1 -> 32
  CHECK(plan({4096, 4097, 1000}, big, 1.0, def, d) == kSkmGiantServed && d[0] == 0 && d[1] == 1 && d[2] == 0, "at and over one slice: %u %u %u", d[0], d[1], d[2]);
  SkmGiantKnobs kn = def;
  kn.keys = 2048;
  CHECK(plan({1ull << 20}, big, 3.5, kn, d) == kSkmGiantServed && d[0] == 10, "more wanted than 2^10: depth %u", d[0]);
  kn.keys = 7168;
  CHECK(plan({100000}, big, 3.5, kn, d) == kSkmGiantServed && d[0] == 6, "keys 7168: depth %u", d[0]);  // 48.8 -> 64
  // the work budget: the sum of slices x records within n x 25 / 100, the costliest bin halved first
  CHECK(plan({100000, 20000}, 16000000, 3.5, def, d) == kSkmGiantServed && d[0] == 5 && d[1] == 5, "budget 4 M: %u %u", d[0], d[1]);  // 12.8 M + 0.64 M -> 3.2 M + 0.64 M
  CHECK(plan({100000, 20000}, 4000000, 3.5, def, d) == kSkmGiantServed && d[0] == 2 && d[1] == 4, "budget 1 M: %u %u", d[0], d[1]);  // -> 0.4 M + 0.32 M
  CHECK(plan({100000, 20000}, 480000, 3.5, def, d) == kSkmGiantServed && d[0] == 0 && d[1] == 0, "budget = one slice each: %u %u", d[0], d[1]);
  CHECK(plan({100000, 20000}, 479999, 3.5, def, d) == kSkmGiantBudget, "one slice each is over the budget");
  kn = def;
  kn.work_pct = 50;
  CHECK(plan({100000, 20000}, 2000000, 3.5, kn, d) == kSkmGiantServed && d[0] == 2 && d[1] == 4, "50 per cent of 2 M: %u %u", d[0], d[1]);
  kn.work_pct = 0;
  CHECK(plan({100000}, big, 3.5, kn, d) == kSkmGiantBudget, "no budget at all");
  // a forced count is honoured: every bin, whatever its size, not halved — it fits or the job is given up
  for (uint64_t s : {1ull, 2ull, 4ull, 64ull, 1024ull}) {
    kn = def;
    kn.slices = s;
    CHECK(plan({100000, 20000, 1025}, big, 3.5, kn, d) == kSkmGiantServed && (1ull << d[0]) == s && d[1] == d[0] && d[2] == d[0], "forced %llu: %u %u %u",
          (unsigned long long)s, d[0], d[1], d[2]);
  }
  kn = def;
  kn.slices = 1024;
  kn.work_pct = 1;
  CHECK(plan({30000}, 200000, 3.5, kn, d) == kSkmGiantBudget, "forced 1024 slices within 1 per cent");
  kn.slices = 3;  // (not a power of two: the next one)
  kn.work_pct = 25;
  CHECK(plan({30000}, big, 3.5, kn, d) == kSkmGiantServed && d[0] == 2, "forced 3: depth %u", d[0]);
  kn.slices = 4;
  kn.max_records = 2000;
  CHECK(plan({30000}, big, 3.5, kn, d) == kSkmGiantCap, "the cap holds for a forced count");
}

int main() {
  check_traversal();
  check_plan();
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("ok\n");
  return 0;
}
