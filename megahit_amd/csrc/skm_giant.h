// Giant bins of the group-by on super-k-mer records in SLICES (s1_skm.hip k_s1_skm / k_count_skm, option s1_skm_giant): the rounds in which
// a workgroup works a bin, and how a bin too large for one workgroup is cut into work items for several.
// Plain C++, host and device: no HIP, no other header of the library (tests/host/skm_giant_check.cpp drives it on the CPU).
//
// A bin is worked in ROUNDS (sub, rj): a round takes the keys whose top `sub` bits of a second 32-bit hash are rj (sub = 0: all keys).  A
// round whose keys overflow the table is BAD and is redone as its two halves (sub + 1, 2 rj) and (sub + 1, 2 rj + 1); a good round is
// complete in itself — nothing is carried from round to round.  So the rounds below (sub0, rj0) are a job of their own: the keys of a bin
// are the disjoint union of the 2^sub0 jobs of depth sub0, and each may go to another workgroup.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MHX_SKMG_HD __host__ __device__ inline
#else
#define MHX_SKMG_HD inline
#endif

namespace mhx {

constexpr int kSkmRoundMaxDepth = 31;    // a bad round at this depth gives the job up
constexpr int kSkmGiantMaxDepth = 10;    // at most 2^10 slices of a bin
constexpr int kSkmGiantMaxBins = 1024;   // giant bins a pass lists

// does the key with second hash `hash32` belong to round (sub, rj)?
MHX_SKMG_HD bool skm_in_round(uint32_t hash32, uint32_t sub, uint32_t rj) { return sub == 0 || (hash32 >> (32 - sub)) == rj; }

// the round behind (sub, rj) of the traversal that started at (sub0, rj0): a bad round goes down to its first half (at kSkmRoundMaxDepth:
// *give_up, and *done); a good one goes to its neighbour and climbs while that is a round already covered by its parent's turn — never
// above sub0.  *done: the climb is back at depth sub0, at (sub0, rj0 + 1).  sub0 = rj0 = 0: a whole bin.
MHX_SKMG_HD void skm_next_round(uint32_t sub, uint32_t rj, bool bad, uint32_t sub0, uint32_t rj0, uint32_t *nsub, uint32_t *nrj, bool *done, bool *give_up) {
  uint32_t s = sub, r = rj;
  bool d = false, g = false;
  if (bad) {
    if (sub >= (uint32_t)kSkmRoundMaxDepth) {
      g = true;
      d = true;
    } else {
      s = sub + 1;
      r = rj << 1;
    }
  } else {
    r = rj + 1;
    while (s > sub0 && (r & 1u) == 0) {
      --s;
      r >>= 1;
    }
    d = s == sub0 && r == rj0 + 1u;
  }
  *nsub = s;
  *nrj = r;
  *done = d;
  *give_up = g;
}

// ---- the plan: how many slices each giant bin gets ----
struct SkmGiantKnobs {
  uint64_t max_records = 1ull << 21;  // s1_skm_giant_max: a bin beyond it gives the job up (measured: DESIGN 4o)
  uint64_t keys = 4096;               // s1_skm_giant_keys: windows a slice should hold (half the table's slots)
  uint64_t work_pct = 25;             // s1_skm_giant_work_pct: records re-read by the slices, in per cent of the job's records
  uint64_t slices = 0;                // s1_skm_giant_slices: 0 automatic, else the slices of every giant bin (a power of two; tests)
};
enum SkmGiantVerdict { kSkmGiantServed = 0, kSkmGiantCap = 1, kSkmGiantBudget = 2, kSkmGiantList = 3 };

MHX_SKMG_HD uint32_t skm_giant_depth_of(uint64_t slices) {  // the smallest depth with 2^depth >= slices, at most kSkmGiantMaxDepth
  uint32_t d = 0;
  while (d < (uint32_t)kSkmGiantMaxDepth && (1ull << d) < slices) ++d;
  return d;
}

// records[g]: the records of giant bin g (g < n_giant); n: the records of the job (of the pass); win_per_rec: its mean windows per record.
// -> the verdict; served: sub0[g] = the depth of bin g (2^sub0[g] slices).
//   wanted      the bin's estimated windows / keys, rounded up to a power of two, at most 2^kSkmGiantMaxDepth (or the forced count)
//   work budget every slice reads the whole bin: sum over g of 2^sub0[g] * records[g] <= n * work_pct / 100 — the costliest bin (slices x
//               records; the first of equals) is halved until the sum fits; all at one slice and still over: kSkmGiantBudget.  A forced
//               count is not halved: it fits or the job is given up
//   cap, list   a bin beyond max_records: kSkmGiantCap; more than kSkmGiantMaxBins bins: kSkmGiantList
inline SkmGiantVerdict skm_giant_plan(const uint64_t *records, int n_giant, uint64_t n, double win_per_rec, const SkmGiantKnobs &kn, uint8_t *sub0) {
  if (n_giant > kSkmGiantMaxBins) return kSkmGiantList;
  for (int g = 0; g < n_giant; ++g)
    if (records[g] > kn.max_records) return kSkmGiantCap;
  const double keys = (double)(kn.keys ? kn.keys : 1);
  const double budget = (double)n * (double)kn.work_pct / 100.0;
  double work = 0.0;
  for (int g = 0; g < n_giant; ++g) {
    uint64_t want = kn.slices;
    if (!want) {
      const double w = (double)records[g] * (win_per_rec > 0.0 ? win_per_rec : 1.0) / keys;
      want = w >= (double)(1u << kSkmGiantMaxDepth) ? (1ull << kSkmGiantMaxDepth) : (uint64_t)w + ((double)(uint64_t)w < w ? 1u : 0u);
    }
    sub0[g] = (uint8_t)skm_giant_depth_of(want);
    work += (double)(1ull << sub0[g]) * (double)records[g];
  }
  while (work > budget) {
    if (kn.slices) return kSkmGiantBudget;
    int at = -1;
    double most = 0.0;
    for (int g = 0; g < n_giant; ++g) {
      const double w = (double)(1ull << sub0[g]) * (double)records[g];
      if (sub0[g] > 0 && w > most) {
        most = w;
        at = g;
      }
    }
    if (at < 0) return kSkmGiantBudget;
    --sub0[at];
    work -= most / 2.0;
  }
  return kSkmGiantServed;
}

}  // namespace mhx
