// read2sdbg stage 1 — and `count` — on super-k-mer records (round 6).  The no-mercy reduction of Read2SdbgS1 (reference
// src/sorting/read_to_sdbg_s1.cpp:208-366 makes one sort item per (k-1)-mer window of every read, :368-464 counts the groups of equal items)
// needs the (k+1)-mers GROUPED, not sorted: is_solid, the multiplicity histogram and the aggregated stage-2 items are functions of the
// multiset of canonical (k+1)-mers; the same holds for KmerCounter (src/sorting/kmer_counter.cpp:158-381), whose edges are ordered afterwards.
// So the grouping key need not be a prefix of the k-mer.  Here it is the MINIMIZER of the (k+1)-mer — the smallest hash of a canonical
// m-mer inside it — which consecutive windows of a read share: a run of windows with one minimizer (a "super-k-mer") leaves the read as
// ONE 16-byte record (its bases, where it starts, how many windows it holds) instead of one 12-byte record per window.
//   k_skm_make    one thread per aligned block of 8 windows: 17 canonical m-mer hashes from one 64-bit window of the store and its
//                 reverse complement, the 8 window minima by a suffix / prefix scan, a record per run of equal bins (3.5 windows per
//                 record at k = 21) -> the record array, SPLIT by the low digit of the bin: 256 ranges, a record goes into the range of its
//                 digit (per workgroup and trip one reservation per digit, the records ordered by digit in an LDS stage before they
//                 leave) — the group-by needs the records grouped by bin, in no order inside a bin, so the first sort pass need not be a
//                 pass over an array this kernel has just written; the digit histograms of the sort passes on the way; windows of ONE
//                 base (poly-A, poly-G) counted beside the records — REP (s1_skm_rep): all windows of period <= 4, per entry of a table
//                 of 320, made into keys by k_skm_rep_publish / k_count_rep_publish; COUNT: a base more either side.  (s1_skm_split = 0, a bin of one
//                 digit, or a range that overflowed — skewed bins: the record array through one cursor, one atomic per workgroup and trip)
//   radix_sort    ONE pass over the high digit of the 16-bit bin, reading the ranges in order (sort_kernels.h SrcSplit; stable, so its
//                 output is ordered by the whole bin); a second beyond 2^16 bins; all digits when the records were not split
//   k_skm_bounds  where each bin starts
//   k_s1_skm      one workgroup per bin at a time: the windows of a wavefront's 64 records (~225) are dealt to the lanes 64 at a time (a bitmap
//                 of run heads, six shuffles per window), canonical key (read_to_sdbg_s1.cpp:228-292: the strand of the (k-1)-mer, then
//                 head / tail), LDS table with 64-bit keys, one walk over the table for the histogram (:430-436), the marks of the
//                 non-solid occurrences (:464, inverted: a key of count 1 < m has one record, whose position sits next to the key) and the
//                 aggregated stage-2 items; several sources per bin (several GPUs: one per sending rank) and the marks as a list there
//   k_count_skm   the same for `count`: in / out characters in the slot, packed edges out, the windows of flagged keys in a second expansion
//                 (EVENTS, several GPUs: those windows leave as a list of events for the ranks that hold the reads)
// 6.0 GB of records at 10 M reads instead of 16: the sort and the read of the group-by move 2.7 x fewer bytes.
// Shapes: no mercy, no lv1 bucket filter (the path cuts large jobs into passes over ranges of its OWN bins), reads of one length or of
// several, min count <= 2 (one GPU, s1_skm_max_m: 3 and 4 — the LOOK form of k_s1_skm, the LV 4 form of k_count_skm), 19 <= k <= 22 (count: 21), positions below 2^36; everything else — and any input with a bin that outgrows what
// one workgroup should stream (repeats other than homopolymers; with s1_skm_rep: other than reads of period <= 4 throughout) — takes the
// prefix plan (s1_stream.hip).  With s1_skm_giant (one GPU) such a bin, up to s1_skm_giant_max records, is listed by k_skm_giants and worked
// in SLICES: the rounds of the bin from a depth on are work items of their own, tickets in front of the batches of bins (skm_giant.h; the
// GIANT forms of k_s1_skm / k_count_skm).  DESIGN.md 4o.
#include <cstring>

#include "s1_shared.h"
#include "skm_deal.h"
#include "skm_giant.h"

namespace mhx {

constexpr int kSkmC = 8;                     // windows per aligned block = the longest run a record holds
constexpr int kSkmW = 10;                    // m-mers per window: m = k + 1 - 9
constexpr int kSkmNM = kSkmC + kSkmW - 1;    // m-mers a block looks at
constexpr int kSkmMinBinBits = 16, kSkmMaxBinBits = 20;  // two sort passes, or three

__device__ __forceinline__ uint32_t skm_mix(uint32_t c) {  // (a bijection of 32 bits: the order of the m-mers)
  uint32_t h = c * 0x9E3779B1u;
  return h ^ (h >> 15);
}
__device__ __forceinline__ uint32_t skm_mix2(uint32_t c) {  // (the second hash of a table key: which half of a bin that overflowed it belongs to)
  uint32_t h = c * 0x9E3779B1u;
  h ^= h >> 15;
  return h * 0x85EBCA6Bu;
}
__device__ __forceinline__ uint32_t skm_bin_of(uint32_t minh) {  // (the minimum of ten hashes is small: mixed once more; the bin = its top bits)
  return (minh ^ (minh >> 16)) * 0x7FEB352Du;
}

// record (16 bytes): w0 = position bits 32.. << 28 | bin << 8 (bits 0..7 zero: the sort passes may rank with LDS atomics, sort_kernels.h
// RANK 2), w1:w2 = the bases of the run, MSB first (k + windows of them: at most 30 at k <= 22) with windows - 1 in the three lowest bits,
// w3 = position of the run's first base in the store, low 32 bits.
// VAR: reads of several lengths — every read gets bpr = ceil((max_len - k) / 8) blocks, its place in the store comes from start[]
// (as the padded item slots of S1GenVarT); a block beyond the read's last window makes nothing.
// COUNT: the records of `count` (KmerCounter, kmer_counter.cpp:158-381) — a window's key is the canonical (k+1)-mer and the table wants the base
// in front of it and the base behind it: the record carries one more base either side of its run (k + windows + 2 <= 31 bases at k <= 21),
// two flags for a run that starts at the first / ends at the last window of its read ('$' there), and its length in the first word:
// w0 = position bits 32.. << 28 | bin << 8 | (windows - 1) << 5 | no_prev << 4 | no_next << 3.
// SPLIT: the record array is 256 ranges of range_cap slots, one per value of the bin's LOW digit, and a record goes into the range of its
// digit, in any order — the first sort pass done where the records are made (the group-by wants the records grouped by bin, nothing more;
// the next pass reads the ranges in order, sort_kernels.h SrcSplit, and is stable: its output is ordered by the whole bin).  Per trip of a
// workgroup: the records counted per digit in LDS, ONE reservation per digit that has any on the 256 cursors split_cur[] (thread d for
// digit d), the records placed into an LDS stage ordered by digit (one returning LDS atomic each), the stage copied out: the records of a
// digit leave as one run.  A trip with more records than the stage holds (stage_n; uniform) writes them from the registers to the places
// reserved.  A reservation beyond its range writes nothing and raises bit 1 of *err: the host makes the records again without the split.
constexpr int kSkmStage = 2560;  // records the stage holds: a trip of 512 x 2 blocks makes 2330 of random sequence (0.284 per window)
// REP (s1_skm_rep): windows of PERIOD <= 4 — (AC)n, (AAG)n, (AGAT)n microsatellites, and the homopolymers with them — never enter a record.
// A (k+1)-mer of period p is its first p bases repeated; one of 20 bases and more with periods 3 and 4 has period 1 (Fine and Wilf).  So a
// window whose period divides 4 is named by its first FOUR bases (entries 0..255) and one of period 3 that is no homopolymer by its first
// THREE (entries 256..319): kSkmRepN direct-indexed entries behind hp[] — stage 1: [e] windows, [kSkmRepN + e] the smallest position of one;
// count: [9 e] windows, [9 e + 1 + x] base x in front, [9 e + 5 + x] base x behind, in the READ's orientation ('$' untallied) — which
// k_skm_rep_publish / k_count_rep_publish turn into keys.  A workgroup tallies the entries it meets in a small LDS hash (a library's
// repeat-throughout reads fall into a handful: (AC)n reads into ACAC and CACA, their other strand into GTGT and TGTG) and adds it to the
// global table ONCE, at its end.  The hash has what LDS is left beside the 81 032 bytes of the SPLIT form while two workgroups share a CU's
// 160 KB: 48 slots of 16 bytes in stage 1, 16 slots of 40 bytes in the count form; an entry's slot is one of the kSkmRepProbes behind its
// hash value.  An entry that finds none goes to the global table from the registers: the lanes of a wavefront that hold the same entry
// (count: and the same bases either side) send ONE add between them — neighbouring lanes hold neighbouring blocks of the same reads.
constexpr int kSkmRepN = 320, kSkmRepAt = 64;  // (the table starts kSkmRepAt values behind hp)
constexpr int kSkmRepSlotsS1 = 48, kSkmRepSlotsCount = 16, kSkmRepProbes = 8;
template <int NT, int J, bool VAR, bool COUNT = false, bool SPLIT = false, bool REP = false>
__global__ __launch_bounds__(NT) void k_skm_make(const uint32_t *__restrict__ seq, const uint64_t *__restrict__ start, uint32_t L, uint32_t bpr, uint64_t n_blocks,
                                                 int k, int bin_bits, uint32_t bin_lo, uint32_t bin_hi, int count_items, uint64_t pos_base,
                                                 unsigned long long *__restrict__ hp, uint4 *__restrict__ out, unsigned long long cap,
                                                 unsigned long long *__restrict__ cursor, uint32_t *__restrict__ err, unsigned long long *__restrict__ digit_hist,
                                                 unsigned long long range_cap, unsigned long long *__restrict__ split_cur, uint32_t stage_n) {
  constexpr long long kNoRoom = -0x7FFFFFFFFFFFFFFFll - 1;
  __shared__ uint32_t sm_scan[NT / kWave + 1];
  __shared__ uint4 stage[SPLIT ? kSkmStage : 1];
  __shared__ uint32_t dcnt[SPLIT ? 256 : 1], dpos[SPLIT ? 256 : 1];  // per low digit: the trip's records, where the next one goes in the stage
  __shared__ long long goff[SPLIT ? 256 : 1];                        // ... its place in the array minus its place in the stage (kNoRoom: dropped)
  __shared__ unsigned long long s_base;
  __shared__ uint32_t dh[3][256];  // the digit histograms of the sort passes, taken while the records are made
  __shared__ uint32_t lbin[J * kSkmC][NT];  // a thread's bins, read back by window number when its records leave (no register array indexed by a variable)
  __shared__ uint32_t hpl[2][12];  // COUNT: the homopolymer windows of this workgroup per class: [0] windows, [1 + x] base x in front, [5 + x] base x behind
  constexpr int kSkmRepSlots = COUNT ? kSkmRepSlotsCount : kSkmRepSlotsS1;
  __shared__ uint32_t rid[REP ? kSkmRepSlots : 1];                    // REP: the entry a slot holds (kSkmRepN: none yet)
  __shared__ uint32_t rtl[REP ? kSkmRepSlots : 1][COUNT ? 9 : 1];     // ... its windows (count: and the bases in front and behind)
  __shared__ unsigned long long rps[REP && !COUNT ? kSkmRepSlots : 1];  // ... the smallest position of one (stage 1)
  const int tid = threadIdx.x;
  if constexpr (REP) {
    if (tid < kSkmRepSlots) {
      rid[tid] = (uint32_t)kSkmRepN;
      if constexpr (!COUNT) rps[tid] = ~0ull;
    }
    if (tid < kSkmRepSlots * (COUNT ? 9 : 1)) rtl[tid / (COUNT ? 9 : 1)][tid % (COUNT ? 9 : 1)] = 0;
  }
  if (tid < 24) hpl[tid / 12][tid % 12] = 0;
  for (int i = tid; i < 768; i += NT) dh[i >> 8][i & 255] = 0;
  if (SPLIT && tid < 256) dcnt[tid] = 0;
  __syncthreads();
  const bool third_digit = bin_bits > 16;
  const int M = k + 1 - (kSkmW - 1);
  const uint32_t mmask = (1u << (2 * M)) - 1u;
  const int K1 = k + 1;
  const unsigned bin_sh = 32u - (unsigned)bin_bits;
  unsigned long long items = 0;  // VAR: what the reference sorts, L - k + 4 items per read that holds an edge (read_to_sdbg_s1.cpp:344-363)
  // HOMOPOLYMER windows — (k+1)-mers of one base: poly-A tails, the poly-G of a two-colour instrument's dark cycles — share ONE key by the
  // million and would all sit behind one minimizer in one bin.  They never enter a record: a window of one base is counted here (hp != null,
  // first pass only: hp[0] / hp[1] = windows of A or T / of C or G, hp[2] / hp[3] = the smallest position of one, should it be the only one)
  // and published as the one or two keys they are by k_skm_hp_publish.
  uint32_t hp_n[2] = {0, 0};
  unsigned long long hp_p[2] = {~0ull, ~0ull};
  // Which read a block belongs to and which of its blocks it is — b / bpr, b % bpr — is divided out ONCE per thread: from trip to trip b
  // grows by gridDim.x * NT * J, from one block of a thread to its next by NT, so quotient and remainder move by those steps' own
  // (uniform) quotients and remainders and one carry (a 64-bit division per block was a quarter of the kernel's vector instructions)
  const uint64_t step_trip = (uint64_t)gridDim.x * (uint64_t)(NT * J);
  const uint64_t trip_r = step_trip / bpr;
  const uint32_t trip_q = (uint32_t)(step_trip - trip_r * bpr), next_r = (uint32_t)NT / bpr, next_q = (uint32_t)NT % bpr;
  uint64_t blk_r = ((uint64_t)blockIdx.x * (uint64_t)(NT * J) + tid) / bpr;  // of the thread's first block of the trip
  uint32_t blk_q = (uint32_t)((uint64_t)blockIdx.x * (uint64_t)(NT * J) + tid - blk_r * bpr);
  // The words of the store a trip's blocks look at are asked for TOGETHER at the head of the trip: the J loads of a thread are in flight
  // at once instead of one after the other, each waited for before the next block's address is worked out (a block beyond its read's
  // last window: fq0 = fnwin = 0)
  uint64_t fa[J];
  uint32_t fq0[J], fnwin[J], fc[J][COUNT ? 4 : 3];
  // REP: one window of entry e (count: bases pv in front, nx behind, 4 = none; stage 1: at position p) -> its slot of the LDS hash, claimed
  // with a compare-and-swap on the first meeting; none among its kSkmRepProbes places: the global table
  [[maybe_unused]] auto rep_tally = [&](uint32_t e, unsigned pv, unsigned nx, uint64_t p) {
    if constexpr (REP) {
      unsigned long long *const tab = hp + kSkmRepAt;
      // (hp[kSkmRepAt - 1]: the slots in use — all of them; s1_skm_rep_slots, tests: fewer, or none)
      const uint32_t n_slots = min((uint32_t)hp[kSkmRepAt - 1], (uint32_t)kSkmRepSlots);
      uint32_t h = n_slots ? (e ^ (e >> 4) ^ (e >> 6)) % n_slots : 0u;
      int slot = -1;
      for (int n = 0; n < kSkmRepProbes && n_slots; ++n) {
        const uint32_t old = atomicCAS(&rid[h], (uint32_t)kSkmRepN, e);
        if (old == (uint32_t)kSkmRepN || old == e) {
          slot = (int)h;
          break;
        }
        h = h + 1 == n_slots ? 0u : h + 1;
      }
      if (slot >= 0) {
        atomicAdd(&rtl[slot][0], 1u);
        if constexpr (COUNT) {
          if (pv < 4) atomicAdd(&rtl[slot][1 + pv], 1u);
          if (nx < 4) atomicAdd(&rtl[slot][5 + nx], 1u);
        } else {
          atomicMin(&rps[slot], (unsigned long long)p);
        }
      } else {
        // the lanes that are here with one entry (count: and the same bases either side) take turns, entry by entry; the first of them adds for all
        const uint32_t sig = COUNT ? e | ((uint32_t)pv << 9) | ((uint32_t)nx << 12) : e;
        for (;;) {
          const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)sig);
          const unsigned long long together = __ballot(sig == s0);  // (asked by every lane still in the loop: the vote names exactly the lanes of this turn)
          if (sig == s0) {
            if ((tid & (kWave - 1)) == __builtin_ctzll(together)) {
              const unsigned long long n = (unsigned long long)__builtin_popcountll(together);
              if constexpr (COUNT) {
                atomicAdd(tab + 9 * e, n);
                if (pv < 4) atomicAdd(tab + 9 * e + 1 + pv, n);
                if (nx < 4) atomicAdd(tab + 9 * e + 5 + nx, n);
              } else {
                atomicAdd(tab + e, n);
              }
            }
            break;
          }
        }
        if constexpr (!COUNT) {  // (the smallest position settles early — positions grow with the trips — and is then only read)
          unsigned long long *const at = tab + kSkmRepN + e;
          if ((unsigned long long)p < __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(at, (unsigned long long)p);
        }
      }
    }
  };
  auto fetch = [&](uint64_t it2) {  // (called once per trip, in the order of the trips)
    uint64_t r = blk_r;
    uint32_t q = blk_q;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const uint64_t b = it2 * (uint64_t)(NT * J) + (uint64_t)j * NT + tid;
      fa[j] = 0;
      fq0[j] = 0;
      fnwin[j] = 0;
      if (j > 0) {
        r += next_r;
        q += next_q;
        if (q >= bpr) {
          q -= bpr;
          ++r;
        }
      }
      if (b < n_blocks) {
        const uint32_t q0 = q * kSkmC;
        uint64_t base;
        uint32_t nwin;
        if constexpr (VAR) {
          base = start[r];
          const uint64_t len_r = start[r + 1] - base;
          nwin = len_r >= (uint64_t)K1 ? (uint32_t)(len_r - k) : 0u;
          if (q0 == 0 && nwin && count_items) items += nwin + (COUNT ? 0 : 4);  // (count: one item per window, kmer_counter.cpp:158-206)
        } else {
          base = r * L;
          nwin = L - k;
        }
        if (q0 < nwin) {
          fa[j] = base + q0;
          fq0[j] = q0;
          fnwin[j] = nwin;
        }
      }
      // (no branch around the loads — the words of all J blocks are asked for before the first is waited for; a block without windows
      //  looks at the first words of the store, which a job on this path has)
      const uint64_t wi = fa[j] >> 4;
      fc[j][0] = seq[wi];
      fc[j][1] = seq[wi + 1];
      fc[j][2] = seq[wi + 2];
      if constexpr (COUNT) fc[j][3] = seq[(fa[j] > 0 ? fa[j] - 1 : 0) >> 4];  // (the word of the base in front of the block)
    }
    blk_r += trip_r;
    blk_q += trip_q;
    if (blk_q >= bpr) {
      blk_q -= bpr;
      ++blk_r;
    }
  };
  for (uint64_t it = blockIdx.x; it * (uint64_t)(NT * J) < n_blocks; it += gridDim.x) {
    uint64_t Wv[J], pos0[J];
    uint32_t smask[J], emask[J];  // per block: the windows that start a run of this pass's bins, and those that end one
    uint32_t bflag[J];            // COUNT: bit 0 the block's first window is its read's first, bit 1 its last window is the read's last, bits 2.. its windows
    fetch(it);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      smask[j] = 0;
      emask[j] = 0;
      bflag[j] = 0;
      Wv[j] = 0;
      pos0[j] = 0;
      {
        const uint32_t q0 = fq0[j], nwin = fnwin[j];
        if (q0 < nwin) {
          const uint64_t a = fa[j];
          const unsigned sh = (unsigned)(a & 15) * 2;
          const uint32_t c0 = fc[j][0], c1 = fc[j][1], c2 = fc[j][2];
          const uint64_t W = ((uint64_t)funnel_l(c0, c1, sh) << 32) | funnel_l(c1, c2, sh);
          const uint64_t R = rc64(W, 32);
          uint32_t h[kSkmNM];
#pragma unroll
          for (int i = 0; i < kSkmNM; ++i) {
            const uint32_t f = (uint32_t)(W >> (64 - 2 * (i + M))) & mmask;
            const uint32_t rv = (uint32_t)(R >> (2 * i)) & mmask;
            h[i] = skm_mix(min(f, rv));
          }
          // window j: the minimum of h[j .. j + 9] = min(suffix minimum inside h[0..9], prefix minimum inside h[10..16])
          uint32_t sfx[kSkmW];
          sfx[kSkmW - 1] = h[kSkmW - 1];
#pragma unroll
          for (int i = kSkmW - 2; i >= 0; --i) sfx[i] = min(h[i], sfx[i + 1]);
          uint32_t pfx = 0xFFFFFFFFu;
          uint32_t bins[kSkmC];
          bins[0] = skm_bin_of(sfx[0]) >> bin_sh;
#pragma unroll
          for (int w = 1; w < kSkmC; ++w) {
            pfx = min(pfx, h[kSkmW - 1 + w]);
            bins[w] = skm_bin_of(min(sfx[w], pfx)) >> bin_sh;
          }
#pragma unroll
          for (int w = 0; w < kSkmC; ++w) lbin[j * kSkmC + w][tid] = bins[w];
          // a pass of the memory plan keeps the bins [bin_lo, bin_hi): the windows of a run share their bin, so runs stay whole
          const uint32_t n_here = min((uint32_t)kSkmC, nwin - q0);
          uint32_t km = 0, sm = 0, hm = 0;
          if constexpr (REP) {
            // window w has period p when base i equals base i + p for i = w .. w + K1 - p - 1.  Periods 1 and 2 imply 4: only 4 and 3 are
            // looked for, each behind the test on the pairs that lie in EVERY window of the block (i = kSkmC - 1 .. K1 - 1 - p): a block of
            // random sequence looks at no window
            const uint64_t d4 = W ^ (W << 8), d3 = W ^ (W << 6);
            uint32_t m4 = 0, m3 = 0;
            if ((d4 & ((~0ull >> (2 * (kSkmC - 1))) & (~0ull << (64 - 2 * (K1 - 4))))) == 0) {
#pragma unroll
              for (int w = 0; w < kSkmC; ++w)
                if ((uint32_t)w < n_here && ((d4 << (2 * w)) >> (64 - 2 * (K1 - 4))) == 0) m4 |= 1u << w;
            }
            if ((d3 & ((~0ull >> (2 * (kSkmC - 1))) & (~0ull << (64 - 2 * (K1 - 3))))) == 0) {
#pragma unroll
              for (int w = 0; w < kSkmC; ++w)
                if ((uint32_t)w < n_here && ((d3 << (2 * w)) >> (64 - 2 * (K1 - 3))) == 0) m3 |= 1u << w;
            }
            hm = m4 | m3;
            if (hm && count_items) {
#pragma unroll
              for (int w = 0; w < kSkmC; ++w)
                if ((hm >> w) & 1u) {
                  // (periods 3 and 4 together: a homopolymer, named by its four bases)
                  const uint32_t e = (m4 >> w) & 1u ? (uint32_t)(W >> (56 - 2 * w)) & 255u : 256u + ((uint32_t)(W >> (58 - 2 * w)) & 63u);
                  unsigned prev_raw = 4, next_raw = 4;
                  if constexpr (COUNT) {
                    prev_raw = q0 + w == 0 ? kSentinel
                                           : (w == 0 ? (unsigned)((fc[j][COUNT ? 3 : 0] >> (30 - 2 * (unsigned)((a - 1) & 15))) & 3u) : (unsigned)(W >> (64 - 2 * w)) & 3u);
                    next_raw = q0 + w + 1 == nwin ? kSentinel : (unsigned)(W >> (62 - 2 * (w + K1))) & 3u;
                  }
                  rep_tally(e, prev_raw, next_raw, pos_base + a + (uint64_t)w);
                }
            }
          } else if (hp) {  // (uniform) windows of one base: adjacent bases equal all along the window
            const uint64_t dx = W ^ (W << 2);  // base i differs from base i + 1: bits 63 - 2i, 62 - 2i
            // (the bases kSkmC - 1 .. K1 - 1 lie in every window of the block: unless they are all equal, which is rare, no window is looked at)
            if ((dx & ((~0ull >> (2 * (kSkmC - 1))) & (~0ull << (64 - 2 * (K1 - 1))))) == 0) {
#pragma unroll
              for (int w = 0; w < kSkmC; ++w)
                if ((uint32_t)w < n_here && ((dx << (2 * w)) >> (64 - 2 * (K1 - 1))) == 0) hm |= 1u << w;
            }
            if (hm && count_items) {
#pragma unroll
              for (int w = 0; w < kSkmC; ++w)
                if ((hm >> w) & 1u) {
                  const unsigned b = (unsigned)(W >> (62 - 2 * w)) & 3u;
                  const unsigned cls = b == 0 || b == 3 ? 0u : 1u;
                  if constexpr (COUNT) {
                    // count: the key is A...A (C...C); a window of T (G) is its reverse complement (strand 1: the bases either side swap and complement)
                    const bool strand = b >= 2;
                    const unsigned prev_raw = q0 + w == 0 ? kSentinel
                                              : (w == 0 ? (unsigned)((fc[j][COUNT ? 3 : 0] >> (30 - 2 * (unsigned)((a - 1) & 15))) & 3u) : (unsigned)(W >> (64 - 2 * w)) & 3u);
                    const unsigned next_raw = q0 + w + 1 == nwin ? kSentinel : (unsigned)(W >> (62 - 2 * (w + K1))) & 3u;
                    const unsigned pv = strand ? comp_or_sentinel(next_raw) : prev_raw, nx = strand ? comp_or_sentinel(prev_raw) : next_raw;
                    atomicAdd(&hpl[cls][0], 1u);
                    if (pv < 4) atomicAdd(&hpl[cls][1 + pv], 1u);
                    if (nx < 4) atomicAdd(&hpl[cls][5 + nx], 1u);
                  } else {
                    ++hp_n[cls];
                    hp_p[cls] = min(hp_p[cls], pos_base + a + (uint64_t)w);
                  }
                }
            }
          }
#pragma unroll
          for (int w = 0; w < kSkmC; ++w)
            if ((uint32_t)w < n_here && !((hm >> w) & 1u) && bins[w] >= bin_lo && bins[w] < bin_hi) km |= 1u << w;
#pragma unroll
          for (int w = 0; w < kSkmC; ++w)
            if (((km >> w) & 1u) && (w == 0 || !((km >> (w - 1)) & 1u) || bins[w] != bins[w > 0 ? w - 1 : 0])) sm |= 1u << w;
          smask[j] = sm;
          emask[j] = km & ((sm >> 1) | ~(km >> 1));  // window w ends a run: the next one starts one, or is not this pass's (bit 8 of km is clear)
          if constexpr (COUNT) {  // the window that starts one base earlier: the base in front of the block's first window, then 31 bases
            const uint64_t pb = a > 0 ? (uint64_t)((fc[j][COUNT ? 3 : 0] >> (30 - 2 * (unsigned)((a - 1) & 15))) & 3u) : 0ull;
            Wv[j] = (W >> 2) | (pb << 62);
            bflag[j] = (q0 == 0 ? 1u : 0u) | (q0 + n_here == nwin ? 2u : 0u) | (n_here << 2);
          } else {
            Wv[j] = W;
          }
          pos0[j] = pos_base + a;  // (several GPUs: this rank's reads start at pos_base of the global read set)
        }
      }
    }
    // the record of the run of windows rs .. re of block j; the runs of this thread, in order
    auto rec_of = [&](int j, int rs, int re, uint32_t run_bin) -> uint4 {
      const int len = re - rs + 1;
      const uint64_t p = pos0[j] + (uint64_t)rs;
      if constexpr (COUNT) {
        const uint64_t bases = (Wv[j] << (2 * rs)) & (~0ull << (64 - 2 * (K1 + len + 1)));
        const uint32_t n_blk = bflag[j] >> 2;
        const uint32_t fl = ((bflag[j] & 1u) && rs == 0 ? 16u : 0u) | ((bflag[j] & 2u) && (uint32_t)(re + 1) == n_blk ? 8u : 0u);
        return make_uint4((run_bin << 8) | ((uint32_t)(p >> 32) << 28) | ((uint32_t)(len - 1) << 5) | fl, (uint32_t)(bases >> 32), (uint32_t)bases, (uint32_t)p);
      } else {
        const uint64_t bases = ((Wv[j] << (2 * rs)) & (~0ull << (64 - 2 * (K1 + len - 1)))) | (uint64_t)(len - 1);
        return make_uint4((run_bin << 8) | ((uint32_t)(p >> 32) << 28), (uint32_t)(bases >> 32), (uint32_t)bases, (uint32_t)p);
      }
    };
    auto walk = [&](auto &&fn) {
#pragma unroll
      for (int j = 0; j < J; ++j) {
        uint32_t sm = smask[j], em = emask[j];
        while (sm) {  // (runs are disjoint and in order: the i-th start goes with the i-th end)
          const int rs = __builtin_ctz(sm), re = __builtin_ctz(em);
          sm &= sm - 1;
          em &= em - 1;
          fn(j, rs, re, lbin[j * kSkmC + rs][tid]);
        }
      }
    };
    if constexpr (SPLIT) {
      walk([&](int, int, int, uint32_t run_bin) {
        atomicAdd(&dcnt[run_bin & 255u], 1u);
        atomicAdd(&dh[1][(run_bin >> 8) & 255u], 1u);
        if (third_digit) atomicAdd(&dh[2][run_bin >> 16], 1u);
      });
      __syncthreads();
      // where each digit starts in the stage: a scan over the 256 counts by the first four wavefronts (one barrier; sm_scan is written
      // again behind the next trip's first barrier)
      const uint32_t c = tid < 256 ? dcnt[tid] : 0u;
      const uint32_t inc = wave_inclusive_sum(c);
      if (tid < 256 && (tid & (kWave - 1)) == kWave - 1) sm_scan[tid / kWave] = inc;
      __syncthreads();
      uint32_t total = 0, start = inc - c;
#pragma unroll
      for (int i = 0; i < 256 / kWave; ++i) {
        const uint32_t t = sm_scan[i];
        if (i < tid / kWave) start += t;
        total += t;
      }
      if (tid < 256) {
        long long off = kNoRoom;
        if (c) {
          const unsigned long long gb = atomicAdd(&split_cur[tid], (unsigned long long)c);
          if (gb + c <= range_cap) off = (long long)((unsigned long long)tid * range_cap + gb) - (long long)start;
          else atomicOr(err, 2u);  // (the kernel runs on to its end: the barriers below are met by all, and nothing is stored for this digit)
          dh[0][tid] += c;
        }
        goff[tid] = off;
        dpos[tid] = start;
        dcnt[tid] = 0;
      }
      __syncthreads();
      const bool direct = total > stage_n;  // (uniform)
      walk([&](int j, int rs, int re, uint32_t run_bin) {
        const uint32_t d = run_bin & 255u;
        const uint32_t pos = atomicAdd(&dpos[d], 1u);
        const uint4 rec = rec_of(j, rs, re, run_bin);
        if (direct) {
          const long long off = goff[d];
          if (off != kNoRoom) out[off + (long long)pos] = rec;
        } else {
          stage[pos] = rec;
        }
      });
      if (!direct) {
        __syncthreads();
        for (uint32_t i = tid; i < total; i += NT) {
          const uint4 rec = stage[i];
          const long long off = goff[(rec.x >> 8) & 255u];
          if (off != kNoRoom) out[off + (long long)i] = rec;
        }
      }
      // (no barrier here: the next trip counts into dcnt, which thread d cleared before the barrier above, and writes goff, dpos and the
      //  stage behind its own barriers — by then every thread has left this copy)
    } else {
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < J; ++j) cnt += (uint32_t)__builtin_popcount(smask[j]);
    uint32_t total = 0;
    const uint32_t excl = block_exclusive_sum<uint32_t, NT>(cnt, sm_scan, &total);
    if (tid == 0) s_base = total ? atomicAdd(cursor, (unsigned long long)total) : 0ull;
    __syncthreads();
    const unsigned long long base = s_base;
    if (base + total > cap) {  // (uniform) more records than the array was sized for: the host takes the prefix plan
      if (tid == 0) atomicOr(err, 1u);
      return;
    }
    unsigned long long at = base + excl;
    walk([&](int j, int rs, int re, uint32_t run_bin) {
      out[at++] = rec_of(j, rs, re, run_bin);
      atomicAdd(&dh[0][run_bin & 255u], 1u);
      atomicAdd(&dh[1][(run_bin >> 8) & 255u], 1u);
      if (third_digit) atomicAdd(&dh[2][run_bin >> 16], 1u);
    });
    }
  }
  if constexpr (VAR) {
    items = wave_sum(items);
    if ((tid & (kWave - 1)) == 0 && items) atomicAdd(cursor + 3, items);
  }
  if constexpr (REP) {  // the workgroup's entries -> the global table, once
    __syncthreads();
    constexpr int NV = COUNT ? 9 : 1;
    if (count_items && tid < kSkmRepSlots * NV) {
      const uint32_t e = rid[tid / NV], v = rtl[tid / NV][tid % NV];
      if (e < (uint32_t)kSkmRepN && v) atomicAdd(hp + kSkmRepAt + (COUNT ? 9 * e + (uint32_t)(tid % NV) : e), (unsigned long long)v);
      if constexpr (!COUNT)
        if (e < (uint32_t)kSkmRepN && v) atomicMin(hp + kSkmRepAt + kSkmRepN + e, rps[tid]);
    }
  }
  if constexpr (COUNT) {
    __syncthreads();
    if (hp && count_items && tid < 24 && hpl[tid / 12][tid % 12]) atomicAdd(hp + 8 + (tid / 12) * 16 + (tid % 12), (unsigned long long)hpl[tid / 12][tid % 12]);
  }
  if (!COUNT && !REP && hp && count_items) {
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      const uint32_t n_w = wave_sum(hp_n[x]);
      if (n_w) {  // (uniform per wavefront)
        unsigned long long pmin = hp_p[x];
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) pmin = min(pmin, (unsigned long long)__shfl_xor((long long)pmin, d, kWave));
        if ((tid & (kWave - 1)) == 0) {
          atomicAdd(hp + x, (unsigned long long)n_w);
          atomicMin(hp + 2 + x, pmin);
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < 768; i += NT)
    if (dh[i >> 8][i & 255]) atomicAdd(&digit_hist[i], (unsigned long long)dh[i >> 8][i & 255]);
}

// ---- the keys of the group-bys, shared with the publish kernels of the windows counted beside the records ----
// stage 1 (read_to_sdbg_s1.cpp:228-292): the strand of the (k-1)-mer — f forward, rc its reverse complement —, then head / tail
__device__ __forceinline__ unsigned long long skm_s1_key(uint64_t f, uint64_t rc, unsigned head, unsigned tail) {
  const bool rev = f > rc || (f == rc && head > 3u - tail);
  const uint64_t kf = f | ((uint64_t)head << 3) | tail, kr = rc | ((uint64_t)(3u - tail) << 3) | (3u - head);
  return rev ? kr : kf;
}
// count (kmer_counter.cpp:179): the smaller of the (k+1)-mer and its reverse complement; *strand: the key is the reverse complement
__device__ __forceinline__ unsigned long long skm_count_key(uint64_t x, uint64_t rcx, bool *strand) {
  *strand = rcx < x;  // rev_edge.cmp(edge) < 0
  return *strand ? rcx : x;
}
// the (k+1)-mer head.S.tail of a stage-1 key, MSB first, and the aggregated stage-2 item of a (k+1)-mer with multiplicity mul
__device__ __forceinline__ uint64_t skm_s1_key_kmer(unsigned long long key, int k, uint64_t kmask) {
  return ((uint64_t)((key >> 3) & 7u) << 62) | ((key & kmask) >> 2) | ((uint64_t)(key & 7u) << (62 - 2 * k));
}
__device__ __forceinline__ uint64_t skm_s2_item(uint64_t x, int k, uint64_t mul) {
  return ((x << 2) & (~0ull << (64 - 2 * k))) | (1ull << 19) | ((x >> 62) << 16) | mul;
}

// the (k+1)-mer of period <= 4 that entry e of the REP table names (k_skm_make): its first four (e < 256) or three bases repeated, MSB first
__device__ __forceinline__ uint64_t skm_rep_window(uint32_t e, int K1) {
  const int p = e < 256u ? 4 : 3;
  const uint64_t unit = e < 256u ? (uint64_t)e << 56 : (uint64_t)(e - 256u) << 58;
  uint64_t x = 0;
  for (int i = 0; i < 32; i += p) x |= unit >> (2 * i);
  return x & (~0ull << (64 - 2 * K1));
}

// REP, stage 1: the at most kSkmRepN entries -> keys (distinct entries may give ONE key: a window and its reverse complement; the key
// expression decides, its tie rule included) -> per key what the walk over the table does: histogram, the mark at the only window of a key
// of count 1 < m, else the aggregated stage-2 items.  One workgroup.  res[0] = the windows counted beside the records, res[1] = the keys
__global__ __launch_bounds__(kSkmRepN) void k_skm_rep_publish(const unsigned long long *__restrict__ tab, int k, uint32_t m, uint8_t *__restrict__ solid_bytes,
                                                              unsigned long long *__restrict__ hist, uint2 *__restrict__ agg_items, unsigned long long *__restrict__ agg_cursor,
                                                              int agg, DigitSpecs agg_specs, unsigned long long *__restrict__ agg_hist, unsigned long long *__restrict__ res) {
  __shared__ unsigned long long s_key[kSkmRepN], s_cnt[kSkmRepN], s_pos[kSkmRepN];
  __shared__ unsigned long long s_tot[2];
  const int e = threadIdx.x, K1 = k + 1;
  const uint64_t kmask = ~0ull << (64 - 2 * (k - 1));
  if (e < 2) s_tot[e] = 0;
  {
    const uint64_t win = skm_rep_window((uint32_t)e, K1);
    const uint64_t f = (win << 2) & kmask, rc = (rc64(win, 32) << (2 * (32 - k))) & kmask;
    const unsigned head = (unsigned)(win >> 62), tail = (unsigned)(win >> (62 - 2 * k)) & 3u;
    s_key[e] = skm_s1_key(f, rc, head, tail);
    s_cnt[e] = tab[e];
    s_pos[e] = tab[kSkmRepN + e];
  }
  __syncthreads();
  unsigned long long cnt = 0, pos = ~0ull;
  bool lead = s_cnt[e] != 0;
  for (int o = 0; o < kSkmRepN; ++o)
    if (s_cnt[o] && s_key[o] == s_key[e]) {
      if (o < e) lead = false;  // (the first entry of a key publishes it)
      cnt += s_cnt[o];
      pos = min(pos, s_pos[o]);
    }
  if (!lead) cnt = 0;
  if (cnt) {
    atomicAdd(&s_tot[0], cnt);
    atomicAdd(&s_tot[1], 1ull);
    const unsigned long long hb = cnt > MHX_MAX_MUL ? (unsigned long long)MHX_MAX_MUL : cnt;
    atomicAdd(&hist[hb], 1ull);  // :430-436
    if (cnt < m) {
      solid_bytes[pos] = 1;  // its only window is a non-solid occurrence
    } else if (agg) {
      const uint64_t x = skm_s1_key_kmer(s_key[e], k, kmask), xr = rc64(x, K1);
      const int n_out = x == xr ? 1 : 2;
      const unsigned long long at = atomicAdd(agg_cursor, (unsigned long long)n_out);
      for (int y = 0; y < n_out; ++y) {
        const uint64_t f = skm_s2_item(y ? xr : x, k, hb);
        agg_items[at + y] = make_uint2((uint32_t)(f >> 32), (uint32_t)f);
        if (agg_hist) {  // the digit histograms of stage 2's sort (k_agg_compact took those of the items before these)
          const uint32_t w[2] = {(uint32_t)(f >> 32), (uint32_t)f};
          for (int p = 0; p < agg_specs.n; ++p) atomicAdd(&agg_hist[p * 256 + words_digit2<2>(w, agg_specs.d[p])], 1ull);
        }
      }
    }
  }
  __syncthreads();
  if (e < 2) res[e] = s_tot[e];
}

// REP, count: the entries -> canonical (k+1)-mers, the tallies of the bases either side moved into the key's orientation (an entry that is
// its key's reverse complement: in front and behind swap and complement), equal keys merged -> what k_count_hp_publish does per key.
// res[0] = edges appended, [1] = keys, [2] = a solid key lacks an in- or out-edge, [3] = the windows counted beside the records
__global__ __launch_bounds__(kSkmRepN) void k_count_rep_publish(const unsigned long long *__restrict__ tab, int k, uint32_t m, unsigned long long *__restrict__ hist,
                                                                unsigned long long *__restrict__ edges_at, unsigned long long *__restrict__ res) {
  __shared__ unsigned long long s_key[kSkmRepN], s_t[kSkmRepN][9];
  __shared__ unsigned long long s_res[4];
  const int e = threadIdx.x, K1 = k + 1;
  if (e < 4) s_res[e] = 0;
  {
    const uint64_t x = skm_rep_window((uint32_t)e, K1);
    bool strand;
    s_key[e] = skm_count_key(x, rc64(x, K1), &strand);
    const unsigned long long *t = tab + 9 * e;
    s_t[e][0] = t[0];
    for (int c = 0; c < 4; ++c) {
      s_t[e][1 + c] = strand ? t[5 + (3 - c)] : t[1 + c];
      s_t[e][5 + c] = strand ? t[1 + (3 - c)] : t[5 + c];
    }
  }
  __syncthreads();
  unsigned long long t[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool lead = s_t[e][0] != 0;
  for (int o = 0; o < kSkmRepN; ++o)
    if (s_t[o][0] && s_key[o] == s_key[e]) {
      if (o < e) lead = false;
      for (int c = 0; c < 9; ++c) t[c] += s_t[o][c];
    }
  if (lead && t[0]) {
    atomicAdd(&s_res[1], 1ull);
    atomicAdd(&s_res[3], t[0]);
    const unsigned long long hb = t[0] > MHX_MAX_MUL ? (unsigned long long)MHX_MAX_MUL : t[0];
    atomicAdd(&hist[hb], 1ull);
    if (t[0] >= m) {
      bool has_in = false, has_out = false;
      for (int c = 0; c < 4; ++c) {
        has_in = has_in || t[1 + c] >= m;
        has_out = has_out || t[5 + c] >= m;
      }
      if (!has_in || !has_out) s_res[2] = 1;
      edges_at[atomicAdd(&s_res[0], 1ull)] = s_key[e] | hb;  // PackEdge, kmer_counter.cpp:32-52
    }
  }
  __syncthreads();
  if (e < 4) res[e] = s_res[e];
}

// the one or two keys the homopolymer windows are (A...A with T...T, C...C with G...G): histogram, the mark of a key seen once, the
// aggregated stage-2 items of a solid one, behind the items of the group-by — as the walk over the table does for every other key
__global__ void k_skm_hp_publish(const unsigned long long *__restrict__ hp, int k, uint32_t m, uint8_t *__restrict__ solid_bytes,
                                 unsigned long long *__restrict__ hist, uint2 *__restrict__ agg_items, uint64_t *__restrict__ agg_cursor, int agg,
                                 DigitSpecs agg_specs, unsigned long long *__restrict__ agg_hist) {
  if (threadIdx.x || blockIdx.x) return;
  for (int x = 0; x < 2; ++x) {
    const unsigned long long cnt = hp[x];
    if (!cnt) continue;
    const unsigned long long hb = cnt > MHX_MAX_MUL ? (unsigned long long)MHX_MAX_MUL : cnt;
    hist[hb] += 1;  // :430-436
    if (cnt < m) {
      solid_bytes[hp[2 + x]] = 1;  // its only window is a non-solid occurrence
    } else if (agg) {
      const uint64_t e0 = x == 0 ? 0ull : 0x5555555555555555ull;  // A...A / C...C, MSB first; the other strand: T...T / G...G
      const uint64_t keep = ~0ull << (64 - 2 * (k + 1));
      const uint64_t xs[2] = {e0 & keep, ~e0 & keep};
      const uint64_t mask_k = ~0ull << (64 - 2 * k);
      uint64_t at = *agg_cursor;
      for (int y = 0; y < 2; ++y) {
        const uint64_t v = xs[y];
        const uint64_t f = ((v << 2) & mask_k) | (1ull << 19) | ((v >> 62) << 16) | hb;
        agg_items[at++] = make_uint2((uint32_t)(f >> 32), (uint32_t)f);
        if (agg_hist) {  // the digit histograms of stage 2's sort (k_agg_compact took those of the items before these)
          const uint32_t w[2] = {(uint32_t)(f >> 32), (uint32_t)f};
          for (int p = 0; p < agg_specs.n; ++p) atomicAdd(&agg_hist[p * 256 + words_digit2<2>(w, agg_specs.d[p])], 1ull);
        }
      }
      *agg_cursor = at;
    }
  }
}

// min count 3 and 4 (s1_skm_max_m): the keys counted beside the records keep the smallest position of their windows and nothing more, so one
// of 1 < count < m windows cannot get its marks.  *res = the count of such a key (the largest of them), 0: none — the entries of the REP
// table that are one key summed first, as k_skm_rep_publish sums them.  One workgroup; writes nothing else
__global__ __launch_bounds__(kSkmRepN) void k_skm_beside_check(const unsigned long long *__restrict__ hp, int rep, int k, uint32_t m, unsigned long long *__restrict__ res) {
  __shared__ unsigned long long s_key[kSkmRepN], s_cnt[kSkmRepN];
  __shared__ unsigned long long s_worst;
  const int e = threadIdx.x, K1 = k + 1;
  const uint64_t kmask = ~0ull << (64 - 2 * (k - 1));
  if (e == 0) s_worst = 0;
  {
    const uint64_t win = skm_rep_window((uint32_t)e, K1);
    const uint64_t f = (win << 2) & kmask, rc = (rc64(win, 32) << (2 * (32 - k))) & kmask;
    const unsigned head = (unsigned)(win >> 62), tail = (unsigned)(win >> (62 - 2 * k)) & 3u;
    s_key[e] = skm_s1_key(f, rc, head, tail);
    s_cnt[e] = rep ? hp[kSkmRepAt + e] : 0ull;
  }
  __syncthreads();
  unsigned long long cnt = 0;
  bool lead = s_cnt[e] != 0;
  for (int o = 0; o < kSkmRepN; ++o)
    if (s_cnt[o] && s_key[o] == s_key[e]) {
      if (o < e) lead = false;
      cnt += s_cnt[o];
    }
  if (!lead) cnt = 0;
  if (e < 2 && !rep) cnt = hp[e];  // (without REP: the two homopolymer classes, a key each)
  if (cnt > 1 && cnt < m) atomicMax(&s_worst, cnt);
  __syncthreads();
  if (e == 0) *res = s_worst;
}

// (Natural super-k-mers — runs cut at eight windows from their OWN start, the windows' minimizer hashes exchanged between the threads of a
//  workgroup through LDS — were built and measured in round 6: 0.23 instead of 0.28 records per window, the two sort passes 5.7 -> 4.8 ms,
//  but the make kernel 3.1 -> 7.9 ms (three barriers, a walk back and a walk forward through LDS per block, 1024-thread workgroups) and the
//  group-by 7.7 -> 8.4 (282 windows per wavefront trip instead of 225: a second, nearly empty round of four chunks).  Not kept:
//  profiles/r06-interim_ab_skm_natural.jsonl.)
// bounds[b] = the first record whose bin is >= b (b = 0 .. n_bins); a thread per bin, a binary search each
__global__ __launch_bounds__(256) void k_skm_bounds(const uint4 *__restrict__ recs, uint64_t n, uint32_t n_bins, uint64_t *__restrict__ bounds,
                                                    uint32_t *__restrict__ max_bin) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b > n_bins) return;
  auto lower = [&](uint32_t v) -> uint64_t {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      const uint32_t bin = (reinterpret_cast<const uint32_t *>(recs + mid)[0] >> 8) & 0xFFFFFu;
      if (bin < v) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  };
  const uint64_t at = b == n_bins ? n : lower(b);
  bounds[b] = at;
  if (b < n_bins) {
    const uint64_t nx = b + 1 == n_bins ? n : lower(b + 1);
    const uint64_t d = nx - at;
    atomicMax(max_bin, d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d);
  }
}

// s1_skm_giant: the bins [bin_lo, bin_hi) of more than `limit` records -> out[1 + i] = (bin, records), in any order, through the cursor in
// the first word of out[0] (zero at launch; it counts every such bin, the list holds the first list_cap); a thread per bin
__global__ __launch_bounds__(256) void k_skm_giants(const uint64_t *__restrict__ bounds, uint32_t bin_lo, uint32_t bin_hi, uint64_t limit, uint2 *__restrict__ out,
                                                    uint32_t list_cap) {
  const uint64_t b = (uint64_t)bin_lo + (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= bin_hi) return;
  const uint64_t d = bounds[b + 1] - bounds[b];
  if (d > limit) {
    const uint32_t at = atomicAdd(reinterpret_cast<uint32_t *>(out), 1u);
    if (at < list_cap) out[1 + at] = make_uint2((uint32_t)b, d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d);
  }
}

struct SkmArgs {
  int k;
  uint32_t m;
  uint8_t *solid_bytes;
  unsigned long long *hist;
  uint2 *agg_raw;
  uint32_t agg_cap;
  uint32_t *agg_counts;
  uint32_t *err;
  uint32_t max_fill;
  int probe_limit;
  uint32_t bin_lo, bin_hi;  // the bins of this pass
  // several GPUs: the reads live on other ranks — a mark is the global position itself, appended to the workgroup's region
  // marks_raw[blockIdx.x * marks_cap ...] (count in marks_counts[blockIdx.x]); the host packs the regions and routes them (comm.hip)
  unsigned long long *marks_raw;
  uint32_t marks_cap;
  uint32_t *marks_counts;
  // GIANT (s1_skm_giant, one source): tickets 0 .. n_giant - 1 are the work items giants[] = (bin, sub0 << 16 | rj0) — the rounds of a bin
  // of more than giant_limit records from (sub0, rj0) on (skm_giant.h); the tickets behind them are the batches, which skip those bins
  const uint2 *giants;
  uint32_t n_giant, giant_limit;
};
// the records of a bin arrive as one sub-range per source: one array on a single GPU; on several, one per sending rank (each ordered by bin)
struct SkmSrcs {
  const uint4 *ptr[kSkmSrcMax];
  const uint64_t *bounds[kSkmSrcMax];  // [n_bins + 1] each
  int n;
};

constexpr int kSkmThreads = 1024, kSkmLogSlots = 13;

// exclusive prefix sum over the wavefront of a value below 16, its total in *total (uniform): one ballot per bit, counted below the lane
// and over the wavefront — a dozen vector and scalar instructions, where wave_inclusive_sum / wave_sum take six LDS round trips in a row
__device__ __forceinline__ uint32_t wave_exclusive_sum_4bit(uint32_t v, uint32_t *total) {
  uint32_t ex = 0, tot = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const unsigned long long has = __ballot((v >> b) & 1u);
    ex += __builtin_amdgcn_mbcnt_hi((uint32_t)(has >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)has, 0u)) << b;
    tot += (uint32_t)__builtin_popcountll(has) << b;
  }
  *total = tot;
  return ex;
}

// TAGS: read sets of 2^32 bases and more — the position bits above 32 ride in the record's first word and next to the key in the table
// DEAL: 0 every lane expands its own record, 1 the windows are dealt to the lanes with six shuffles, 2 with three (skm_deal.h)
// GIANT: the first a.n_giant tickets are slices of giant bins (one source); the other forms are the code they were without it
// LOOK (s1_skm_max_m, min count 3 and 4; DEAL 2, one GPU): a key of count 1 < c < m has c windows to mark and the slot keeps the position of
// ONE — a round that holds such a key expands its records a second time, and every window whose key's count is below m marks itself.  The
// table is cleared behind that look instead of during the walk: three more barriers a round.  The other forms are the code they were
template <bool AGG, bool TAGS, int DEAL, bool GIANT = false, bool LOOK = false>
__global__ __launch_bounds__(kSkmThreads) void k_s1_skm(SkmSrcs srcs, SkmArgs a, uint32_t *__restrict__ ticket) {
  static_assert(!LOOK || (DEAL == 2 && !GIANT), "the second look is built on the three-shuffle deal, bins whole");
  constexpr int NT = kSkmThreads, NSLOT = 1 << kSkmLogSlots, W = NSLOT / NT;
  constexpr unsigned long long kEmpty = ~0ull;  // never a key: head / tail bits 63 do not occur
  constexpr int NLIST = 1024;
  __shared__ unsigned long long keys[NSLOT];
  __shared__ uint32_t cnts[NSLOT];
  __shared__ uint32_t fpos[NSLOT];
  __shared__ uint8_t ftag[TAGS ? NSLOT : 4];
  __shared__ uint32_t lhist[kSegHist];
  __shared__ unsigned long long slist_k[AGG ? NLIST : 1];
  __shared__ uint32_t slist_c[AGG ? NLIST : 1];
  __shared__ unsigned long long heads[DEAL ? kSkmThreads / kWave : 1][8];  // DEAL, per wavefront: bit g set = window g of the trip is the first of its record
  __shared__ uint32_t s_bad2[2], s_nclaimed2[2], s_list_n2[2];  // per round, double-buffered: the next round's are cleared while this round's are read
  __shared__ uint32_t s_agg_cur, s_mark_cur, s_tk;
  __shared__ uint32_t s_look;  // LOOK (touched by no other form): the round holds a key of count 1 < c < m (set in the walk, cleared with the table)
  __shared__ uint64_t s_lo[kSkmSrcMax][kSkmBatch + 1];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = DEAL ? tid / kWave : 0;
  const uint32_t le_lo = lane >= 31 ? 0xFFFFFFFFu : (2u << lane) - 1u, le_hi = lane < 32 ? 0u : (lane == 63 ? 0xFFFFFFFFu : (2u << (lane - 32)) - 1u);  // lanes <= this one
  const int k = a.k, K1 = k + 1;
  const uint32_t m = a.m;
  const uint64_t kmask = ~0ull << (64 - 2 * (k - 1));
  uint2 *const agg_end = AGG ? a.agg_raw + (size_t)(blockIdx.x + 1) * a.agg_cap : nullptr;
  for (int i = tid; i < NSLOT; i += NT) {
    keys[i] = kEmpty;
    cnts[i] = 0;
  }
  for (int i = tid; i < kSegHist; i += NT) lhist[i] = 0;
  if (tid == 0) {
    s_bad2[0] = s_bad2[1] = 0;
    s_nclaimed2[0] = s_nclaimed2[1] = 0;
    s_list_n2[0] = s_list_n2[1] = 0;
    s_agg_cur = 0;
    s_mark_cur = 0;
    if constexpr (LOOK) s_look = 0;
  }
  const int n_src = srcs.n;
  unsigned long long *const marks_out = a.marks_raw ? a.marks_raw + (size_t)blockIdx.x * a.marks_cap : nullptr;
  int rp = 0;  // the round's parity
  __syncthreads();

  // the aggregated stage-2 items of a solid key (one per strand; one for a palindrome) -> this workgroup's region, from its end
  auto emit_items = [&](unsigned long long key, uint32_t cnt, bool dense, bool valid) {
    uint64_t x = 0, xr = 0;
    uint32_t n_out = 0;
    if (valid) {
      x = skm_s1_key_kmer(key, k, kmask);
      xr = rc64(x, K1);
      n_out = x == xr ? 1u : 2u;
    }
    uint32_t at;
    bool ok;
    if (dense) {
      const uint32_t incl = wave_inclusive_sum(n_out);
      const uint32_t tot = __shfl(incl, kWave - 1, kWave);
      if (!tot) return;
      uint32_t wbase = 0;
      if (lane == 0) wbase = atomicAdd(&s_agg_cur, tot);
      wbase = __shfl(wbase, 0, kWave);
      ok = wbase + tot <= a.agg_cap;
      at = wbase + incl - n_out;
    } else {
      at = atomicAdd(&s_agg_cur, n_out);
      ok = at + n_out <= a.agg_cap;
    }
    if (!ok) {
      atomicOr(a.err, 1u);
      return;
    }
    if (n_out) {
      const uint64_t mul = cnt > MHX_MAX_MUL ? (uint64_t)MHX_MAX_MUL : cnt;
      const uint64_t f = skm_s2_item(x, k, mul);
      agg_end[-1 - (long)at] = make_uint2((uint32_t)(f >> 32), (uint32_t)f);
      if (n_out == 2) {
        const uint64_t b = skm_s2_item(xr, k, mul);
        agg_end[-2 - (long)at] = make_uint2((uint32_t)(b >> 32), (uint32_t)b);
      }
    }
  };

  uint4 pre = make_uint4(0u, 0u, 0u, 0u);  // a first trip requested ahead (of the bin that starts at pre_at)
  uint64_t pre_at = 0;
  bool pre_ok = false;
  for (;;) {
    if (tid == 0) s_tk = atomicAdd(ticket, 1u);
    __syncthreads();
    // GIANT: the first tickets are slices of giant bins — the bin alone in the batch, its rounds from (sub0, rj0) on
    uint32_t sub0 = 0, rj0 = 0;
    bool slice = false;
    if constexpr (GIANT) slice = s_tk < a.n_giant;  // (uniform)
    if (slice) {
      // (the item is the same in every lane: kept in scalar registers through the rounds)
      const uint2 item = a.giants[(uint32_t)__builtin_amdgcn_readfirstlane((int)s_tk)];
      const uint32_t depth_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)item.y);
      sub0 = depth_at >> 16;
      rj0 = depth_at & 0xFFFFu;
      if (tid <= kSkmBatch) s_lo[0][tid] = srcs.bounds[0][item.x + (tid ? 1u : 0u)];
    } else {
      const uint64_t bin0 = (uint64_t)a.bin_lo + (uint64_t)(s_tk - (GIANT ? a.n_giant : 0u)) * kSkmBatch;
      if (bin0 >= a.bin_hi) break;
      if (tid < n_src * (kSkmBatch + 1)) {
        const int q = tid / (kSkmBatch + 1), x = tid - q * (kSkmBatch + 1);
        s_lo[q][x] = srcs.bounds[q][min(bin0 + x, (uint64_t)a.bin_hi)];
      }
    }
    __syncthreads();
    for (int bb = 0; bb < kSkmBatch; ++bb) {
      bool any = false;
      for (int q = 0; q < n_src; ++q) any = any || s_lo[q][bb] != s_lo[q][bb + 1];
      if (!any) continue;
      const uint64_t lo0 = s_lo[0][bb], hi0 = s_lo[0][bb + 1];
      if constexpr (GIANT)
        if (!slice && hi0 - lo0 > (uint64_t)a.giant_limit) continue;  // (uniform) a giant bin inside a batch: its slices are tickets of their own
      // the bin in rounds: round (sub, rj) takes the keys whose top `sub` bits of a second hash are rj (a round that overflows the
      // table is redone in two halves; skm_giant.h) — a slice of a giant bin: the rounds from (sub0, rj0) on
      uint32_t sub = sub0, rj = rj0;
      for (;;) {
        uint32_t seen = 0;
        // A: insert, source by source (the round's first trip was requested before the walk of the round before it)
        for (int q = 0; q < n_src; ++q) {
        const uint64_t lo = s_lo[q][bb], hi = s_lo[q][bb + 1];
        if (lo == hi) continue;
        const uint4 *__restrict__ recs = srcs.ptr[q];
        uint4 nxt = q == 0 && pre_ok && pre_at == lo ? pre : (lo + tid < hi ? recs[lo + tid] : make_uint4(0u, 0u, 0u, 0u));
        if (q == 0) pre_ok = false;
        for (uint64_t base = lo; base < hi; base += NT) {
          const uint4 r = nxt;
          const bool in = base + tid < hi;
          if (base + NT + tid < hi) nxt = recs[base + NT + tid];
          if (seen > a.max_fill) continue;  // (uniform per wavefront; the round is redone in halves anyway)
          const uint32_t len = in ? (r.z & 7u) + 1u : 0u;
          const uint8_t tag = TAGS ? (uint8_t)(r.x >> 28) : (uint8_t)0;
          uint32_t claims = 0;
          // (the slot found — the key's own, or a free one claimed: count it, and remember the window that claimed it)
          auto settle = [&](unsigned long long old, unsigned long long key, uint32_t hh, uint32_t pos, uint8_t tg) -> bool {
            if (old != kEmpty && old != key) return false;
            atomicAdd(&cnts[hh], 1u);
            if (old == kEmpty) {  // only read back when the count stays 1: then this window is the key's only one
              fpos[hh] = pos;
              if constexpr (TAGS) ftag[hh] = tg;
              ++claims;
            }
            return true;
          };
          const uint64_t rec_b = ((uint64_t)r.y << 32) | r.z;
          if constexpr (DEAL != 0) {
            // The windows of the wavefront's 64 records (~225) are DEALT to the lanes, 64 at a time: window g belongs to the record whose
            // run of windows starts at or before g — a bitmap of run heads per wavefront, one population count per window — and comes
            // over with six shuffles (DEAL 1) or three (DEAL 2).  All lanes work on every step (own-record expansion: 44 % of the lane
            // steps, below); four steps share one round of compare-and-swaps and one retry loop.
            uint32_t start, T;  // the record's first window, and the windows of the trip (uniform)
            if constexpr (DEAL == 2) {
              start = wave_exclusive_sum_4bit(len, &T);  // (from ballots: DEAL 1 takes six dependent shuffles here, and six more for the claims below)
            } else {
              const uint32_t incl = wave_inclusive_sum(len);
              T = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
              start = incl - len;
            }
            // (the LDS executes a wavefront's operations in order: clear, set, read — no barrier between them)
            if (lane < 8) heads[wv][lane] = 0ull;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (len) atomicOr(&heads[wv][start >> 6], 1ull << (start & 63u));
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const unsigned long long hv = __hip_atomic_load(&heads[wv][lane & 7], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint32_t hv_lo = (uint32_t)hv, hv_hi = (uint32_t)(hv >> 32);
            const uint32_t bh = r.y, bl = r.z;
            // DEAL 1 shuffles the record's reverse complement (of its 32 base slots, once: a window's is a sub-window of it) and its
            // position less its start (position of window g of the trip = pd + g), and counts the heads in front of a step's windows,
            // minus one; DEAL 2 carries that count and the windows behind the last head (skm_deal.h)
            [[maybe_unused]] uint32_t qh = 0, ql = 0, pd = 0, cbase_m1 = 0xFFFFFFFFu;
            [[maybe_unused]] SkmDealCarry dc;
            if constexpr (DEAL == 1) {
              const uint64_t rec_r = rc64(rec_b, 32);
              qh = (uint32_t)(rec_r >> 32), ql = (uint32_t)rec_r;
              pd = r.w - start;
            }
#pragma unroll
            for (int grp = 0; grp < 2; ++grp) {
              if ((uint32_t)(grp * 4 * kWave) >= T) break;  // (uniform)
              unsigned long long key[4], old1[4];
              uint32_t h1[4], pos[4], mine = 0;
              uint8_t tg[4];
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                const int c = grp * 4 + u;
                const uint32_t w_lo = (uint32_t)__builtin_amdgcn_readlane((int)hv_lo, c), w_hi = (uint32_t)__builtin_amdgcn_readlane((int)hv_hi, c);
                // DEAL 2: the record's lane and the window's index in it come from the bitmap, the reverse complement from the window:
                // three shuffles (the base bits, the position) where DEAL 1 has six
                uint32_t o, j, xbh, xbl, p0;
                uint64_t win, rc;
                bool mn;  // the window is one of the trip's
                if constexpr (DEAL == 2) {
                  const SkmDealAt d = skm_deal_at(((uint64_t)w_hi << 32) | w_lo, (uint32_t)lane, dc);
                  o = d.o;
                  j = d.j & 7u;  // (a window past the end of the trip: any shift that is defined)
                  xbh = __shfl(bh, (int)o, kWave), xbl = __shfl(bl, (int)o, kWave);
                  p0 = __shfl(r.w, (int)o, kWave);
                  win = (((uint64_t)xbh << 32) | xbl) << (2 * j);
                  rc = skm_win_rc(win, k, kmask);
                  pos[u] = p0 + j;
                  mn = lane < (int)T - c * kWave;  // (g < T, against a scalar)
                } else {
                  const uint32_t g = (uint32_t)(c * kWave) + (uint32_t)lane;
                  o = cbase_m1 + (uint32_t)__builtin_popcount(w_lo & le_lo) + (uint32_t)__builtin_popcount(w_hi & le_hi);
                  cbase_m1 += (uint32_t)__builtin_popcount(w_lo) + (uint32_t)__builtin_popcount(w_hi);
                  xbh = __shfl(bh, (int)o, kWave), xbl = __shfl(bl, (int)o, kWave);
                  const uint32_t xqh = __shfl(qh, (int)o, kWave), xql = __shfl(ql, (int)o, kWave);
                  const uint32_t so = __shfl(start, (int)o, kWave), pdo = __shfl(pd, (int)o, kWave);
                  j = g - so;
                  win = (((uint64_t)xbh << 32) | xbl) << (2 * j);  // the (k+1)-mer head.S.tail, MSB first
                  rc = ((((uint64_t)xqh << 32) | xql) << (2 * (32 - k - j))) & kmask;
                  pos[u] = pdo + g;
                  p0 = pdo + so;
                  mn = g < T;
                }
                const uint64_t f = (win << 2) & kmask;
                const unsigned head = (unsigned)(win >> 62), tail = ((uint32_t)win >> (62 - 2 * k)) & 3u;  // (k <= 22: the tail sits in the low word)
                key[u] = skm_s1_key(f, rc, head, tail);
                const uint32_t klo = (uint32_t)key[u], khi = (uint32_t)(key[u] >> 32);
                if (sub) mn = mn && skm_in_round(skm_mix2((klo * 0xC2B2AE35u) ^ (khi * 0x27D4EB2Fu)), sub, rj);  // (uniform branch)
                mine |= mn ? 1u << u : 0u;
                h1[u] = ((klo * 0x9E3779B1u) ^ (khi * 0x85EBCA6Bu)) >> (32 - kSkmLogSlots);
                if constexpr (TAGS) {  // (p0, the record's own position word: a run across a multiple of 2^32 carries into the tag)
                  tg[u] = (uint8_t)(__shfl((uint32_t)tag, (int)o, kWave) + (pos[u] < p0 ? 1u : 0u));
                } else {
                  tg[u] = 0;
                }
              }
              if (a.probe_limit <= 0) {
                if (mine) s_bad2[rp] = 1;
                mine = 0;
              }
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                old1[u] = kEmpty;
                if ((mine >> u) & 1u) old1[u] = atomicCAS(&keys[h1[u]], kEmpty, key[u]);
              }
              bool has = false;
              unsigned long long pk = 0;
              uint32_t ph = 0, pp = 0;
              uint8_t pt = 0;
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                if ((mine >> u) & 1u) {
                  if (!settle(old1[u], key[u], h1[u], pos[u], tg[u])) {
                    uint32_t hh = (h1[u] + 1) & (NSLOT - 1);
                    if (!has) {
                      has = true;
                      pk = key[u], ph = hh, pp = pos[u], pt = tg[u];
                    } else {
                      int n = 0;
                      while (!settle(atomicCAS(&keys[hh], kEmpty, key[u]), key[u], hh, pos[u], tg[u])) {
                        hh = (hh + 1) & (NSLOT - 1);
                        if (++n >= a.probe_limit) {
                          s_bad2[rp] = 1;
                          break;
                        }
                      }
                    }
                  }
                }
              }
              int turns = 0;
              while (__ballot(has)) {
                if (has) {
                  if (settle(atomicCAS(&keys[ph], kEmpty, pk), pk, ph, pp, pt)) has = false;
                  else ph = (ph + 1) & (NSLOT - 1);
                }
                if (++turns > a.probe_limit) {  // (uniform: every lane counts the same turns)
                  if (has) s_bad2[rp] = 1;
                  break;
                }
              }
            }
          } else {
            // Every lane expands its own record, four windows at a time: the keys are independent of each other, so their compare-and-swaps
            // go out back to back and one LDS round trip serves four windows; lanes whose record is shorter idle.
            const uint64_t rec_r = rc64(rec_b, 32);  // (of the record's 32 base slots, once: a window's reverse complement is a sub-window of it)
  #pragma unroll
            for (int half = 0; half < 2; ++half) {
              if (half == 1 && __ballot(len > 4u) == 0) break;  // (uniform)
              unsigned long long key[4], old1[4];
              uint32_t h1[4], mine = 0;
  #pragma unroll
              for (int u = 0; u < 4; ++u) {
                const int j = half * 4 + u;
                const uint64_t win = rec_b << (2 * j);  // the (k+1)-mer head.S.tail, MSB first
                const uint64_t f = (win << 2) & kmask;
                const uint64_t rc = (rec_r << (2 * (32 - k - j))) & kmask;
                const unsigned head = (unsigned)(win >> 62), tail = (unsigned)(win >> (62 - 2 * k)) & 3u;
                key[u] = skm_s1_key(f, rc, head, tail);
                const uint32_t klo = (uint32_t)key[u], khi = (uint32_t)(key[u] >> 32);
                bool mn = (uint32_t)j < len;
                if (sub) mn = mn && skm_in_round(skm_mix2((klo * 0xC2B2AE35u) ^ (khi * 0x27D4EB2Fu)), sub, rj);  // (uniform branch)
                mine |= mn ? 1u << u : 0u;
                h1[u] = ((klo * 0x9E3779B1u) ^ (khi * 0x85EBCA6Bu)) >> (32 - kSkmLogSlots);
              }
              if (a.probe_limit <= 0) {
                if (mine) s_bad2[rp] = 1;
                mine = 0;
              }
  #pragma unroll
              for (int u = 0; u < 4; ++u) {
                old1[u] = kEmpty;
                if ((mine >> u) & 1u) old1[u] = atomicCAS(&keys[h1[u]], kEmpty, key[u]);
              }
              // a lane that met another key keeps the window pending — one per lane; a second one of the same four is seen to on the spot —
              // and the pending windows of all lanes are retried together
              bool has = false;
              unsigned long long pk = 0;
              uint32_t ph = 0, pp = 0;
              uint8_t pt = 0;
  #pragma unroll
              for (int u = 0; u < 4; ++u) {
                if ((mine >> u) & 1u) {
                  const uint32_t pos = r.w + (uint32_t)(half * 4 + u);
                  const uint8_t ptag = TAGS ? (uint8_t)(tag + (pos < r.w ? 1 : 0)) : (uint8_t)0;  // (a run across a multiple of 2^32)
                  if (!settle(old1[u], key[u], h1[u], pos, ptag)) {
                    uint32_t hh = (h1[u] + 1) & (NSLOT - 1);
                    if (!has) {
                      has = true;
                      pk = key[u], ph = hh, pp = pos, pt = ptag;
                    } else {
                      int n = 0;
                      while (!settle(atomicCAS(&keys[hh], kEmpty, key[u]), key[u], hh, pos, ptag)) {
                        hh = (hh + 1) & (NSLOT - 1);
                        if (++n >= a.probe_limit) {
                          s_bad2[rp] = 1;
                          break;
                        }
                      }
                    }
                  }
                }
              }
              int turns = 0;
              while (__ballot(has)) {
                if (has) {
                  if (settle(atomicCAS(&keys[ph], kEmpty, pk), pk, ph, pp, pt)) has = false;
                  else ph = (ph + 1) & (NSLOT - 1);
                }
                if (++turns > a.probe_limit) {  // (uniform: every lane counts the same turns)
                  if (has) s_bad2[rp] = 1;
                  break;
                }
              }
            }
          }
          {
            uint32_t c;
            if constexpr (DEAL == 2) wave_exclusive_sum_4bit(claims, &c);  // (a lane deals with eight windows a trip at the most)
            else c = wave_sum(claims);
            if (lane == 0 && c) atomicAdd(&s_nclaimed2[rp], c);
            seen = __hip_atomic_load(&s_nclaimed2[rp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            seen = (uint32_t)__builtin_amdgcn_readfirstlane((int)seen);
          }
        }
        }  // (sources)
        __syncthreads();  // the table is complete
        const bool bad = s_bad2[rp] != 0 || s_nclaimed2[rp] > a.max_fill;
        if (tid == 0) {  // (the other parity: last read behind the first barrier of the round before this one)
          s_bad2[rp ^ 1] = 0;
          s_nclaimed2[rp ^ 1] = 0;
          s_list_n2[rp ^ 1] = 0;
        }
        uint32_t nsub, nrj;
        bool done, give_up;
        skm_next_round(sub, rj, bad, sub0, rj0, &nsub, &nrj, &done, &give_up);
        if (give_up && tid == 0) atomicOr(a.err, 1u);
        {  // the first trip of what comes next — this bin again, or the next bin of the batch that holds records — is requested here (first source;
           // used only where the next insert starts at pre_at: a ticket of the other kind, or a bin that is skipped, asks again)
          uint64_t nlo = lo0, nhi = hi0;
          if (done) {
            nlo = nhi = 0;
            for (int nb = bb + 1; nb < kSkmBatch; ++nb)
              if (s_lo[0][nb] != s_lo[0][nb + 1] && !(GIANT && !slice && s_lo[0][nb + 1] - s_lo[0][nb] > (uint64_t)a.giant_limit)) {
                nlo = s_lo[0][nb];
                nhi = s_lo[0][nb + 1];
                break;
              }
          }
          if (nlo != nhi) {
            pre = nlo + tid < nhi ? srcs.ptr[0][nlo + tid] : make_uint4(0u, 0u, 0u, 0u);
            pre_at = nlo;
            pre_ok = true;
          }
        }
        // C: one walk over the table — per distinct key: histogram, the mark of a non-solid key's only record, the solid keys listed
        unsigned long long wk[W];
        uint32_t wc[W], wp[W];
        uint8_t wt[W];
#pragma unroll
        for (int it = 0; it < W; ++it) {
          const int sl = it * NT + tid;
          wk[it] = keys[sl];
          wc[it] = cnts[sl];
          wp[it] = fpos[sl];
          wt[it] = TAGS ? ftag[sl] : (uint8_t)0;
        }
        if constexpr (!LOOK) {
#pragma unroll
        for (int it = 0; it < W; ++it) {
          const int sl = it * NT + tid;
          keys[sl] = kEmpty;
          cnts[sl] = 0;
        }
        }  // (LOOK: the second look reads the table; it is cleared behind that)
        uint32_t want_bits = 0, mark_bits = 0;
        [[maybe_unused]] bool look_mine = false;
#pragma unroll
        for (int it = 0; it < W; ++it) {
          if (wk[it] != kEmpty && !bad) {
            const uint32_t cnt = wc[it];
            const uint32_t hb = cnt > MHX_MAX_MUL ? (uint32_t)MHX_MAX_MUL : cnt;  // :430-436
            if (hb < kSegHist) atomicAdd(&lhist[hb], 1u);
            else atomicAdd(&a.hist[hb], 1ull);
            if (cnt < m) mark_bits |= 1u << it;  // count 1 < m <= 2: the key's only window is a non-solid occurrence
            else if (AGG) want_bits |= 1u << it;
            // (LOOK, m = 3 or 4: a key of count 1 is marked here all the same — a round of such keys alone needs no look; one of count 2 or
            //  3 below m gets ONE of its marks here, the window that claimed the slot, and all of them in the look)
            if constexpr (LOOK) look_mine = look_mine || (cnt > 1u && cnt < m);
          }
        }
        if constexpr (LOOK) {  // (one flag for the workgroup, from a ballot: as s_flagged of k_count_skm)
          if (__ballot(look_mine) && lane == 0) s_look = 1;
        }
        if (!marks_out) {  // (uniform)
#pragma unroll
          for (int it = 0; it < W; ++it)
            if ((mark_bits >> it) & 1u) a.solid_bytes[((uint64_t)wt[it] << 32) | wp[it]] = 1;
        } else {  // several GPUs: the mark is the global position itself, appended to this workgroup's region
          const uint32_t n_mk = (uint32_t)__builtin_popcount(mark_bits);
          const uint32_t incl = wave_inclusive_sum(n_mk);
          const uint32_t tot = __shfl(incl, kWave - 1, kWave);
          if (tot) {
            uint32_t mbase = 0;
            if (lane == 0) mbase = atomicAdd(&s_mark_cur, tot);
            mbase = __shfl(mbase, 0, kWave);
            uint32_t at = mbase + incl - n_mk;
#pragma unroll
            for (int it = 0; it < W; ++it)
              if ((mark_bits >> it) & 1u) {
                if (at < a.marks_cap) marks_out[at] = ((unsigned long long)wt[it] << 32) | wp[it];
                else atomicOr(a.err, 2u);
                ++at;
              }
          }
        }
        if constexpr (AGG) {
          const uint32_t n_w = (uint32_t)__builtin_popcount(want_bits);
          const uint32_t incl = wave_inclusive_sum(n_w);
          const uint32_t tot = __shfl(incl, kWave - 1, kWave);
          if (tot) {
            uint32_t lbase = 0;
            if (lane == 0) lbase = atomicAdd(&s_list_n2[rp], tot);
            lbase = __shfl(lbase, 0, kWave);
            uint32_t at = lbase + incl - n_w;
#pragma unroll
            for (int it = 0; it < W; ++it)
              if ((want_bits >> it) & 1u) {
                if (at < (uint32_t)NLIST) {
                  slist_k[at] = wk[it];
                  slist_c[at] = wc[it];
                } else {
                  emit_items(wk[it], wc[it], false, true);  // (more solid keys in one round than the list holds: in place)
                }
                ++at;
              }
          }
        }
        __syncthreads();  // the table is empty, the list complete
        if constexpr (AGG) {
          const uint32_t n_list = min(s_list_n2[rp], (uint32_t)NLIST);
          for (uint32_t base = 0; base < n_list; base += NT) {
            const uint32_t i = base + tid;
            const bool v = i < n_list;
            emit_items(v ? slist_k[i] : 0ull, v ? slist_c[i] : 0u, true, v);
          }
        }
        if constexpr (LOOK) {
          // The second look.  (Barrier between walk and look: the one above — behind it s_look is written and every thread has taken its
          // slots into registers; the look only READS keys and cnts, which nobody writes until the clear below.)
          if (tid == 0 && !bad) {  // (for the plan line: a.err[1] the rounds walked, a.err[2] those that took the look)
            atomicAdd(a.err + 1, 1u);
            if (s_look) atomicAdd(a.err + 2, 1u);
          }
          if (s_look && !bad) {  // (uniform; a round that was not bad holds every one of its windows in the table)
            for (int q = 0; q < n_src; ++q) {
              const uint64_t lo = s_lo[q][bb], hi = s_lo[q][bb + 1];
              const uint4 *__restrict__ recs = srcs.ptr[q];
              for (uint64_t base = lo; base < hi; base += NT) {
                const bool in = base + tid < hi;
                const uint4 r = in ? recs[base + tid] : make_uint4(0u, 0u, 0u, 0u);
                const uint32_t len = in ? (r.z & 7u) + 1u : 0u;
                const uint8_t tag = TAGS ? (uint8_t)(r.x >> 28) : (uint8_t)0;
                uint32_t T;
                const uint32_t start = wave_exclusive_sum_4bit(len, &T);
                // (the bitmap of run heads, as the insert makes it: clear, set, read, in the wavefront's own order)
                if (lane < 8) heads[wv][lane] = 0ull;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (len) atomicOr(&heads[wv][start >> 6], 1ull << (start & 63u));
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const unsigned long long hv = __hip_atomic_load(&heads[wv][lane & 7], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const uint32_t hv_lo = (uint32_t)hv, hv_hi = (uint32_t)(hv >> 32);
                SkmDealCarry dc;
                for (uint32_t c = 0; c * kWave < T; ++c) {  // (uniform)
                  const uint32_t w_lo = (uint32_t)__builtin_amdgcn_readlane((int)hv_lo, (int)c), w_hi = (uint32_t)__builtin_amdgcn_readlane((int)hv_hi, (int)c);
                  const SkmDealAt d = skm_deal_at(((uint64_t)w_hi << 32) | w_lo, (uint32_t)lane, dc);
                  const uint32_t o = d.o, j = d.j & 7u;
                  const uint32_t xbh = __shfl(r.y, (int)o, kWave), xbl = __shfl(r.z, (int)o, kWave), p0 = __shfl(r.w, (int)o, kWave);
                  const uint64_t win = (((uint64_t)xbh << 32) | xbl) << (2 * j);
                  const uint64_t rc = skm_win_rc(win, k, kmask), f = (win << 2) & kmask;
                  const unsigned head = (unsigned)(win >> 62), tail = ((uint32_t)win >> (62 - 2 * k)) & 3u;
                  const unsigned long long key = skm_s1_key(f, rc, head, tail);
                  const uint32_t klo = (uint32_t)key, khi = (uint32_t)(key >> 32), pos = p0 + j;
                  [[maybe_unused]] uint32_t tg = 0;
                  if constexpr (TAGS) tg = (uint8_t)(__shfl((uint32_t)tag, (int)o, kWave) + (pos < p0 ? 1u : 0u));  // (the carry across 2^32, as the insert has it)
                  bool mn = c * kWave + (uint32_t)lane < T;
                  // (a redone half takes its own windows only: those of the other half are not in the table)
                  if (sub) mn = mn && skm_in_round(skm_mix2((klo * 0xC2B2AE35u) ^ (khi * 0x27D4EB2Fu)), sub, rj);
                  if (mn) {
                    uint32_t h = ((klo * 0x9E3779B1u) ^ (khi * 0x85EBCA6Bu)) >> (32 - kSkmLogSlots);
                    // the window's key IS in the table; a fault of the logic must not spin: NSLOT steps at the most, then an error the host throws on
                    int n = 0;
                    while (keys[h] != key && n < NSLOT) {
                      h = (h + 1) & (NSLOT - 1);
                      ++n;
                    }
                    if (n >= NSLOT) atomicOr(a.err, 4u);
                    else if (cnts[h] < m) a.solid_bytes[((uint64_t)tg << 32) | pos] = 1;
                  }
                }
              }
            }
          }
          __syncthreads();  // between look and clear: every wavefront has finished its look-ups (and read s_look) before a slot is emptied
#pragma unroll
          for (int it = 0; it < W; ++it) {
            const int sl = it * NT + tid;
            keys[sl] = kEmpty;
            cnts[sl] = 0;
          }
          if (tid == 0) s_look = 0;
          // between clear and the next round's inserts: a slot is emptied by ONE thread, and another wavefront's compare-and-swap on it must
          // come behind that (the other forms clear a slot in the walk, in front of the barrier above the list)
          __syncthreads();
        }
        // (no barrier here: the next round's inserts touch the table and the other parity's counters only; its walk, which writes the
        //  list again, comes behind that round's first barrier — by then every thread has left this loop)
        rp ^= 1;
        sub = nsub;
        rj = nrj;
        if (done) break;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < kSegHist; i += NT)
    if (lhist[i]) atomicAdd(&a.hist[i], (unsigned long long)lhist[i]);
  if (AGG && tid == 0) a.agg_counts[blockIdx.x] = s_agg_cur < a.agg_cap ? s_agg_cur : a.agg_cap;
  if (marks_out && tid == 0) a.marks_counts[blockIdx.x] = s_mark_cur < a.marks_cap ? s_mark_cur : a.marks_cap;
}

// count: the one or two keys the homopolymer windows are -> histogram, the packed edge of a solid one behind the passes' edges.  A solid one
// WITHOUT an in- or out-edge would have to move first_0_out / last_0_in of every read that holds such a window: res[2] says so and the
// caller takes the prefix plan (poly-A / poly-G stretches are preceded and followed by their own base: not seen in practice)
__global__ void k_count_hp_publish(const unsigned long long *__restrict__ hp, int k, uint32_t m, unsigned long long *__restrict__ hist,
                                   unsigned long long *__restrict__ edges_at, unsigned long long *__restrict__ res) {
  if (threadIdx.x || blockIdx.x) return;
  unsigned long long n_edges = 0, n_keys = 0, flagged = 0;
  for (int x = 0; x < 2; ++x) {
    const unsigned long long *t = hp + 8 + x * 16;
    const unsigned long long cnt = t[0];
    if (!cnt) continue;
    ++n_keys;
    const unsigned long long hb = cnt > MHX_MAX_MUL ? (unsigned long long)MHX_MAX_MUL : cnt;
    hist[hb] += 1;
    if (cnt >= m) {
      bool has_in = false, has_out = false;
      for (int c = 0; c < 4; ++c) {
        has_in = has_in || t[1 + c] >= m;
        has_out = has_out || t[5 + c] >= m;
      }
      if (!has_in || !has_out) flagged = 1;
      const uint64_t key = (x == 0 ? 0ull : 0x5555555555555555ull) & (~0ull << (64 - 2 * (k + 1)));
      edges_at[n_edges++] = key | hb;  // PackEdge, kmer_counter.cpp:32-52
    }
  }
  res[0] = n_edges;
  res[1] = n_keys;
  res[2] = flagged;
}

// ---------------------------------------------------------------------------------------------------------------
// `count` on super-k-mer records (KmerCounter::Lv2Postprocess, kmer_counter.cpp:254-381, on the records k_skm_make<.., COUNT> makes): the
// table key is the canonical (k+1)-mer (the smaller of the window and its reverse complement, :179), the slot's third word holds, per base
// in front and base behind — in the key's orientation — "seen once" and "seen twice" bits (min count <= 2: has_in / has_out need no more);
// the walk over the table takes the histogram, sends a solid key's packed edge (PackEdge, :32-52) to the workgroup's region and leaves two
// flag bits in the slot of a solid key without an in- or out-edge; a bin that has such a key is expanded once more, and the windows of the
// flagged keys move first_0_out / last_0_in of their reads (:307-368).  One GPU; the windows are dealt to the lanes as in k_s1_skm.
struct CountSkmArgs {
  int k;
  uint32_t m;
  unsigned long long *hist, *ctr;  // ctr[4]: distinct keys
  unsigned long long *edges_raw;   // per-workgroup regions of packed edges, filled from the front
  uint32_t edges_cap;
  uint32_t *edges_counts;
  uint32_t *err;
  uint32_t max_fill;
  int probe_limit;
  uint32_t bin_lo, bin_hi;
  const uint64_t *c_start;
  uint64_t c_n_seqs;
  uint32_t c_fixed_len;
  uint32_t *first_0_out, *last_0_in_p1;
  // EVENTS (several GPUs: the reads live on other ranks): per-workgroup regions of events, position << 1 | (1: first_0_out, 0: last_0_in) —
  // what k_s1_stream<COUNT> writes and k_apply_count_events reads; ev_counts[workgroup] is the region's cursor (zero at launch)
  unsigned long long *ev_raw;
  uint32_t ev_cap;
  uint32_t *ev_counts;
  // GIANT: as in SkmArgs — the work items of the giant bins (the first n_giant tickets), the records above which a batch skips a bin
  const uint2 *giants;
  uint32_t n_giant, giant_limit;
};

// LV: the levels of the thermometer per neighbouring base — 2 (min count <= 2), or 4 (s1_skm_max_m, min count 3 and 4: base in front x
// bits 4x .. 4x + 3, base behind x bits 16 + 4x .. 19 + 4x of chw, bit l of a field = "seen l + 1 times"; all 32 bits, the two flags written
// over the word after the walk as in the other form).  LV 4 is built for G 2, one GPU, bins whole; the LV 2 forms are the code they were
template <bool TAGS, int G, bool EVENTS = false, bool GIANT = false, int LV = 2>
__global__ __launch_bounds__(kSkmThreads) void k_count_skm(SkmSrcs srcs, CountSkmArgs a, uint32_t *__restrict__ ticket) {
  static_assert(LV == 2 || (LV == 4 && G == 2 && !EVENTS && !GIANT), "four levels: one GPU, bins whole");
  constexpr int NT = kSkmThreads, NSLOT = 1 << kSkmLogSlots, W = NSLOT / NT;
  constexpr unsigned long long kEmpty = ~0ull;  // never a key: the bits below the (k+1)-mer are zero
  __shared__ unsigned long long keys[NSLOT];
  __shared__ uint32_t cnts[NSLOT];
  __shared__ uint32_t chw[NSLOT];  // base in front x: bit 2x seen once, 2x + 1 seen twice; base behind x: bits 8 + 2x, 9 + 2x (LV 4: four bits a base, above); after the walk: flags << 30
  __shared__ uint32_t lhist[kSegHist];
  __shared__ unsigned long long heads[kSkmThreads / kWave][8];
  __shared__ uint32_t s_bad, s_nclaimed, s_edge_cur, s_flagged, s_tk;
  __shared__ uint64_t s_lo[kSkmSrcMax][kSkmBatch + 1];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  const uint32_t le_lo = lane >= 31 ? 0xFFFFFFFFu : (2u << lane) - 1u, le_hi = lane < 32 ? 0u : (lane == 63 ? 0xFFFFFFFFu : (2u << (lane - 32)) - 1u);
  const int k = a.k, K1 = k + 1;
  const uint32_t m = a.m;
  const uint64_t kmask = ~0ull << (64 - 2 * K1);
  const int n_src = srcs.n;
  unsigned long long *const eout = a.edges_raw + (size_t)blockIdx.x * a.edges_cap;
  for (int i = tid; i < NSLOT; i += NT) {
    keys[i] = kEmpty;
    cnts[i] = 0;
    chw[i] = 0;
  }
  for (int i = tid; i < kSegHist; i += NT) lhist[i] = 0;
  if (tid == 0) {
    s_bad = 0;
    s_nclaimed = 0;
    s_edge_cur = 0;
    s_flagged = 0;
  }
  __syncthreads();
  unsigned long long n_dist_all = 0;

  // One window of the trip, dealt to this lane: window g of the wavefront's records belongs to the record whose run starts at or before g
  // (bitmap of run heads, hv) and comes over with seven shuffles.
  struct Win {
    bool valid, fwd;
    unsigned long long key;
    unsigned pv, nx;   // base in front / behind in the key's orientation (4: none)
    uint32_t pos;      // low word of the window's position
    uint8_t tag;
  };
  struct Trip {
    uint32_t T, start, pd, hv_lo, hv_hi, bh, bl, qh, ql, meta;
    uint8_t tag;
  };
  auto open_trip = [&](const uint4 &r, bool in) -> Trip {
    Trip t;
    const uint32_t len = in ? ((r.x >> 5) & 7u) + 1u : 0u;
    const uint32_t incl = wave_inclusive_sum(len);
    t.T = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
    t.start = incl - len;
    if (lane < 8) heads[wv][lane] = 0ull;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (len) atomicOr(&heads[wv][t.start >> 6], 1ull << (t.start & 63u));
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const unsigned long long hv = __hip_atomic_load(&heads[wv][lane & 7], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    t.hv_lo = (uint32_t)hv;
    t.hv_hi = (uint32_t)(hv >> 32);
    const uint64_t rec_b = ((uint64_t)r.y << 32) | r.z;
    const uint64_t rec_r = rc64(rec_b, 32);
    t.bh = r.y, t.bl = r.z, t.qh = (uint32_t)(rec_r >> 32), t.ql = (uint32_t)rec_r;
    t.pd = r.w - t.start;
    t.meta = (r.x & 0xFFu) | (len << 8);  // flags, and the run's length for its last window
    t.tag = TAGS ? (uint8_t)(r.x >> 28) : (uint8_t)0;
    return t;
  };
  auto deal = [&](const Trip &t, int c, uint32_t &cbase_m1) -> Win {
    Win w;
    const uint32_t g = (uint32_t)(c * kWave) + (uint32_t)lane;
    const uint32_t w_lo = (uint32_t)__builtin_amdgcn_readlane((int)t.hv_lo, c), w_hi = (uint32_t)__builtin_amdgcn_readlane((int)t.hv_hi, c);
    const uint32_t o = cbase_m1 + (uint32_t)__builtin_popcount(w_lo & le_lo) + (uint32_t)__builtin_popcount(w_hi & le_hi);
    cbase_m1 += (uint32_t)__builtin_popcount(w_lo) + (uint32_t)__builtin_popcount(w_hi);
    const uint32_t xbh = __shfl(t.bh, (int)o, kWave), xbl = __shfl(t.bl, (int)o, kWave);
    const uint32_t xqh = __shfl(t.qh, (int)o, kWave), xql = __shfl(t.ql, (int)o, kWave);
    const uint32_t so = __shfl(t.start, (int)o, kWave), pdo = __shfl(t.pd, (int)o, kWave), mo = __shfl(t.meta, (int)o, kWave);
    const uint32_t j = g - so;
    const uint64_t B = ((uint64_t)xbh << 32) | xbl, R = ((uint64_t)xqh << 32) | xql;
    const uint64_t x = (B << (2 * (1 + j))) & kmask;                 // the window: slots 1 + j .. j + k + 1 of the record
    const uint64_t rcx = (R << (2 * (32 - 1 - K1 - j))) & kmask;     // its reverse complement: a sub-window of the record's
    const unsigned pb = (unsigned)(B >> (62 - 2 * j)) & 3u, nb = (unsigned)(B >> (60 - 2 * K1 - 2 * j)) & 3u;
    const unsigned prev = j == 0 && (mo & 16u) ? kSentinel : pb, next = j + 1 == (mo >> 8) && (mo & 8u) ? kSentinel : nb;
    bool strand;
    w.key = skm_count_key(x, rcx, &strand);
    w.fwd = !strand;
    w.pv = strand ? comp_or_sentinel(next) : prev;
    w.nx = strand ? comp_or_sentinel(prev) : next;
    w.pos = pdo + g;
    if constexpr (TAGS) w.tag = (uint8_t)(__shfl((uint32_t)t.tag, (int)o, kWave) + (w.pos < pdo + so ? 1u : 0u));
    else w.tag = 0;
    w.valid = g < t.T;
    return w;
  };
  auto slot_of = [&](unsigned long long key) -> uint32_t {
    const uint32_t klo = (uint32_t)key, khi = (uint32_t)(key >> 32);
    return ((klo * 0x9E3779B1u) ^ (khi * 0x85EBCA6Bu)) >> (32 - kSkmLogSlots);
  };
  auto in_round = [&](unsigned long long key, uint32_t sub, uint32_t rj) -> bool {
    if (!sub) return true;
    const uint32_t klo = (uint32_t)key, khi = (uint32_t)(key >> 32);
    return skm_in_round(skm_mix2((klo * 0xC2B2AE35u) ^ (khi * 0x27D4EB2Fu)), sub, rj);
  };

  for (;;) {
    if (tid == 0) s_tk = atomicAdd(ticket, 1u);
    __syncthreads();
    // GIANT: the first tickets are slices of giant bins — the bin alone in the batch, its rounds from (sub0, rj0) on
    uint32_t sub0 = 0, rj0 = 0;
    bool slice = false;
    if constexpr (GIANT) slice = s_tk < a.n_giant;  // (uniform)
    if (slice) {
      // (the item is the same in every lane: kept in scalar registers through the rounds)
      const uint2 item = a.giants[(uint32_t)__builtin_amdgcn_readfirstlane((int)s_tk)];
      const uint32_t depth_at = (uint32_t)__builtin_amdgcn_readfirstlane((int)item.y);
      sub0 = depth_at >> 16;
      rj0 = depth_at & 0xFFFFu;
      if (tid <= kSkmBatch) s_lo[0][tid] = srcs.bounds[0][item.x + (tid ? 1u : 0u)];
    } else {
      const uint64_t bin0 = (uint64_t)a.bin_lo + (uint64_t)(s_tk - (GIANT ? a.n_giant : 0u)) * kSkmBatch;
      if (bin0 >= a.bin_hi) break;
      if (tid < n_src * (kSkmBatch + 1)) {
        const int q = tid / (kSkmBatch + 1), x = tid - q * (kSkmBatch + 1);
        s_lo[q][x] = srcs.bounds[q][min(bin0 + x, (uint64_t)a.bin_hi)];
      }
    }
    __syncthreads();
    for (int bb = 0; bb < kSkmBatch; ++bb) {
      bool any = false;
      for (int q = 0; q < n_src; ++q) any = any || s_lo[q][bb] != s_lo[q][bb + 1];
      if (!any) continue;
      if constexpr (GIANT)
        if (!slice && s_lo[0][bb + 1] - s_lo[0][bb] > (uint64_t)a.giant_limit) continue;  // (uniform) a giant bin inside a batch: its slices are tickets of their own
      uint32_t sub = sub0, rj = rj0;  // (a slice of a giant bin: the rounds from (sub0, rj0) on; skm_giant.h)
      for (;;) {
        uint32_t seen = 0;
        // A: insert
        for (int q = 0; q < n_src; ++q) {
          const uint64_t lo = s_lo[q][bb], hi = s_lo[q][bb + 1];
          const uint4 *__restrict__ recs = srcs.ptr[q];
          for (uint64_t base = lo; base < hi; base += NT) {
            const bool in = base + tid < hi;
            const uint4 r = in ? recs[base + tid] : make_uint4(0u, 0u, 0u, 0u);
            if (seen > a.max_fill) continue;
            const Trip t = open_trip(r, in);
            uint32_t claims = 0;
            // (the slot found — the key's own, or a free one claimed: count the window and the bases either side of it)
            auto settle = [&](unsigned long long old, unsigned long long key, uint32_t hh, unsigned pv, unsigned nx) -> bool {
              if (old != kEmpty && old != key) return false;
              atomicAdd(&cnts[hh], 1u);
              if (old == kEmpty) ++claims;
              if constexpr (LV == 4) {
                // an occurrence climbs its base's field until it sets a bit that was clear: every occurrence sets ONE bit, whatever the
                // order the lanes arrive in, so bit l is set once l + 1 occurrences have been here (at most four operations; a fifth
                // occurrence finds the field full and leaves it)
                uint32_t add = (pv < 4 ? 1u << (4 * pv) : 0u) | (nx < 4 ? 1u << (16 + 4 * nx) : 0u);  // ('$' counts for nothing)
#pragma unroll
                for (int l = 0; l < LV; ++l) {
                  if (!add) break;
                  const uint32_t o = atomicOr(&chw[hh], add);
                  add = (o & add & 0x77777777u) << 1;  // the bits that were set already: one level up (not out of the field)
                }
              } else {
              const uint32_t add1 = (pv < 4 ? 1u << (2 * pv) : 0u) | (nx < 4 ? 1u << (8 + 2 * nx) : 0u);  // ('$' counts for nothing)
              if (add1) {
                const uint32_t o = atomicOr(&chw[hh], add1);
                const uint32_t again = ((o & add1) << 1) & ~o;  // a base seen before and now again: seen twice
                if (again) atomicOr(&chw[hh], again);
              }
              }
              return true;
            };
            uint32_t cbase_m1 = 0xFFFFFFFFu;
#pragma unroll
            for (int grp = 0; grp < 8 / G; ++grp) {  // G chunks of 64 windows share one round of compare-and-swaps and one retry loop
              if ((uint32_t)(grp * G * kWave) >= t.T) break;  // (uniform)
              Win w[G];
              unsigned long long old1[G];
              uint32_t h1[G], mine = 0;
#pragma unroll
              for (int u = 0; u < G; ++u) {
                w[u] = deal(t, grp * G + u, cbase_m1);
                const bool mn = w[u].valid && in_round(w[u].key, sub, rj);
                mine |= mn ? 1u << u : 0u;
                h1[u] = slot_of(w[u].key);
              }
              if (a.probe_limit <= 0) {
                if (mine) s_bad = 1;
                mine = 0;
              }
#pragma unroll
              for (int u = 0; u < G; ++u) {
                old1[u] = kEmpty;
                if ((mine >> u) & 1u) old1[u] = atomicCAS(&keys[h1[u]], kEmpty, w[u].key);
              }
              bool has = false;
              unsigned long long pk = 0;
              uint32_t ph = 0;
              unsigned ppv = 0, pnx = 0;
#pragma unroll
              for (int u = 0; u < G; ++u) {
                if ((mine >> u) & 1u) {
                  if (!settle(old1[u], w[u].key, h1[u], w[u].pv, w[u].nx)) {
                    uint32_t hh = (h1[u] + 1) & (NSLOT - 1);
                    if (!has) {
                      has = true;
                      pk = w[u].key, ph = hh, ppv = w[u].pv, pnx = w[u].nx;
                    } else {
                      int n = 0;
                      while (!settle(atomicCAS(&keys[hh], kEmpty, w[u].key), w[u].key, hh, w[u].pv, w[u].nx)) {
                        hh = (hh + 1) & (NSLOT - 1);
                        if (++n >= a.probe_limit) {
                          s_bad = 1;
                          break;
                        }
                      }
                    }
                  }
                }
              }
              int turns = 0;
              while (__ballot(has)) {
                if (has) {
                  if (settle(atomicCAS(&keys[ph], kEmpty, pk), pk, ph, ppv, pnx)) has = false;
                  else ph = (ph + 1) & (NSLOT - 1);
                }
                if (++turns > a.probe_limit) {  // (uniform: every lane counts the same turns)
                  if (has) s_bad = 1;
                  break;
                }
              }
            }
            {
              const uint32_t c = wave_sum(claims);
              if (lane == 0 && c) atomicAdd(&s_nclaimed, c);
              seen = __hip_atomic_load(&s_nclaimed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              seen = (uint32_t)__builtin_amdgcn_readfirstlane((int)seen);
            }
          }
        }
        __syncthreads();  // the table is complete
        const bool bad = s_bad != 0 || s_nclaimed > a.max_fill;
        uint32_t nsub, nrj;
        bool done, give_up;
        skm_next_round(sub, rj, bad, sub0, rj0, &nsub, &nrj, &done, &give_up);
        if (give_up && tid == 0) atomicOr(a.err, 1u);
        // C: one walk over the table — per distinct (k+1)-mer: histogram, has_in / has_out from the seen-twice (m = 2) or seen-once (m = 1)
        // bits, the packed edge of a solid key -> this workgroup's region; a solid key without an in- or out-edge keeps two flag bits
        unsigned long long wk[W];
        uint32_t wc[W], wf[W];
#pragma unroll
        for (int it = 0; it < W; ++it) {
          const int sl = it * NT + tid;
          wk[it] = keys[sl];
          wc[it] = cnts[sl];
          wf[it] = chw[sl];
        }
        [[maybe_unused]] const uint32_t lvl = m >= 2 ? 0xAAu : 0x55u;
        uint32_t solid_bits = 0, n_dist = 0;
        bool any_flag = false;
#pragma unroll
        for (int it = 0; it < W; ++it) {
          uint32_t fb = 0;
          if (wk[it] != kEmpty && !bad) {
            ++n_dist;
            const uint32_t cnt = wc[it];
            const uint32_t hb = cnt > MHX_MAX_MUL ? (uint32_t)MHX_MAX_MUL : cnt;
            if (hb < kSegHist) atomicAdd(&lhist[hb], 1u);
            else atomicAdd(&a.hist[hb], 1ull);
            if (cnt >= m) {
              solid_bits |= 1u << it;
              bool has_in, has_out;
              if constexpr (LV == 4) {  // bit m - 1 of every field
                has_in = (wf[it] & (0x1111u << (m - 1u))) != 0;
                has_out = (wf[it] & (0x11110000u << (m - 1u))) != 0;
              } else {
                has_in = (wf[it] & lvl) != 0, has_out = ((wf[it] >> 8) & lvl) != 0;
              }
              fb = (has_in ? 0u : 1u) | (has_out ? 0u : 2u);
              any_flag = any_flag || fb != 0;
            }
          }
          chw[it * NT + tid] = fb << 30;
        }
        n_dist_all += n_dist;
        if (__ballot(any_flag) && lane == 0) s_flagged = 1;
        {  // the solid keys' packed edges (PackEdge, kmer_counter.cpp:32-52: multiplicity in the low 16 bits) -> the region, from its front
          const uint32_t n_e = (uint32_t)__builtin_popcount(solid_bits);
          const uint32_t incl = wave_inclusive_sum(n_e);
          const uint32_t tot = __shfl(incl, kWave - 1, kWave);
          if (tot) {
            uint32_t ebase = 0;
            if (lane == 0) ebase = atomicAdd(&s_edge_cur, tot);
            ebase = __shfl(ebase, 0, kWave);
            if (ebase + tot > a.edges_cap) {
              if (lane == 0) atomicOr(a.err, 1u);
            } else {
              uint32_t at = ebase + incl - n_e;
#pragma unroll
              for (int it = 0; it < W; ++it)
                if ((solid_bits >> it) & 1u) {
                  const uint32_t mul = wc[it] > MHX_MAX_MUL ? (uint32_t)MHX_MAX_MUL : wc[it];
                  eout[at++] = wk[it] | mul;
                }
            }
          }
        }
        __syncthreads();  // the flags are in the slots
        if (s_flagged && !bad) {  // the windows of the flagged keys: first_0_out / last_0_in of their reads (kmer_counter.cpp:307-368)
          for (int q = 0; q < n_src; ++q) {
            const uint64_t lo = s_lo[q][bb], hi = s_lo[q][bb + 1];
            const uint4 *__restrict__ recs = srcs.ptr[q];
            for (uint64_t base = lo; base < hi; base += NT) {
              const bool in = base + tid < hi;
              const uint4 r = in ? recs[base + tid] : make_uint4(0u, 0u, 0u, 0u);
              const Trip t = open_trip(r, in);
              uint32_t cbase_m1 = 0xFFFFFFFFu;
              for (uint32_t c = 0; c * kWave < t.T; ++c) {
                const Win w = deal(t, (int)c, cbase_m1);
                uint32_t f = 0;
                if (w.valid && in_round(w.key, sub, rj)) {  // (a key of another round is not in the table)
                  uint32_t h = slot_of(w.key);
                  while (keys[h] != w.key) h = (h + 1) & (NSLOT - 1);
                  f = chw[h] >> 30;
                }
                if constexpr (EVENTS) {
                  // the same as events for the ranks that hold the reads: one reservation per wavefront in this workgroup's region
                  const uint32_t ne = (f & 1u) + (f >> 1);
                  const uint32_t incl = wave_inclusive_sum(ne);
                  const uint32_t tot = __shfl(incl, kWave - 1, kWave);
                  if (tot) {  // (uniform)
                    uint32_t ebase = 0;
                    if (lane == 0) ebase = atomicAdd(&a.ev_counts[blockIdx.x], tot);
                    ebase = __shfl(ebase, 0, kWave);
                    if (ebase + tot > a.ev_cap || ebase + tot < ebase) {
                      if (lane == 0) atomicOr(a.err, 2u);
                    } else {
                      const unsigned long long abs = ((unsigned long long)w.tag << 32) | w.pos;
                      unsigned long long *const ev = a.ev_raw + (size_t)blockIdx.x * a.ev_cap;
                      uint32_t at = ebase + incl - ne;
                      if (f & 1u) ev[at++] = (abs << 1) | (w.fwd ? 0ull : 1ull);
                      if (f & 2u) ev[at] = (abs << 1) | (w.fwd ? 1ull : 0ull);
                    }
                  }
                } else if (f) {
                  // no in-edge (f & 1): strand 0 -> last_0_in = max(off), strand 1 -> first_0_out = min(off + 1); no out-edge (f & 2): the roles swap
                  const uint64_t abs = ((uint64_t)w.tag << 32) | w.pos;
                  const uint64_t rid = seq_of_offset(a.c_start, a.c_n_seqs, a.c_fixed_len, abs);
                  const uint32_t off = (uint32_t)(abs - (a.c_fixed_len ? rid * a.c_fixed_len : a.c_start[rid]));
                  if (f & 1u) {
                    if (w.fwd) atomicMax(&a.last_0_in_p1[rid], off + 1);
                    else atomicMin(&a.first_0_out[rid], off + 1);
                  }
                  if (f & 2u) {
                    if (w.fwd) atomicMin(&a.first_0_out[rid], off + 1);
                    else atomicMax(&a.last_0_in_p1[rid], off + 1);
                  }
                }
              }
            }
          }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < W; ++it) {
          const int sl = it * NT + tid;
          keys[sl] = kEmpty;
          cnts[sl] = 0;
          chw[sl] = 0;
        }
        if (tid == 0) {
          s_bad = 0;
          s_nclaimed = 0;
          s_flagged = 0;
        }
        __syncthreads();
        sub = nsub;
        rj = nrj;
        if (done) break;
      }
    }
  }
  n_dist_all = wave_sum(n_dist_all);
  if (lane == 0 && n_dist_all) atomicAdd(a.ctr + 4, n_dist_all);
  __syncthreads();
  for (int i = tid; i < kSegHist; i += NT)
    if (lhist[i]) atomicAdd(&a.hist[i], (unsigned long long)lhist[i]);
  if (tid == 0) a.edges_counts[blockIdx.x] = s_edge_cur < a.edges_cap ? s_edge_cur : a.edges_cap;
}

// ---- host ----
// s1_skm_max_m: the largest min count served on super-k-mer records on ONE GPU — 2, or 3 / 4 with the LOOK form of k_s1_skm and the LV 4 form
// of k_count_skm (values outside 2..4: the nearest)
uint32_t s1_skm_max_m(const mhx_ctx *c) { return (uint32_t)std::min<long long>(std::max<long long>(c->opt<Opt::s1_skm_max_m>(), 2), 4); }

bool s1_skm_applies(const mhx_ctx *c, uint32_t k, uint32_t m, int want_mercy) {
  const SeqSet &s = c->seqs;
  const long long knob = c->opt<Opt::s1_skm>();
  if (!knob || want_mercy || c->global_bases || c->n_parts > 1 || c->filter_on || c->accumulate || c->pos_base) return false;
  if (k < 19 || k > 22 || m < 1 || m > s1_skm_max_m(c)) return false;
  if (!s.n_seqs || s.max_len < k + 1 || (s.n_bases >> 36)) return false;
  // (reads of several lengths: every read takes the blocks of the longest — while at least s1_var_min_fill per cent of them hold windows)
  if (!s.fixed_len && (double)s.n_bases * 100.0 < (double)c->opt<Opt::s1_var_min_fill>() * (double)s.n_seqs * s.max_len) return false;
  const char *e = getenv("MHX_S1_MARK");
  if (e && strcmp(e, "nonsolid")) return false;  // (a caller that asks for another polarity of the marks, or atomics into the bitmap)
  const uint64_t n_win = s.n_bases > s.n_seqs * (uint64_t)k ? s.n_bases - s.n_seqs * (uint64_t)k : 0;
  return knob >= 2 || n_win >= (uint64_t)c->opt<Opt::s1_skm_min_windows>();
}

// several GPUs (comm.hip dist_s1_skm): this rank's say — the same shape with a global layout; at most kSkmSrcMax ranks (one source per sender)
bool s1_skm_dist_applies(const mhx_ctx *c, uint32_t k, uint32_t m) {
  const SeqSet &s = c->seqs;
  if (!c->opt<Opt::s1_skm>() || !c->opt<Opt::dist_skm>() || !c->global_bases || c->n_parts > kSkmSrcMax || c->filter_on || c->accumulate) return false;
  if (k < 19 || k > 22 || m < 1 || m > 2 || (c->global_bases >> 36)) return false;
  if (!s.n_seqs || s.max_len < k + 1) return false;
  if (!s.fixed_len && (double)s.n_bases * 100.0 < (double)c->opt<Opt::s1_var_min_fill>() * (double)s.n_seqs * s.max_len) return false;
  if (getenv("MHX_S1_MARK") || !c->opt<Opt::dist_sparse_marks>()) return false;
  return s1_skm_passes(c, k) == 1;
}

// make the records, order them by bin, find the bins.  -> false: gave up (more records than the array was sized for, or a bin that one
// workgroup should not stream alone: low-complexity reads) — nothing published
int s1_skm_passes(const mhx_ctx *c, uint32_t k) {
  // the two record arrays of a pass together take s1_skm_pass_gb (hipMalloc costs per byte on this driver — seconds per 100 GB — while one
  // more pass costs one more scan of the reads by k_skm_make: 28 ms at 100 M reads); s1_skm_passes forces a count (tests)
  const SeqSet &s = c->seqs;
  if (const long long f = c->opt<Opt::s1_skm_passes>()) return (int)std::min<long long>(64, std::max<long long>(1, f));
  const uint64_t n_win = s.n_bases > s.n_seqs * (uint64_t)k ? s.n_bases - s.n_seqs * (uint64_t)k : 0;
  const double need = (double)n_win * (double)std::max<long long>(c->opt<Opt::s1_skm_cap_pct>(), 1) / 100.0 * 32.0;
  const double budget = (double)std::max<long long>(c->opt<Opt::s1_skm_pass_gb>(), 1) * 1e9;
  return (int)std::min(64.0, std::max(1.0, std::ceil(need / budget)));
}

bool s1_skm_front(mhx_ctx *c, uint32_t k, SkmFront *f, int pass, int n_passes, int bin_bits_agreed, bool for_count, bool bins_whole) {
  SeqSet &s = c->seqs;
  hipStream_t st = c->stream;
  const bool var = s.fixed_len == 0;
  const uint32_t L = var ? s.max_len : s.fixed_len, bpr = (L - k + kSkmC - 1) / kSkmC;
  const uint64_t n_blocks = s.n_seqs * (uint64_t)bpr;
  const uint64_t n_win = var ? (s.n_bases > s.n_seqs * (uint64_t)k ? s.n_bases - s.n_seqs * (uint64_t)k : 0) : s.n_seqs * (uint64_t)(L - k);  // (var: an estimate)
  // the array: 0.284 records per window of random sequence at m = k - 8 (fewer in repeats); s1_skm_cap_pct per cent of the windows
  // (a pass of several: its share of the bins, which the hash fills evenly, and 15 % on top)
  const uint64_t cap_all = n_win * (uint64_t)std::max<long long>(c->opt<Opt::s1_skm_cap_pct>(), 1) / 100;
  const uint64_t cap = std::max<uint64_t>(n_passes > 1 ? cap_all / n_passes + cap_all / n_passes * 15 / 100 : cap_all, 1u << 16);
  // bins: ~5000 records each (20 000 windows: what the table of one workgroup takes in one round) — 2^16 up to 14 M reads of 150 bases,
  // up to 2^20 and a third sort pass beyond
  int bin_bits = kSkmMinBinBits;
  while (bin_bits < kSkmMaxBinBits && (double)n_win * 0.29 / (double)(1ull << bin_bits) > 8192.0) ++bin_bits;
  if (const long long fb = c->opt<Opt::s1_skm_bin_bits>()) bin_bits = (int)std::min<long long>(kSkmMaxBinBits, std::max<long long>(8, fb));
  if (bin_bits_agreed > 0) bin_bits = bin_bits_agreed;  // (several GPUs: the ranks made it from the size of the whole job)
  // (bits 0..7 of the first word are zero in every record: all passes may rank with LDS atomics)
  std::vector<SortPass> passes;
  for (int lo = 0; lo < bin_bits; lo += 8) passes.push_back(SortPass{8 + lo, std::min(8, bin_bits - lo), 0, 0, 0});
  // s1_skm_split: k_skm_make puts every record into the range of its bin's low digit — the first sort pass done where the records are made —
  // and the sort starts at the second digit, reading the ranges in order.  Needs a second pass (the group-by cannot read an array with holes);
  // a range that overflows (a skewed input: the ranges hold the even share of hash-uniform bins and the array's slack) makes the records again, unsplit
  const std::vector<SortPass> passes_rest(passes.begin() + (passes.empty() ? 0 : 1), passes.end());
  bool split = c->opt<Opt::s1_skm_split>() != 0 && passes.size() >= 2 && sort_takes_split_first_pass(c, passes_rest);
  const uint64_t cap_split = std::max<uint64_t>(cap, 1u << 20), range_cap = cap_split / 256 / kSortSplitUnit * kSortSplitUnit;
  const uint64_t cap_alloc = split ? cap_split : cap;
  uint4 *buf_a = c->ws("items_a", cap_alloc * 16 + 64).as<uint4>();
  uint4 *buf_b = c->ws("items_b", cap_alloc * 16 + 64).as<uint4>();
  unsigned long long *cursor = c->ws("skm_cursor", 64).as<unsigned long long>();
  uint32_t *err = reinterpret_cast<uint32_t *>(cursor + 1);
  uint32_t *max_bin = err + 1;
  unsigned long long *split_cur = split ? c->ws("skm_split_cursors", (256 + 257) * 8).as<unsigned long long>() : nullptr;
  const uint32_t stage_n = (uint32_t)std::min<long long>(std::max<long long>(c->opt<Opt::s1_skm_split_stage>(kSkmStage), 0), kSkmStage);
  unsigned long long *pre_hist = c->ws("sort_pre_hist", (size_t)kMaxFusedPasses * 256 * 8).as<unsigned long long>();
  constexpr int NT = 512, J = 2;
  const uint64_t cus = c->n_cus > 0 ? (uint64_t)c->n_cus : 256;
  // (s1_skm_make_grid: fewer workgroups, each with several trips over the blocks — tests on libraries of a few trips in all)
  const long long grid_knob = c->opt<Opt::s1_skm_make_grid>();
  const unsigned grid = (unsigned)std::min<uint64_t>(div_ceil(n_blocks, (uint64_t)NT * J), grid_knob > 0 ? (uint64_t)grid_knob : cus * 8);
  const uint32_t n_bins = 1u << bin_bits;
  const uint32_t bin_lo = (uint32_t)((uint64_t)n_bins * pass / n_passes), bin_hi = (uint32_t)((uint64_t)n_bins * (pass + 1) / n_passes);
  // homopolymer windows are counted beside the records on one GPU (several GPUs, stage 1: they stay in the records; a job with many gives the
  // path up.  count's tallies carry no position: on several GPUs the ranks add theirs up, comm.hip dist_count_skm)
  unsigned long long *hp = nullptr;
  if ((!c->global_bases || for_count) && c->opt<Opt::s1_skm_hp>()) hp = c->ws("skm_hp", 512).as<unsigned long long>();  // [0..3] stage 1: windows per class, a position each; [8 + 16 class + ..] count: windows, bases in front, bases behind
  // s1_skm_rep: the windows of period <= 4 join them (k_skm_make<.., REP>) — looked at only where the homopolymer windows are counted aside,
  // on one GPU; the table sits behind the homopolymer counters
  const bool rep = hp && !c->global_bases && c->n_parts <= 1 && c->opt<Opt::s1_skm_rep>() != 0;
  if (rep) hp = c->ws("skm_hp", (size_t)(kSkmRepAt + kSkmRepN * 9) * 8).as<unsigned long long>();
  // (s1_skm_rep_slots: slots of a workgroup's LDS hash in use — tests: few or none, and the entries go to the global table from the registers)
  const unsigned long long rep_slots = (unsigned long long)std::min<long long>(std::max<long long>(c->opt<Opt::s1_skm_rep_slots>(), 0), 64);
  unsigned long long hp_init[48] = {0};
  hp_init[2] = hp_init[3] = ~0ull;
  unsigned long long h[4] = {0, 0, 0, 0};
  std::vector<unsigned long long> h_dh(passes.size() * 256), h_fill(256);
#define MHX_MAKE(VARV, COUNTV, SPLITV) MHX_MAKE_R(VARV, COUNTV, SPLITV, false)
#define MHX_MAKE_R(VARV, COUNTV, SPLITV, REPV)                                                                                                                           \
  hipLaunchKernelGGL((k_skm_make<NT, J, VARV, COUNTV, SPLITV, REPV>), dim3(grid), dim3(NT), 0, st, s.words.as<uint32_t>(), s.start.as<uint64_t>(), L, bpr, n_blocks, (int)k, \
                     bin_bits, bin_lo, bin_hi, pass == 0 ? 1 : 0, c->pos_base, hp, buf_a, (unsigned long long)cap, cursor, err, pre_hist,                            \
                     (unsigned long long)range_cap, split_cur, stage_n)
  // everything the kernel counts starts from zero — also when the records are made a second time
  auto make = [&](bool split_now) {
    MHX_HIP(hipMemsetAsync(cursor, 0, 64, st));
    MHX_HIP(hipMemsetAsync(pre_hist, 0, (size_t)3 * 256 * 8, st));
    if (split_now) MHX_HIP(hipMemsetAsync(split_cur, 0, 256 * 8, st));
    if (hp && pass == 0) MHX_HIP(hipMemcpyAsync(hp, hp_init, sizeof hp_init, hipMemcpyHostToDevice, st));
    if (rep && pass == 0) {  // counts from zero, positions (stage 1: the second kSkmRepN values) from the largest
      MHX_HIP(hipMemsetAsync(hp + kSkmRepAt, 0, (size_t)kSkmRepN * 9 * 8, st));
      MHX_HIP(hipMemcpyAsync(hp + kSkmRepAt - 1, &rep_slots, 8, hipMemcpyHostToDevice, st));
      if (!for_count) MHX_HIP(hipMemsetAsync(hp + kSkmRepAt + kSkmRepN, 0xFF, (size_t)kSkmRepN * 8, st));
    }
    MHX_LAUNCH(c, for_count ? "count_skm_make" : "s1_skm_make", (double)s.n_bases / 4 + (double)n_win * 16 / 3.5, {
      if (rep && split_now) {
        if (var && for_count) MHX_MAKE_R(true, true, true, true);
        else if (var) MHX_MAKE_R(true, false, true, true);
        else if (for_count) MHX_MAKE_R(false, true, true, true);
        else MHX_MAKE_R(false, false, true, true);
      } else if (rep) {
        if (var && for_count) MHX_MAKE_R(true, true, false, true);
        else if (var) MHX_MAKE_R(true, false, false, true);
        else if (for_count) MHX_MAKE_R(false, true, false, true);
        else MHX_MAKE_R(false, false, false, true);
      } else if (split_now) {
        if (var && for_count) MHX_MAKE(true, true, true);
        else if (var) MHX_MAKE(true, false, true);
        else if (for_count) MHX_MAKE(false, true, true);
        else MHX_MAKE(false, false, true);
      } else {
        if (var && for_count) MHX_MAKE(true, true, false);
        else if (var) MHX_MAKE(true, false, false);
        else if (for_count) MHX_MAKE(false, true, false);
        else MHX_MAKE(false, false, false);
      }
    });
    MHX_HIP(hipMemcpyAsync(h, cursor, 32, hipMemcpyDeviceToHost, st));
    MHX_HIP(hipMemcpyAsync(h_dh.data(), pre_hist, h_dh.size() * 8, hipMemcpyDeviceToHost, st));
    if (split_now) MHX_HIP(hipMemcpyAsync(h_fill.data(), split_cur, 256 * 8, hipMemcpyDeviceToHost, st));
    MHX_HIP(hipStreamSynchronize(st));
  };
  make(split);
  if (split && ((uint32_t)h[1] & 2u)) {  // a range overflowed: the records again through the one cursor, and all passes
    split = false;
    make(false);
  }
#undef MHX_MAKE
#undef MHX_MAKE_R
  if (split) {  // (no cursor of all records: they are what the ranges hold)
    h[0] = 0;
    for (int d = 0; d < 256; ++d) h[0] += h_fill[d];
  }
  f->n_records = 0;
  f->hp = hp;
  f->rep = rep;
  f->giants = nullptr;
  f->n_giant_items = f->giant_limit = f->giant_bins = f->giant_largest = 0;
  f->why = nullptr;
  if ((uint32_t)h[1] != 0 || h[0] > cap) return false;
  const uint64_t n = h[0];
  // s1_skm_giant: a bin over the limit is worked in slices by several workgroups (skm_giant.h) instead of costing the job the path — one GPU
  // (bins_whole: min count 3 and 4 — the forms of the group-by that serve them take a bin whole; one beyond s1_skm_max_bin gives the job up)
  const bool giant = !bins_whole && !c->global_bases && c->n_parts <= 1 && c->opt<Opt::s1_skm_giant>() != 0;
  SkmGiantKnobs gk;
  gk.max_records = (uint64_t)std::max<long long>(c->opt<Opt::s1_skm_giant_max>(), 1);
  gk.keys = (uint64_t)std::max<long long>(c->opt<Opt::s1_skm_giant_keys>(), 1);
  gk.work_pct = (uint64_t)std::max<long long>(c->opt<Opt::s1_skm_giant_work_pct>(), 0);
  gk.slices = (uint64_t)std::min<long long>(std::max<long long>(c->opt<Opt::s1_skm_giant_slices>(), 0), 1 << kSkmGiantMaxDepth);
  {  // a bin far over the limit shows in the digit histograms already — one value of EVERY digit stands out by its records: no need to
     // order the records to find it (low-complexity reads: 1 % of (AC)n reads put 1.7 M records behind one minimizer)
    const uint64_t n_bins_pass = std::max<uint64_t>(1, ((1ull << bin_bits) + n_passes - 1) / n_passes);
    // (s1_skm_giant: a bin over the limit is served — up to s1_skm_giant_max records, which is what must still be found here)
    const uint64_t limit = giant ? gk.max_records : std::max<uint64_t>((uint64_t)c->opt<Opt::s1_skm_max_bin>(), 16 * (n / n_bins_pass + 1));
    bool all = n > 0;
    uint64_t smallest_excess = ~0ull;
    for (size_t p = 0; p < passes.size() && all; ++p) {
      const uint64_t vals = 1ull << passes[p].bits;
      uint64_t mx = 0;
      for (uint64_t d = 0; d < vals; ++d) mx = std::max<uint64_t>(mx, h_dh[p * 256 + d]);
      const uint64_t mean = n / std::max<uint64_t>(1, (p + 1 == passes.size() && n_passes > 1) ? std::max<uint64_t>(1, vals / n_passes) : vals);
      const uint64_t excess = mx > mean ? mx - mean : 0;
      smallest_excess = std::min(smallest_excess, excess);
      all = excess >= limit + limit / 2;  // (1.5 x: the values of a digit differ by a few per cent of their mean — 256 bins each — far below the limit)
    }
    if (all) {
      f->n_records = n;
      f->max_bin = (uint32_t)std::min<uint64_t>(smallest_excess, 0xFFFFFFFFu);
      if (giant) f->why = "beyond s1_skm_giant_max";
      return false;
    }
  }
  const std::vector<SortPass> &sort_passes = split ? passes_rest : passes;
  SortPrep prep;  // (radix_sort: no histogram read of its own)
  prep.buf = buf_a;
  prep.n = n;
  prep.hist_passes = (int)sort_passes.size();
  prep.hist_sig = passes_signature(sort_passes);
  std::vector<unsigned long long> h_ubase(257, 0);  // (alive until the sort has run: the copy is asynchronous)
  if (split) {  // the units of the pass: every range rounded up to whole units, the room behind a range's records is not visited
    for (int d = 0; d < 256; ++d) h_ubase[d + 1] = h_ubase[d] + div_ceil((uint64_t)h_fill[d], kSortSplitUnit);
    unsigned long long *ubase = split_cur + 256;
    MHX_HIP(hipMemcpyAsync(ubase, h_ubase.data(), 257 * 8, hipMemcpyHostToDevice, st));
    prep.split_fill = split_cur;
    prep.split_ubase = ubase;
    prep.split_units = h_ubase[256];
    prep.split_range_cap = range_cap;
    prep.hist_first = 1;
  }
  uint32_t *sorted = radix_sort(c, reinterpret_cast<uint32_t *>(buf_a), reinterpret_cast<uint32_t *>(buf_b), n, 4, 1, sort_passes, &prep);
  uint64_t *bounds = c->ws("s1_bucket_bounds", ((size_t)n_bins + 1) * 8 + 64).as<uint64_t>();
  MHX_LAUNCH(c, "s1_skm_bounds", (double)n_bins * 8 * 30,
             hipLaunchKernelGGL(k_skm_bounds, dim3((n_bins + 1 + 255) / 256), dim3(256), 0, st, reinterpret_cast<const uint4 *>(sorted), n, n_bins, bounds, max_bin));
  // a bin of many times the mean is low-complexity sequence (one minimizer for millions of windows): the prefix plan has the giant path
  const uint64_t limit = std::max<uint64_t>((uint64_t)c->opt<Opt::s1_skm_max_bin>(), 16 * (n / (bin_hi - bin_lo) + 1));
  constexpr uint32_t kListCap = (uint32_t)kSkmGiantMaxBins + 1;  // (one more than is served: the cursor says how many there were)
  uint2 *giant_list = nullptr;
  if (giant && bin_hi > bin_lo) {  // the bins over the limit, listed behind the bounds (read back only when there is one)
    giant_list = c->ws("skm_giant_list", (size_t)(1 + kListCap) * 8).as<uint2>();
    MHX_HIP(hipMemsetAsync(giant_list, 0, 8, st));
    MHX_LAUNCH(c, "s1_skm_giants", (double)(bin_hi - bin_lo) * 8,
               hipLaunchKernelGGL(k_skm_giants, dim3((bin_hi - bin_lo + 255) / 256), dim3(256), 0, st, bounds, bin_lo, bin_hi, limit, giant_list, kListCap));
  }
  uint32_t h_max = 0;
  MHX_HIP(hipMemcpyAsync(&h_max, max_bin, 4, hipMemcpyDeviceToHost, st));
  MHX_HIP(hipStreamSynchronize(st));
  f->n_src = 1;
  f->src[0] = reinterpret_cast<const uint4 *>(sorted);
  f->src_bounds[0] = bounds;
  f->spare = sorted == reinterpret_cast<uint32_t *>(buf_a) ? reinterpret_cast<uint32_t *>(buf_b) : reinterpret_cast<uint32_t *>(buf_a);
  f->spare_bytes = cap_alloc * 16;  // (the whole buffer: the workgroups' output regions are cut from it, and a small job's are thin)
  f->n_records = n;
  f->n_windows = n_win;
  if (pass == 0) f->n_items = var ? h[3] : s.n_seqs * (uint64_t)(L - k + (for_count ? 0 : 4));
  f->n_bins = n_bins;
  f->bin_lo = bin_lo;
  f->bin_hi = bin_hi;
  f->bin_bits = bin_bits;
  f->max_bin = h_max;
  if (h_max <= limit) return true;
  if (!giant_list) return false;
  // s1_skm_giant: the plan of the giant bins (skm_giant.h) and their work items, the largest bins first, a bin's slices in a row
  std::vector<uint2> h_list(1 + kListCap);
  MHX_HIP(hipMemcpyAsync(h_list.data(), giant_list, h_list.size() * 8, hipMemcpyDeviceToHost, st));
  MHX_HIP(hipStreamSynchronize(st));
  const uint32_t n_listed = h_list[0].x;
  std::vector<uint2> bins(h_list.begin() + 1, h_list.begin() + 1 + std::min(n_listed, kListCap));
  std::sort(bins.begin(), bins.end(), [](const uint2 &x, const uint2 &y) { return x.y != y.y ? x.y > y.y : x.x < y.x; });
  std::vector<uint64_t> recs(bins.size());
  for (size_t g = 0; g < bins.size(); ++g) recs[g] = bins[g].y;
  std::vector<uint8_t> depth(bins.size() + 1, 0);
  const double win_per_rec = n ? (double)n_win / (double)n_passes / (double)n : 1.0;
  switch (skm_giant_plan(recs.data(), (int)recs.size(), n, win_per_rec, gk, depth.data())) {
    case kSkmGiantServed: break;
    case kSkmGiantCap: f->why = "beyond s1_skm_giant_max"; return false;
    case kSkmGiantBudget: f->why = "its slices beyond s1_skm_giant_work_pct"; return false;
    default: f->why = "more than 1024 such bins"; return false;
  }
  std::vector<uint2> items;
  for (size_t g = 0; g < bins.size(); ++g)
    for (uint32_t rj0 = 0; rj0 < (1u << depth[g]); ++rj0) items.push_back(make_uint2(bins[g].x, ((uint32_t)depth[g] << 16) | rj0));
  uint2 *d_items = c->ws("skm_giant_items", items.size() * 8 + 64).as<uint2>();
  MHX_HIP(hipMemcpyAsync(d_items, items.data(), items.size() * 8, hipMemcpyHostToDevice, st));
  MHX_HIP(hipStreamSynchronize(st));  // (items leaves scope)
  f->giants = d_items;
  f->n_giant_items = (uint32_t)items.size();
  f->giant_limit = (uint32_t)std::min<uint64_t>(limit, 0xFFFFFFFFu);
  f->giant_bins = (uint32_t)bins.size();
  f->giant_largest = bins.empty() ? 0u : bins[0].y;
  return true;
}

void s1_skm_groups_launch(mhx_ctx *c, bool agg, unsigned grid, const SkmFront &f, uint32_t k, uint32_t m, uint8_t *solid_bytes, unsigned long long *hist,
                          uint2 *agg_raw, uint32_t agg_cap, uint32_t *agg_counts, uint32_t *err, unsigned long long *marks_raw, uint32_t marks_cap,
                          uint32_t *marks_counts) {
  hipStream_t st = c->stream;
  uint32_t *ticket = c->ws("s1_stream_ticket", 64).as<uint32_t>();
  MHX_HIP(hipMemsetAsync(ticket, 0, 4, st));
  const uint32_t nslot = 1u << kSkmLogSlots;
  SkmArgs a{(int)k, m, solid_bytes, hist, agg_raw, agg_cap, agg_counts, err,
            (uint32_t)std::min<long long>(std::max<long long>(c->opt<Opt::s1_stream_fill>(nslot * 7 / 8), 1), nslot), (int)std::min<long long>(c->opt<Opt::s1_stream_probes>(), 1024),
            f.bin_lo, f.bin_hi, marks_raw, marks_cap, marks_counts, f.giants, f.n_giant_items, f.giant_limit};
  const bool giant = f.n_giant_items != 0 && f.n_src == 1;  // (the front lists giant bins on one GPU only)
  SkmSrcs srcs{};
  srcs.n = f.n_src;
  for (int q = 0; q < f.n_src; ++q) {
    srcs.ptr[q] = f.src[q];
    srcs.bounds[q] = f.src_bounds[q];
  }
  const uint64_t n_bits = c->global_bases ? c->global_bases : c->seqs.n_bases;
  const bool tags = (n_bits >> 32) != 0 || c->opt<Opt::s1_skm_tags>() != 0;
  const long long deal = std::min<long long>(std::max<long long>(c->opt<Opt::s1_skm_deal>(), 0), 2);  // (a value outside 0..2: the nearest form)
#define MHX_SKM_G(AGGV, TAGV, GV)                                                                                                \
  do {                                                                                                                           \
    if (deal == 2) hipLaunchKernelGGL((k_s1_skm<AGGV, TAGV, 2, GV>), dim3(grid), dim3(kSkmThreads), 0, st, srcs, a, ticket);      \
    else if (deal == 1) hipLaunchKernelGGL((k_s1_skm<AGGV, TAGV, 1, GV>), dim3(grid), dim3(kSkmThreads), 0, st, srcs, a, ticket); \
    else hipLaunchKernelGGL((k_s1_skm<AGGV, TAGV, 0, GV>), dim3(grid), dim3(kSkmThreads), 0, st, srcs, a, ticket);                \
  } while (0)
#define MHX_SKM(AGGV, TAGV)                  \
  do {                                       \
    if (giant) MHX_SKM_G(AGGV, TAGV, true);  \
    else MHX_SKM_G(AGGV, TAGV, false);       \
  } while (0)
  // min count 3 and 4 (s1_skm_max_m): the LOOK form, whatever s1_skm_deal says — one GPU (the marks go to the byte map), bins whole
  const bool look = m >= 3;
  if (look && (marks_raw || giant)) throw Error("s1_skm_groups: min count 3 and 4 are served on one GPU, bins whole");
#define MHX_SKM_LOOK(AGGV, TAGV) hipLaunchKernelGGL((k_s1_skm<AGGV, TAGV, 2, false, true>), dim3(grid), dim3(kSkmThreads), 0, st, srcs, a, ticket)
  MHX_LAUNCH(c, "s1_skm_groups", (double)f.n_records * 16, {
    if (look && agg && tags) MHX_SKM_LOOK(true, true);
    else if (look && agg) MHX_SKM_LOOK(true, false);
    else if (look && tags) MHX_SKM_LOOK(false, true);
    else if (look) MHX_SKM_LOOK(false, false);
    else if (agg && tags) MHX_SKM(true, true);
    else if (agg) MHX_SKM(true, false);
    else if (tags) MHX_SKM(false, true);
    else MHX_SKM(false, false);
  });
#undef MHX_SKM_LOOK
#undef MHX_SKM
#undef MHX_SKM_G
}

// ---- `count` on super-k-mer records: one GPU, 19 <= k <= 21 (k + 10 bases and two flags in a record), min count <= 2 (s1_skm_max_m: up to 4), one pass ----
bool count_skm_applies(const mhx_ctx *c, uint32_t k, uint32_t m) {
  const SeqSet &s = c->seqs;
  const long long knob = c->opt<Opt::count_skm>();
  if (!knob || !c->opt<Opt::s1_skm>() || c->global_bases || c->n_parts > 1 || c->filter_on || c->accumulate || c->pos_base) return false;
  if (k < 19 || k > 21 || m < 1 || m > s1_skm_max_m(c)) return false;
  if (!s.n_seqs || s.max_len < k + 1 || (s.n_bases >> 36)) return false;
  if (!s.fixed_len && (double)s.n_bases * 100.0 < (double)c->opt<Opt::s1_var_min_fill>() * (double)s.n_seqs * s.max_len) return false;
  const uint64_t n_win = s.n_bases > s.n_seqs * (uint64_t)k ? s.n_bases - s.n_seqs * (uint64_t)k : 0;
  return knob >= 2 || c->opt<Opt::s1_skm>() >= 2 || n_win >= (uint64_t)c->opt<Opt::s1_skm_min_windows>();
}
// the group-by's launch over the sources of `f`, edges to `grid` regions of `region` entries in `edges_raw`.  ev_raw: the EVENTS form — the
// windows of flagged keys leave as events in regions of ev_cap entries (several GPUs) instead of moving first_0_out / last_0_in here.
// -> the kernel's error bits (0: done), the distinct keys in *n_distinct
static uint32_t count_skm_launch(mhx_ctx *c, uint32_t k, uint32_t m, const SkmFront &f, unsigned grid, unsigned long long *edges_raw, uint32_t region, uint32_t *counts,
                                 uint32_t *first_0_out, uint32_t *last_0_in_p1, unsigned long long *hist, unsigned long long *ev_raw, uint32_t ev_cap,
                                 uint32_t *ev_counts, uint64_t *n_distinct) {
  SeqSet &s = c->seqs;
  hipStream_t st = c->stream;
  unsigned long long *ctr = c->ws("s1_counters", 64).as<unsigned long long>();
  uint32_t *seg_err = c->ws("s1_seg_err", 64).as<uint32_t>();
  uint32_t *ticket = c->ws("s1_stream_ticket", 64).as<uint32_t>();
  MHX_HIP(hipMemsetAsync(ctr, 0, 64, st));
  MHX_HIP(hipMemsetAsync(seg_err, 0, 4, st));
  MHX_HIP(hipMemsetAsync(ticket, 0, 4, st));
  if (ev_raw) MHX_HIP(hipMemsetAsync(ev_counts, 0, (size_t)grid * 4, st));
  const uint32_t nslot = 1u << kSkmLogSlots;
  CountSkmArgs a{(int)k, m, hist, ctr, edges_raw, region, counts, seg_err,
                 (uint32_t)std::min<long long>(std::max<long long>(c->opt<Opt::s1_stream_fill>(nslot * 7 / 8), 1), nslot), (int)std::min<long long>(c->opt<Opt::s1_stream_probes>(), 1024),
                 f.bin_lo, f.bin_hi, s.start.as<uint64_t>(), s.n_seqs, s.fixed_len, first_0_out, last_0_in_p1, ev_raw, ev_cap, ev_counts,
                 f.giants, f.n_giant_items, f.giant_limit};
  const bool giant = f.n_giant_items != 0 && f.n_src == 1 && !ev_raw;  // (the front lists giant bins on one GPU only)
  SkmSrcs srcs{};
  srcs.n = f.n_src;
  for (int q = 0; q < f.n_src; ++q) {
    srcs.ptr[q] = f.src[q];
    srcs.bounds[q] = f.src_bounds[q];
  }
  const uint64_t n_bits = c->global_bases ? c->global_bases : s.n_bases;
  const bool tags = (n_bits >> 32) != 0 || c->opt<Opt::s1_skm_tags>() != 0;
  const bool g2 = c->opt<Opt::count_skm_group>() == 2;  // (four chunks per round of compare-and-swaps spill registers here: measured 13.6 against 13.1 ms)
#define MHX_CSKM(EV, GV)                                                                                                                 \
  do {                                                                                                                                   \
    if (tags && g2) hipLaunchKernelGGL((k_count_skm<true, 2, EV, GV>), dim3(grid), dim3(kSkmThreads), 0, st, srcs, a, ticket);            \
    else if (tags) hipLaunchKernelGGL((k_count_skm<true, 4, EV, GV>), dim3(grid), dim3(kSkmThreads), 0, st, srcs, a, ticket);             \
    else if (g2) hipLaunchKernelGGL((k_count_skm<false, 2, EV, GV>), dim3(grid), dim3(kSkmThreads), 0, st, srcs, a, ticket);              \
    else hipLaunchKernelGGL((k_count_skm<false, 4, EV, GV>), dim3(grid), dim3(kSkmThreads), 0, st, srcs, a, ticket);                      \
  } while (0)
  // min count 3 and 4 (s1_skm_max_m): four thermometer levels, whatever count_skm_group says — one GPU, bins whole
  const bool lv4 = m >= 3;
  if (lv4 && (ev_raw || giant)) throw Error("count_skm_groups: min count 3 and 4 are served on one GPU, bins whole");
  MHX_LAUNCH(c, "count_skm_groups", (double)f.n_records * 16, {
    if (lv4 && tags) hipLaunchKernelGGL((k_count_skm<true, 2, false, false, 4>), dim3(grid), dim3(kSkmThreads), 0, st, srcs, a, ticket);
    else if (lv4) hipLaunchKernelGGL((k_count_skm<false, 2, false, false, 4>), dim3(grid), dim3(kSkmThreads), 0, st, srcs, a, ticket);
    else if (ev_raw) MHX_CSKM(true, false);
    else if (giant) MHX_CSKM(false, true);
    else MHX_CSKM(false, false);
  });
#undef MHX_CSKM
  uint32_t e = 0;
  unsigned long long h_ctr[8] = {0};
  MHX_HIP(hipMemcpyAsync(&e, seg_err, 4, hipMemcpyDeviceToHost, st));
  MHX_HIP(hipMemcpyAsync(h_ctr, ctr, 64, hipMemcpyDeviceToHost, st));
  MHX_HIP(hipStreamSynchronize(st));
  *n_distinct = h_ctr[4];
  return e;
}

// -> false: gave up (record array, a bin of low-complexity reads, an edge region): the caller's arrays may hold partial results of this attempt
// (pass of n_passes: a job whose record arrays would take more than s1_skm_pass_gb runs in passes over ranges of bins, as stage 1 does; the
//  caller packs every pass's edge regions behind the earlier passes' edges and orders them once at the end)
bool count_skm_groups(mhx_ctx *c, uint32_t k, uint32_t m, uint32_t *first_0_out, uint32_t *last_0_in_p1, unsigned long long *hist, CountStreamOut *o, bool *touched,
                      int pass, int n_passes) {
  SkmFront f{};
  if (!s1_skm_front(c, k, &f, pass, n_passes, 0, true, m >= 3)) {
    if (f.why) o->skm_why = "a bin of " + std::to_string(f.max_bin) + " records, " + f.why;
    return false;
  }
  const uint64_t cus = c->n_cus > 0 ? (uint64_t)c->n_cus : 256;
  // (tickets: the slices of the giant bins, then the batches)
  const unsigned grid = (unsigned)std::min<uint64_t>(cus, std::max<uint64_t>(1, f.n_giant_items + div_ceil((uint64_t)(f.bin_hi - f.bin_lo), (uint64_t)kSkmBatch)));
  const uint32_t region = (uint32_t)std::min<uint64_t>(f.spare_bytes / 8 / grid, 0xFFFFFFF0u);
  uint32_t *counts = c->ws("cs_edge_counts", (size_t)grid * 4).as<uint32_t>();
  *touched = true;
  uint64_t n_distinct = 0;
  if (count_skm_launch(c, k, m, f, grid, reinterpret_cast<unsigned long long *>(f.spare), region, counts, first_0_out, last_0_in_p1, hist, nullptr, 0, nullptr, &n_distinct))
    return false;
  o->grid = grid;
  o->cap = region;
  o->counts = counts;
  o->spare = f.spare;
  o->sorted = nullptr;
  if (pass == 0) o->n_items = f.n_items;
  o->n_distinct = n_distinct;
  o->events = nullptr;
  o->n_events = 0;
  o->skm_hp = f.hp;
  o->skm_rep = f.rep;
  o->skm_records = f.n_records;
  o->skm_windows = f.n_windows;
  o->skm_max_bin = f.max_bin;
  o->skm_bin_bits = f.bin_bits;
  o->skm_giant_bins = f.giant_bins;
  o->skm_giant_slices = f.n_giant_items;
  o->skm_giant_largest = f.giant_largest;
  return true;
}

// several GPUs (comm.hip dist_count_skm): this rank's say.  The shape of count_skm_applies under a global layout, at most kSkmSrcMax ranks (one
// source per sender), no memory plan; a rank without a window (no reads, or none of k + 1 bases) takes part: it sends nothing and owns its bins
bool count_skm_dist_applies(const mhx_ctx *c, uint32_t k, uint32_t m) {
  const SeqSet &s = c->seqs;
  if (!c->opt<Opt::count_skm>() || !c->opt<Opt::s1_skm>() || !c->opt<Opt::dist_skm>() || !c->opt<Opt::count_skm_dist>()) return false;
  if (!c->global_bases || c->n_parts > kSkmSrcMax || c->filter_on || c->accumulate || (c->global_bases >> 36)) return false;
  if (k < 19 || k > 21 || m < 1 || m > 2) return false;
  if (s.n_seqs && s.max_len >= k + 1 && !s.fixed_len &&
      (double)s.n_bases * 100.0 < (double)c->opt<Opt::s1_var_min_fill>() * (double)s.n_seqs * s.max_len)
    return false;
  return s1_skm_passes(c, k) == 1;
}

// the owner's half: the group-by over the sources the ranks sent for this rank's bins (f: n_src, src, src_bounds, bin_lo / bin_hi, n_records).  The
// solid edges of the bins leave in `grid` regions (o->spare, o->cap, o->counts) and the events of the flagged keys' windows as one dense list
// (o->events); `hist` takes the histogram of this owner's keys.  -> false: an edge or event region overflowed
bool count_skm_owner(mhx_ctx *c, uint32_t k, uint32_t m, const SkmFront &f, unsigned long long *hist, CountStreamOut *o) {
  hipStream_t st = c->stream;
  const uint64_t cus = c->n_cus > 0 ? (uint64_t)c->n_cus : 256;
  const unsigned grid = (unsigned)std::min<uint64_t>(cus, std::max<uint64_t>(1, div_ceil((uint64_t)(f.bin_hi - f.bin_lo), (uint64_t)kSkmBatch)));
  // edge regions: two entries per record this owner holds, as on one GPU (there: the spare sort buffer), and at least 4096 a workgroup — the
  // owner's records may be many more than the rank made; they go to a buffer of their own when the spare one is smaller
  const uint64_t want = std::max<uint64_t>(f.n_records * 2, (uint64_t)grid * 4096);
  unsigned long long *edges_raw = reinterpret_cast<unsigned long long *>(f.spare);
  uint64_t have = f.spare ? f.spare_bytes / 8 : 0;
  if (have < want) {
    edges_raw = c->ws("cs_skm_owner_edges", want * 8 + 64).as<unsigned long long>();
    have = want;
  }
  const uint32_t region = (uint32_t)std::min<uint64_t>(have / grid, 0xFFFFFFF0u);
  // event regions: at most two per window of a solid key without an in- or out-edge (read ends, tips: a few per thousand windows);
  // count_skm_ev_cap sets the entries of a region (tests)
  const long long ev_knob = c->opt<Opt::count_skm_ev_cap>();
  const uint64_t ev_total = std::max<uint64_t>(f.n_records / (uint64_t)std::max<long long>(c->opt<Opt::count_event_share>(), 1) * 4, (uint64_t)grid * 4096);
  const uint32_t ev_cap = ev_knob > 0 ? (uint32_t)std::min<long long>(ev_knob, 0xFFFFFFF0ll) : (uint32_t)std::min<uint64_t>(ev_total / grid, 0xFFFFFFF0u);
  unsigned long long *ev_raw = c->ws("cs_events", (size_t)grid * ev_cap * 8 + 64).as<unsigned long long>();
  uint32_t *counts = c->ws("cs_edge_counts", (size_t)grid * 4).as<uint32_t>();
  uint32_t *ev_counts = c->ws("cs_event_counts", (size_t)grid * 4).as<uint32_t>();
  uint64_t n_distinct = 0;
  if (count_skm_launch(c, k, m, f, grid, edges_raw, region, counts, nullptr, nullptr, hist, ev_raw, ev_cap, ev_counts, &n_distinct)) return false;
  std::vector<uint32_t> h_ec(grid);
  MHX_HIP(hipMemcpyAsync(h_ec.data(), ev_counts, (size_t)grid * 4, hipMemcpyDeviceToHost, st));
  MHX_HIP(hipStreamSynchronize(st));
  uint64_t n_events = 0;
  for (uint32_t v : h_ec) n_events += v;  // (no region overflowed: every cursor is within ev_cap)
  o->grid = grid;
  o->cap = region;
  o->counts = counts;
  o->spare = reinterpret_cast<uint32_t *>(edges_raw);
  o->sorted = nullptr;
  o->n_items = 0;
  o->n_distinct = n_distinct;
  o->events = ev_raw;  // (regions still: count.hip packs them)
  o->n_events = n_events;
  o->ev_cap = ev_cap;
  o->ev_counts = ev_counts;
  o->skm_hp = nullptr;
  o->skm_records = f.n_records;
  o->skm_windows = 0;
  o->skm_max_bin = f.max_bin;
  o->skm_bin_bits = f.bin_bits;
  return true;
}

// count: the homopolymer keys -> histogram, edges behind `edges_at`.  -> edges appended, keys, and whether a solid one lacks an in- or out-edge
void count_skm_hp_publish(mhx_ctx *c, const unsigned long long *hp, uint32_t k, uint32_t m, unsigned long long *hist, unsigned long long *edges_at,
                          uint64_t *n_edges, uint64_t *n_keys, bool *flagged) {
  unsigned long long *res = c->ws("skm_hp_res", 64).as<unsigned long long>();
  hipLaunchKernelGGL(k_count_hp_publish, dim3(1), dim3(64), 0, c->stream, hp, (int)k, m, hist, edges_at, res);
  unsigned long long h[3] = {0, 0, 0};
  MHX_HIP(hipMemcpyAsync(h, res, 24, hipMemcpyDeviceToHost, c->stream));
  MHX_HIP(hipStreamSynchronize(c->stream));
  *n_edges = h[0];
  *n_keys = h[1];
  *flagged = h[2] != 0;
}

// the homopolymer keys counted by k_skm_make -> histogram, mark or aggregated items (after the last pass of the group-by)
void s1_skm_hp_publish(mhx_ctx *c, const SkmFront &f, uint32_t k, uint32_t m, uint8_t *solid_bytes, unsigned long long *hist, uint2 *agg_items,
                       uint64_t *agg_cursor, bool agg, const DigitSpecs *agg_specs, unsigned long long *agg_hist) {
  if (!f.hp) return;
  DigitSpecs specs;
  specs.n = 0;
  if (agg_specs && agg_hist) specs = *agg_specs;
  MHX_LAUNCH(c, "s1_skm_hp", 64.0, hipLaunchKernelGGL(k_skm_hp_publish, dim3(1), dim3(64), 0, c->stream, f.hp, (int)k, m, solid_bytes, hist, agg_items, agg_cursor,
                                                       agg ? 1 : 0, specs, agg_specs ? agg_hist : nullptr));
}

uint64_t s1_skm_beside_below(mhx_ctx *c, const SkmFront &f, uint32_t k, uint32_t m) {
  if (!f.hp || m < 3) return 0;
  unsigned long long *res = c->ws("skm_hp_res", 64).as<unsigned long long>();
  hipLaunchKernelGGL(k_skm_beside_check, dim3(1), dim3(kSkmRepN), 0, c->stream, f.hp, f.rep ? 1 : 0, (int)k, m, res);
  unsigned long long h = 0;
  MHX_HIP(hipMemcpyAsync(&h, res, 8, hipMemcpyDeviceToHost, c->stream));
  MHX_HIP(hipStreamSynchronize(c->stream));
  return h;
}

// s1_skm_rep: the keys of the windows of period <= 4 counted by k_skm_make<.., REP> (after the last pass of the group-by; agg_items has room for
// 2 kSkmRepN items).  -> the windows counted beside the records
uint64_t s1_skm_rep_publish(mhx_ctx *c, const SkmFront &f, uint32_t k, uint32_t m, uint8_t *solid_bytes, unsigned long long *hist, uint2 *agg_items,
                            uint64_t *agg_cursor, bool agg, const DigitSpecs *agg_specs, unsigned long long *agg_hist) {
  if (!f.hp || !f.rep) return 0;
  DigitSpecs specs;
  specs.n = 0;
  if (agg_specs && agg_hist) specs = *agg_specs;
  unsigned long long *res = c->ws("skm_hp_res", 64).as<unsigned long long>();
  MHX_LAUNCH(c, "s1_skm_rep", (double)kSkmRepN * 16,
             hipLaunchKernelGGL(k_skm_rep_publish, dim3(1), dim3(kSkmRepN), 0, c->stream, f.hp + kSkmRepAt, (int)k, m, solid_bytes, hist, agg_items,
                                reinterpret_cast<unsigned long long *>(agg_cursor), agg ? 1 : 0, specs, agg_specs ? agg_hist : nullptr, res));
  unsigned long long h[2] = {0, 0};
  MHX_HIP(hipMemcpyAsync(h, res, 16, hipMemcpyDeviceToHost, c->stream));
  MHX_HIP(hipStreamSynchronize(c->stream));
  return h[0];
}

// count: the same -> histogram, edges behind `edges_at` (room for kSkmRepN).  -> edges appended, keys, whether a solid one lacks an in- or
// out-edge, and the windows counted beside the records
void count_skm_rep_publish(mhx_ctx *c, const unsigned long long *hp, uint32_t k, uint32_t m, unsigned long long *hist, unsigned long long *edges_at,
                           uint64_t *n_edges, uint64_t *n_keys, bool *flagged, uint64_t *n_windows) {
  unsigned long long *res = c->ws("skm_hp_res", 64).as<unsigned long long>();
  MHX_LAUNCH(c, "count_skm_rep", (double)kSkmRepN * 72,
             hipLaunchKernelGGL(k_count_rep_publish, dim3(1), dim3(kSkmRepN), 0, c->stream, hp + kSkmRepAt, (int)k, m, hist, edges_at, res));
  unsigned long long h[4] = {0, 0, 0, 0};
  MHX_HIP(hipMemcpyAsync(h, res, 32, hipMemcpyDeviceToHost, c->stream));
  MHX_HIP(hipStreamSynchronize(c->stream));
  *n_edges = h[0];
  *n_keys = h[1];
  *flagged = h[2] != 0;
  *n_windows = h[3];
}

// several GPUs: where the bins start in an array of records ordered by bin (a source of the owner's group-by)
void s1_skm_bounds_of(mhx_ctx *c, const uint4 *recs, uint64_t n, uint32_t n_bins, uint64_t *bounds) {
  uint32_t *scratch = c->ws("skm_cursor", 64).as<uint32_t>() + 8;
  hipLaunchKernelGGL(k_skm_bounds, dim3((n_bins + 1 + 255) / 256), dim3(256), 0, c->stream, recs, n, n_bins, bounds, scratch);
}

}  // namespace mhx
