// `local`, first half: map every read of the library to the contigs and group the reads that hang over a contig end.
//
// Replaces HashMapper (src/localasm/hash_mapper.cpp), MappingResultCollector (src/localasm/mapping_result_collector.h) and the
// drivers EstimateInsertSize / LocalRange / MapToContigs (src/localasm/local_assemble.cpp:83-223) of the reference:
//   index    every `sparsity`-th seed of `seed` bases of every contig, keyed by its canonical form, in an open-addressing table
//            of 16-byte slots (key, value): one thread per (contig, seed slot), a 64-bit compare-and-swap on the key, the value
//            OR-ed in; a key met again gets bit 63 of its value set and is never used (LoadAndBuild :80-97), so the table does
//            not depend on the order of the inserts.  The empty key is ~0: the canonical form is the smaller of a seed and its
//            reverse complement, and the reverse complement of 32 T is 0, so no canonical key of <= 32 bases equals it.
//   map      one wavefront per read (TryMap :135-268): the lanes take the read's positions 64 at a time, each builds its window
//            from the packed words (nothing is rolled), looks it up, forms the candidate record, clips it to the contig and
//            counts its matching bases (Match :103-133, 16 bases per popcount).  The reference keeps the distinct records and
//            picks the one with the strictly largest positive match count, none when two distinct records share it; that is
//            the reduction "larger count wins; equal count, equal record: that record; equal count, other record: tie",
//            which is associative and commutative, so duplicates need not be removed and the order does not matter.
//   collect  one thread per read (per pair of a paired library) emits the 0..2 (4) items of AddSingle / AddMate as
//            {contig * 2 + end, encoded value} through a cursor; the record sort orders them by all three words; the bounds
//            of every (contig, end) are lower bounds in the sorted array.
// The insert-size estimate (batches of 2^18 reads, Histgram::Trim, the integer mean, LocalRange) is host code without any
// device call: mhx_local_insert_size.
#include <algorithm>
#include <cmath>
#include <map>

#include "dev_prims.h"
#include "mhx_internal.h"

namespace mhx {

constexpr uint64_t kLmPadWords = 64;            // window loads read up to two words past a sequence's last word
constexpr unsigned long long kLmEmpty = ~0ull;  // no canonical key of <= 32 bases (see above)
constexpr unsigned long long kLmDup = 1ull << 63;
constexpr uint32_t kLmMinReadLen = 50;          // TryMap :140
constexpr int kLmMaxOffsetBits = 14;            // EncodeMappingRead: offset | is_mate:1 | mismatch:4 | strand:1 | read id:44

struct LmSlot {
  unsigned long long key, val;
};

__device__ __forceinline__ uint64_t lm_hash(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// the `seed` bases at base offset abs as a 2 * seed bit number -> its canonical form; *rc: the reverse complement is the smaller
__device__ __forceinline__ uint64_t lm_canonical(const uint32_t *__restrict__ seq, uint64_t abs, int seed, unsigned *rc) {
  uint32_t w[2];
  load_chars<2>(seq, abs, seed, w);
  const uint64_t f = ((((uint64_t)w[0]) << 32) | w[1]) >> (64 - 2 * seed);
  uint64_t r = (((uint64_t)rc_word(w[1])) << 32) | rc_word(w[0]);
  if (seed < 32) r &= (1ull << (2 * seed)) - 1;
  *rc = r < f ? 1u : 0u;
  return r < f ? r : f;
}

// `len` (1..16) bases at base offset abs, first base in the top bits, zero below
__device__ __forceinline__ uint32_t lm_word(const uint32_t *__restrict__ seq, uint64_t abs, int len) {
  const uint64_t w0 = abs >> 4;
  const uint32_t x = funnel_l(seq[w0], seq[w0 + 1], (unsigned)(abs & 15) * 2);
  return len < 16 ? x & (0xFFFFFFFFu << (32 - 2 * len)) : x;
}

__global__ __launch_bounds__(256) void k_lm_index(const uint32_t *__restrict__ ctg, const uint64_t *__restrict__ cstart,
                                                  const uint64_t *__restrict__ slot_start, uint64_t n_ctg, uint64_t n_slots, int seed,
                                                  int sparsity, LmSlot *__restrict__ table, uint64_t mask, unsigned long long *__restrict__ n_keys) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots) return;
  uint64_t lo = 0, hi = n_ctg;  // the contig whose slots hold t (contigs without a slot share their start with the next one)
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (slot_start[mid] <= t) lo = mid;
    else hi = mid;
  }
  const uint64_t j = (t - slot_start[lo]) * (uint64_t)sparsity;
  unsigned rc;
  const unsigned long long key = lm_canonical(ctg, cstart[lo] + j, seed, &rc);
  const unsigned long long val = (lo << 32) | (j << 1) | rc;
  uint64_t h = lm_hash(key) & mask;
  for (;;) {  // the table is at most half full
    const unsigned long long prev = atomicCAS(&table[h].key, kLmEmpty, key);
    if (prev == kLmEmpty) {
      atomicOr(&table[h].val, val);  // (the value starts as 0; a repeat may set bit 63 before or after)
      atomicAdd(n_keys, 1ull);
      return;
    }
    if (prev == key) {
      atomicOr(&table[h].val, kLmDup);
      return;
    }
    h = (h + 1) & mask;
  }
}

__global__ void k_lm_clear(LmSlot *__restrict__ table, uint64_t cap) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cap) *reinterpret_cast<ulonglong2 *>(&table[i]) = make_ulonglong2(kLmEmpty, 0ull);
}

// the value of a key, bit 63 set when it is absent or was seen twice
__device__ __forceinline__ unsigned long long lm_lookup(const LmSlot *__restrict__ table, uint64_t mask, unsigned long long key) {
  uint64_t h = lm_hash(key) & mask;
  for (;;) {
    const ulonglong2 s = *reinterpret_cast<const ulonglong2 *>(&table[h]);
    if (s.x == key) return s.y;
    if (s.x == kLmEmpty) return kLmDup;
    h = (h + 1) & mask;
  }
}

// the best candidate so far: match count, "two distinct records share it", the record in three words
struct LmBest {
  int m, tie;
  unsigned long long a, b, c;
};
__device__ __forceinline__ void lm_combine(LmBest &x, const LmBest &y) {
  if (y.m > x.m) x = y;
  else if (y.m == x.m && x.m > 0 && (y.tie || x.a != y.a || x.b != y.b || x.c != y.c)) x.tie = 1;
}

__global__ __launch_bounds__(256) void k_lm_map(const uint32_t *__restrict__ reads, const uint64_t *__restrict__ rstart, uint64_t n_reads,
                                                const uint32_t *__restrict__ ctg, const uint64_t *__restrict__ cstart,
                                                const LmSlot *__restrict__ table, uint64_t mask, int seed, int min_map_len,
                                                const int *__restrict__ threshold, mhx_local_record *__restrict__ out) {
  const uint64_t r = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;  // the same for all lanes of a wavefront
  if (r >= n_reads) return;
  const int lane = lane_id();
  const uint64_t st = rstart[r];
  const int len = (int)(rstart[r + 1] - st);
  LmBest best = {0, 0, 0, 0, 0};
  if (len >= seed && len >= (int)kLmMinReadLen) {
    for (int p = lane; p + seed <= len; p += kWave) {
      unsigned qs;
      const unsigned long long key = lm_canonical(reads, st + p, seed, &qs);
      const unsigned long long val = lm_lookup(table, mask, key);
      if (val & kLmDup) continue;
      const uint32_t cid = (uint32_t)(val >> 32);
      const int coff = (int)((val & 0xFFFFFFFFull) >> 1);
      const int strand = (int)((val & 1ull) ^ qs);
      const uint64_t cst = cstart[cid];
      const int clen = (int)(cstart[cid + 1] - cst);
      const int i = p + seed - 1;  // the reference's position: the window's last base
      int cfrom = strand == 0 ? coff - p : coff - (len - 1 - i);
      int cto = strand == 0 ? coff + seed - 1 + len - 1 - i : coff + i;
      cfrom = max(cfrom, 0);
      cto = min(clen - 1, cto);
      const int span = cto - cfrom + 1;
      if (span < len && span < min_map_len) continue;
      const int qfrom = strand == 0 ? p - (coff - cfrom) : i - (cto - coff);
      const int qto = strand == 0 ? p + (cto - coff) : i + (coff - cfrom);
      // Match: the count can only fall, so its early return equals a test of the final count
      int mism = 0;
      for (int q = qfrom; q <= qto; q += 16) {
        const int n = min(16, qto - q + 1);
        const uint32_t qw = lm_word(reads, st + q, n);
        uint32_t rw;
        if (strand == 0) {
          rw = lm_word(ctg, cst + cfrom + (q - qfrom), n);
        } else {
          rw = rc_word(lm_word(ctg, cst + cto - (q + n - 1 - qfrom), n)) << (2 * (16 - n));
        }
        uint32_t x = qw ^ rw;
        x |= x >> 1;
        mism += __popc(x & 0x55555555u);
      }
      const int qspan = qto - qfrom + 1;
      const int match = qspan - mism;
      if (match < threshold[qspan] || match <= 0) continue;
      LmBest cand;
      cand.m = match;
      cand.tie = 0;
      cand.a = ((unsigned long long)cid << 32) | (uint32_t)cfrom;
      cand.b = ((unsigned long long)(uint32_t)cto << 32) | (uint32_t)qfrom;
      cand.c = ((unsigned long long)(uint32_t)qto << 1) | (unsigned)strand;
      lm_combine(best, cand);
    }
  }
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    LmBest o;
    o.m = __shfl_xor(best.m, d, kWave);
    o.tie = __shfl_xor(best.tie, d, kWave);
    o.a = __shfl_xor(best.a, d, kWave);
    o.b = __shfl_xor(best.b, d, kWave);
    o.c = __shfl_xor(best.c, d, kWave);
    lm_combine(best, o);
  }
  if (lane == 0) {
    mhx_local_record rec = {};
    if (best.m > 0 && !best.tie) {
      rec.contig_id = (uint32_t)(best.a >> 32);
      rec.contig_from = (int32_t)(uint32_t)best.a;
      rec.contig_to = (int32_t)(uint32_t)(best.b >> 32);
      rec.query_from = (int32_t)(uint32_t)best.b;
      rec.query_to = (int32_t)(best.c >> 1);
      rec.mismatch = (uint32_t)(rec.query_to - rec.query_from + 1 - best.m);
      rec.strand = (uint32_t)(best.c & 1ull);
      rec.valid = 1;
    }
    out[r] = rec;
  }
}

// the valid records: one atomic per workgroup
__global__ __launch_bounds__(256) void k_lm_count_valid(const mhx_local_record *__restrict__ rec, uint64_t n, unsigned long long *__restrict__ n_valid) {
  __shared__ unsigned part[256 / kWave];
  unsigned mine = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) mine += rec[i].valid != 0;
  mine = wave_sum(mine);
  if (lane_id() == 0) part[threadIdx.x / kWave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned all = 0;
    for (int w = 0; w < 256 / kWave; ++w) all += part[w];
    if (all) atomicAdd(n_valid, (unsigned long long)all);
  }
}

// AddSingle / AddMate (mapping_result_collector.h:19-65): the item of a record, if any
__device__ __forceinline__ unsigned long long lm_encode(uint32_t offset, unsigned is_mate, uint32_t mismatch, uint32_t strand, uint64_t read_id) {
  unsigned long long v = offset;
  v = (v << 1) | is_mate;
  v = (v << 4) | (mismatch < 15 ? mismatch : 15u);
  v = (v << 1) | strand;
  return (v << 44) | read_id;
}
// which end of its contig a record is collected at: 0 the start, 1 the end, -1 none
__device__ __forceinline__ int lm_single_end(const mhx_local_record &r, int clen, int rlen, int range) {
  if (r.contig_to < range && r.query_from != 0 && r.query_to == rlen - 1) return 0;
  if (r.contig_from + range >= clen && r.query_to < rlen - 1 && r.query_from == 0) return 1;
  return -1;
}
__device__ __forceinline__ int lm_mate_end(const mhx_local_record &r1, const mhx_local_record &r2, int clen, int range) {
  if (r2.valid && r2.contig_id == r1.contig_id) return -1;
  if (r1.contig_to < range && r1.strand == 1) return 0;
  if (r1.contig_from + range >= clen && r1.strand == 0) return 1;
  return -1;
}
// (by value from the end chosen, after both tests: one body for either end)
__device__ __forceinline__ uint4 lm_item(const mhx_local_record &r, int clen, int end, unsigned is_mate, uint64_t read_id) {
  const uint32_t off = end == 0 ? (uint32_t)r.contig_to : (uint32_t)(clen - 1 - r.contig_from);
  const unsigned long long v = lm_encode(off, is_mate, r.mismatch, r.strand, read_id);
  return make_uint4(r.contig_id * 2 + (uint32_t)end, (uint32_t)(v >> 32), (uint32_t)(v & 0xFFFFFFFFull), 0u);
}

// MapToContigs (local_assemble.cpp:166-223) of one library on the records of k_lm_map.  counters: [0] aligned, [1] added
__global__ __launch_bounds__(256) void k_lm_collect(const mhx_local_record *__restrict__ rec, const uint64_t *__restrict__ rstart,
                                                    const uint64_t *__restrict__ cstart, uint64_t lib_begin, uint64_t lib_end, int paired,
                                                    int range, uint4 *__restrict__ items, unsigned long long *__restrict__ cursor,
                                                    unsigned long long *__restrict__ counters) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t i = lib_begin + (paired ? 2 * t : t);
  const bool live = i < lib_end;  // (no early return: the whole wavefront takes part in the sums below)
  // (the end of each of the four possible items in a named variable, the items formed by value where they are stored: an array indexed
  // by a running count would live in scratch memory)
  int e_s1 = -1, e_m1 = -1, e_s2 = -1, e_m2 = -1, mapped = 0, clen1 = 0, clen2 = 0;
  mhx_local_record r1 = {}, r2 = {};
  if (live) {
    r1 = rec[i];
    if (paired) {
      r2 = rec[i + 1];
      if (r1.valid) {
        ++mapped;
        clen1 = (int)(cstart[r1.contig_id + 1] - cstart[r1.contig_id]);
        e_s1 = lm_single_end(r1, clen1, (int)(rstart[i + 1] - rstart[i]), range);
        e_m1 = lm_mate_end(r1, r2, clen1, range);
      }
      if (r2.valid) {
        ++mapped;
        clen2 = (int)(cstart[r2.contig_id + 1] - cstart[r2.contig_id]);
        e_s2 = lm_single_end(r2, clen2, (int)(rstart[i + 2] - rstart[i + 1]), range);
        e_m2 = lm_mate_end(r2, r1, clen2, range);
      }
    } else if (r1.valid) {
      ++mapped;
      clen1 = (int)(cstart[r1.contig_id + 1] - cstart[r1.contig_id]);
      e_s1 = lm_single_end(r1, clen1, (int)(rstart[i + 1] - rstart[i]), range);
    }
  }
  // one atomic per wavefront and counter: the wavefront's items take one stretch of the array, dealt out by a prefix sum
  const unsigned n = (e_s1 >= 0) + (e_m1 >= 0) + (e_s2 >= 0) + (e_m2 >= 0);
  const unsigned upto = wave_inclusive_sum(n);
  const unsigned n_wave = __shfl(upto, kWave - 1, kWave), mapped_wave = wave_sum((unsigned)mapped);
  unsigned long long base = 0;
  if (lane_id() == 0) {
    if (mapped_wave) atomicAdd(&counters[0], (unsigned long long)mapped_wave);
    if (n_wave) {
      atomicAdd(&counters[1], (unsigned long long)n_wave);
      base = atomicAdd(cursor, (unsigned long long)n_wave);
    }
  }
  base = __shfl(base, 0, kWave);
  if (n) {
    unsigned long long at = base + upto - n;
    if (e_s1 >= 0) items[at++] = lm_item(r1, clen1, e_s1, 0, i);
    if (e_m1 >= 0) items[at++] = lm_item(r1, clen1, e_m1, 1, i + 1);  // (AddMate files a record under its mate's id)
    if (e_s2 >= 0) items[at++] = lm_item(r2, clen2, e_s2, 0, i + 1);
    if (e_m2 >= 0) items[at++] = lm_item(r2, clen2, e_m2, 1, i);
  }
}

// where the items of every (contig, end) start in the sorted array: off[g] = first item whose key is >= g, g = 0 .. n_groups
__global__ void k_lm_bounds(const uint4 *__restrict__ items, uint64_t n_items, uint64_t n_groups, unsigned long long *__restrict__ off) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g > n_groups) return;
  uint64_t lo = 0, hi = n_items;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if ((uint64_t)items[mid].x < g) lo = mid + 1;
    else hi = mid;
  }
  off[g] = lo;
}
__global__ void k_lm_values(const uint4 *__restrict__ items, uint64_t n_items, unsigned long long *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  out[i] = ((unsigned long long)items[i].y << 32) | items[i].z;
}

int local_index(mhx_ctx *c, const uint32_t *ctg_words, uint64_t ctg_n_words, uint64_t n_ctg, const uint64_t *ctg_start, uint32_t seed,
                uint32_t sparsity, uint64_t *index_size) {
  hipStream_t st = c->stream;
  c->lm_ready = c->lm_mapped = false;
  if (seed < 1 || seed > 32) throw Error("local_index: seed_kmer must be 1..32");
  if (sparsity < 1) throw Error("local_index: sparsity must be at least 1");
  if (n_ctg >= (1ull << 31)) throw Error("local_index: too many contigs");  // bit 63 of a value flags a repeat; contig * 2 + end is a 32-bit word
  std::vector<uint64_t> slot_start(n_ctg + 1, 0);
  for (uint64_t i = 0; i < n_ctg; ++i) {
    if (ctg_start[i + 1] < ctg_start[i] || ctg_start[i + 1] > ctg_n_words * 16) throw Error("local_index: contig_start is not ascending inside contig_words");
    const uint64_t len = ctg_start[i + 1] - ctg_start[i];
    if (len >= (1ull << 30)) throw Error("local_index: a contig of 2^30 bases or more");  // (contig offset + read length stays a 32-bit int)
    slot_start[i + 1] = slot_start[i] + (len >= seed ? (len - seed + sparsity) / sparsity : 0);
  }
  const uint64_t n_slots = slot_start[n_ctg];
  uint64_t cap = 64;
  while (cap < 2 * n_slots) cap <<= 1;
  uint32_t *cw = c->ws("lm_ctg_words", (ctg_n_words + kLmPadWords) * 4).as<uint32_t>();
  uint64_t *cs = c->ws("lm_ctg_start", (n_ctg + 2) * 8).as<uint64_t>();
  uint64_t *ss = c->ws("lm_slot_start", (n_ctg + 2) * 8).as<uint64_t>();
  LmSlot *table = c->ws("lm_table", cap * sizeof(LmSlot)).as<LmSlot>();
  unsigned long long *ctr = c->ws("lm_counters", 64).as<unsigned long long>();
  MHX_HIP(hipMemsetAsync(cw, 0, (ctg_n_words + kLmPadWords) * 4, st));
  if (ctg_n_words) MHX_HIP(hipMemcpyAsync(cw, ctg_words, ctg_n_words * 4, hipMemcpyHostToDevice, st));
  MHX_HIP(hipMemcpyAsync(cs, ctg_start, (n_ctg + 1) * 8, hipMemcpyHostToDevice, st));
  MHX_HIP(hipMemcpyAsync(ss, slot_start.data(), (n_ctg + 1) * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_lm_clear, dim3((unsigned)div_ceil(cap, 256)), dim3(256), 0, st, table, cap);
  MHX_HIP(hipGetLastError());
  MHX_HIP(hipMemsetAsync(ctr, 0, 64, st));
  if (n_slots) {
    MHX_LAUNCH(c, "local_index", (double)n_slots * 16,
               hipLaunchKernelGGL(k_lm_index, dim3((unsigned)div_ceil(n_slots, 256)), dim3(256), 0, st, cw, cs, ss, n_ctg, n_slots, (int)seed,
                                  (int)sparsity, table, cap - 1, ctr));
  }
  unsigned long long n_keys = 0;
  MHX_HIP(hipMemcpyAsync(&n_keys, ctr, 8, hipMemcpyDeviceToHost, st));
  MHX_HIP(hipStreamSynchronize(st));  // (also: slot_start may go)
  if (index_size) *index_size = n_keys;
  c->lm_ready = true;
  c->lm_n_ctg = n_ctg;
  c->lm_cap = cap;
  c->lm_seed = seed;
  return 0;
}

int local_map(mhx_ctx *c, int32_t min_mapping_len, double similarity, uint64_t *n_valid) {
  hipStream_t st = c->stream;
  if (!c->lm_ready) throw Error("local_map: run mhx_local_index first");
  c->lm_mapped = false;
  SeqSet &s = c->seqs;  // the reads, forward orientation
  const uint64_t n_reads = s.n_seqs;
  if (n_reads >= (1ull << 44)) throw Error("local_map: read ids of 2^44 and more do not fit the collector's items");
  if (s.max_len >= (1u << 30)) throw Error("local_map: a read of 2^30 bases or more");
  if ((n_reads + 3) / 4 >= (1ull << 31)) throw Error("local_map: too many reads for one launch");
  // lround(similarity * span) of every span a read can have (Match :116), rounded by the host's libm as the reference's is
  std::vector<int> thr((size_t)s.max_len + 1);
  for (size_t i = 0; i < thr.size(); ++i) thr[i] = (int)lround(similarity * (int)i);
  int *d_thr = c->ws("lm_threshold", thr.size() * 4).as<int>();
  unsigned long long *ctr = c->ws("lm_counters", 64).as<unsigned long long>();
  MHX_HIP(hipMemcpyAsync(d_thr, thr.data(), thr.size() * 4, hipMemcpyHostToDevice, st));
  MHX_HIP(hipMemsetAsync(ctr, 0, 64, st));
  DevBuf &rec = c->result(MHX_BUF_LOCAL_REC, (n_reads ? n_reads : 1) * sizeof(mhx_local_record));
  rec.used = n_reads * sizeof(mhx_local_record);
  if (n_reads) {
    MHX_LAUNCH(c, "local_map", (double)s.n_bases / 4 + (double)n_reads * 32,
               hipLaunchKernelGGL(k_lm_map, dim3((unsigned)div_ceil(n_reads, 256 / kWave)), dim3(256), 0, st, s.words.as<uint32_t>(),
                                  s.start.as<uint64_t>(), n_reads, c->work["lm_ctg_words"].as<uint32_t>(), c->work["lm_ctg_start"].as<uint64_t>(),
                                  c->work["lm_table"].as<LmSlot>(), c->lm_cap - 1, (int)c->lm_seed, (int)min_mapping_len, d_thr,
                                  rec.as<mhx_local_record>()));
    hipLaunchKernelGGL(k_lm_count_valid, dim3((unsigned)std::min<uint64_t>(div_ceil(n_reads, 256), 4096)), dim3(256), 0, st,
                       rec.as<mhx_local_record>(), n_reads, ctr);
    MHX_HIP(hipGetLastError());
  }
  unsigned long long nv = 0;
  MHX_HIP(hipMemcpyAsync(&nv, ctr, 8, hipMemcpyDeviceToHost, st));
  MHX_HIP(hipStreamSynchronize(st));  // (also: thr may go)
  if (n_valid) *n_valid = nv;
  c->lm_mapped = true;
  c->lm_n_reads = n_reads;
  return 0;
}

int local_collect(mhx_ctx *c, uint32_t n_libs, const uint64_t *lib_begin, const uint64_t *lib_end, const int32_t *lib_paired,
                  const int32_t *lib_local_range, uint64_t *n_mapped, uint64_t *n_added) {
  hipStream_t st = c->stream;
  if (!c->lm_ready) throw Error("local_collect: run mhx_local_index first");
  if (!c->lm_mapped || c->lm_n_reads != c->seqs.n_seqs) throw Error("local_collect: run mhx_local_map on the loaded reads first");
  const uint64_t n_reads = c->lm_n_reads, n_ctg = c->lm_n_ctg;
  uint64_t in_libs = 0;
  for (uint32_t l = 0; l < n_libs; ++l) {
    if (lib_begin[l] > lib_end[l] || lib_end[l] > n_reads) throw Error("local_collect: a library's reads lie outside the loaded reads");
    if (lib_paired[l] && ((lib_end[l] - lib_begin[l]) & 1)) throw Error("local_collect: a paired library with an odd number of reads");
    if (lib_local_range[l] < 0 || lib_local_range[l] > (1 << kLmMaxOffsetBits))
      throw Error("local_collect: a local range above 2^14: the contig offsets would not fit the items");
    in_libs += lib_end[l] - lib_begin[l];
  }
  if (in_libs > n_reads) throw Error("local_collect: the libraries overlap");  // (the items' room is two per read)
  const mhx_local_record *rec = c->results[MHX_BUF_LOCAL_REC].as<mhx_local_record>();
  const uint64_t *cs = c->work["lm_ctg_start"].as<uint64_t>();
  uint4 *ia = c->ws("lm_items_a", (2 * n_reads + 1) * 16 + 64).as<uint4>();
  uint4 *ib = c->ws("lm_items_b", (2 * n_reads + 1) * 16 + 64).as<uint4>();
  unsigned long long *ctr = c->ws("lm_collect_counters", (2 * (size_t)n_libs + 2) * 8).as<unsigned long long>();  // [0] cursor, [2 + 2 l ...] per library
  MHX_HIP(hipMemsetAsync(ctr, 0, (2 * (size_t)n_libs + 2) * 8, st));
  for (uint32_t l = 0; l < n_libs; ++l) {
    const uint64_t n = lib_end[l] - lib_begin[l], threads = lib_paired[l] ? n / 2 : n;
    if (!threads) continue;
    MHX_LAUNCH(c, "local_collect", (double)n * 32,
               hipLaunchKernelGGL(k_lm_collect, dim3((unsigned)div_ceil(threads, 256)), dim3(256), 0, st, rec, c->seqs.start.as<uint64_t>(), cs,
                                  lib_begin[l], lib_end[l], lib_paired[l] ? 1 : 0, (int)lib_local_range[l], ia, ctr, ctr + 2 + 2 * l));
  }
  std::vector<unsigned long long> h(2 * (size_t)n_libs + 2);
  MHX_HIP(hipMemcpyAsync(h.data(), ctr, h.size() * 8, hipMemcpyDeviceToHost, st));
  MHX_HIP(hipStreamSynchronize(st));
  const uint64_t n_items = h[0];
  for (uint32_t l = 0; l < n_libs; ++l) {
    if (n_mapped) n_mapped[l] = h[2 + 2 * l];
    if (n_added) n_added[l] = h[3 + 2 * l];
  }
  uint4 *sorted = ia;
  if (n_items > 1) {
    // LSD passes over the bits that can be set only: the read id, then strand .. offset (value bits 44 and up; an offset is below its
    // library's range), then contig * 2 + end.  (Not sort_whole_key: its prefix plan assumes keys spread over the top bits of word 0,
    // which are all zero here.)
    auto bits_of = [](uint64_t x) {
      int b = 1;
      while (x >> b) ++b;
      return b;
    };
    int max_range = 1;
    for (uint32_t l = 0; l < n_libs; ++l) max_range = std::max(max_range, (int)lib_local_range[l]);
    std::vector<SortPass> plan;
    for (const std::pair<int, int> &r : {std::pair<int, int>{0, bits_of(n_reads)}, std::pair<int, int>{44, 50 + bits_of((uint64_t)max_range)},
                                         std::pair<int, int>{64, 64 + bits_of(2 * n_ctg + 1)}}) {
      for (const SortPass &ps : make_passes(3, r.first, r.second)) plan.push_back(ps);
    }
    sorted = reinterpret_cast<uint4 *>(radix_sort(c, reinterpret_cast<uint32_t *>(ia), reinterpret_cast<uint32_t *>(ib), n_items, 4, 3, plan));
  }
  DevBuf &vals = c->result(MHX_BUF_LOCAL_ITEMS, (n_items ? n_items : 1) * 8);
  vals.used = n_items * 8;
  DevBuf &off = c->result(MHX_BUF_LOCAL_OFFSETS, (2 * n_ctg + 1) * 8);
  if (n_items) hipLaunchKernelGGL(k_lm_values, dim3((unsigned)div_ceil(n_items, 256)), dim3(256), 0, st, sorted, n_items, vals.as<unsigned long long>());
  hipLaunchKernelGGL(k_lm_bounds, dim3((unsigned)div_ceil(2 * n_ctg + 1, 256)), dim3(256), 0, st, sorted, n_items, 2 * n_ctg, off.as<unsigned long long>());
  MHX_HIP(hipGetLastError());
  MHX_HIP(hipStreamSynchronize(st));
  return 0;
}

// EstimateInsertSize (local_assemble.cpp:83-138) of one library on the records of mhx_local_map, and LocalRange (:140-153).
// Histgram<int> (utils/histgram.h): Trim(0.01) drops whole values from either side while they fit a half per cent each;
// mean() is the int sum over the size_t count, an integer quotient; sd() is over doubles in ascending order of the values.
int local_insert_size(const mhx_local_record *rec, const uint32_t *read_len, uint64_t lib_begin, uint64_t lib_end, uint32_t max_read_len,
                      int paired, double *mean, double *sd, int32_t *local_range) {
  double mu = 0, sigma = 0;
  if (paired) {
    std::map<int, size_t> hist;
    size_t size = 0;
    const size_t batch = (size_t)1 << 18;
    const uint64_t n = lib_end - lib_begin;
    uint64_t done = 0;
    while (size < batch && done < n) {
      const uint64_t from = done;
      done = std::min<uint64_t>(from + batch, n);
      for (uint64_t i = from; i + 1 < done; i += 2) {
        const mhx_local_record &a = rec[lib_begin + i], &b = rec[lib_begin + i + 1];
        if (!a.valid || !b.valid || a.contig_id != b.contig_id || a.strand == b.strand) continue;
        const int la = (int)read_len[lib_begin + i], lb = (int)read_len[lib_begin + i + 1];
        const int v = a.strand == 0 ? b.contig_to + lb - b.query_to - (a.contig_from - a.query_from)
                                    : a.contig_to + la - a.query_to - (b.contig_from - b.query_from);
        if (v >= la && v >= lb) {
          ++hist[v];
          ++size;
        }
      }
    }
    // Trim(0.01)
    const size_t trim = (size_t)(size * 0.01 / 2 + 0.5);
    std::vector<int> gone;
    size_t sum = 0;
    for (auto it = hist.begin(); it != hist.end() && sum + it->second <= trim; ++it) {
      sum += it->second;
      gone.push_back(it->first);
    }
    size -= sum;
    sum = 0;
    for (auto it = hist.rbegin(); it != hist.rend() && sum + it->second <= trim; ++it) {
      sum += it->second;
      gone.push_back(it->first);
    }
    size -= sum;
    for (int v : gone) hist.erase(v);
    if (size) {
      int isum = 0;  // `value_type sum`: an int that takes size_t products (wraps as the reference's does)
      double dsum = 0, dsq = 0;
      for (auto &kv : hist) {
        isum = (int)((size_t)isum + (size_t)kv.first * kv.second);
        dsum += 1.0 * kv.first * kv.second;
        dsq += 1.0 * kv.first * kv.first * kv.second;
      }
      mu = (double)((size_t)isum / size);
      sigma = std::sqrt(dsq / size - (dsum / size) * (dsum / size));
    } else {
      // mean() of an empty histogram is 0; its variance is 0 / 0
      sigma = std::sqrt(0.0 / (double)size - (0.0 / (double)size) * (0.0 / (double)size));
    }
  }
  int32_t range = (int32_t)max_read_len - 1;
  if (paired && mu >= (double)(int)max_read_len) range = (int32_t)std::min(2 * mu, mu + 3 * sigma);
  if (range > 650) range = 650;  // kMaxLocalRange
  if (mean) *mean = mu;
  if (sd) *sd = sigma;
  if (local_range) *local_range = range;
  return 0;
}

}  // namespace mhx
