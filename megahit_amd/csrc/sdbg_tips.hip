// SURVEY.md §8f N4 — SdBG-level tip trimming on the device-resident graph of N1.
//
// sdbg_pruning::RemoveTips (reference src/assembly/sdbg_pruning.cpp:61-179) over the succinct de Bruijn graph's
// navigation (src/sdbg/sdbg.h:106-121 Forward/Backward on rank/select, :240-330 ComputeIncomings/ComputeOutgoings):
// one thread per edge, the graph = the MHX_BUF_SDBG_* buffers that mhx_sdbg_build_index left in HBM, the result = the
// updated MHX_BUF_SDBG_INVALID bit vector (+ the number of tips removed) — the first graph-cleaning pass of `assemble`
// without the graph ever leaving the GPU.  rank / select are answered from the reference-layout tables (l2 + l1 +
// in-interval popcounts; select = binary search over the intervals between two select samples, then a word scan).
#include "sdbg_nav.h"

namespace mhx {

// RemoveTips, first loop (sdbg_pruning.cpp:150-157): everything that is neither a source nor a sink is ignored
__global__ void k_tips_init(DevSdbg g, unsigned long long *__restrict__ ignored) {
  const uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= g.n) return;
  if (!sd_indeg_zero(g, id) && !sd_outdeg_zero(g, id)) bit_set(ignored, id);
}
// Trim (sdbg_pruning.cpp:61-145), the two walking loops: backward from the sinks (dir 0), forward from the sources (dir 1).
// A path is at most `len` edges, so it is walked twice instead of stored: once to decide, once to mark.
// The nodes a walk starts from are the few that `ignored` does not cover (sources and sinks: ~1 % of the edges): they are
// listed first (one popcount pass over the bitmap + a scan), and the walk kernel runs one thread per LISTED node instead of
// one per node of the graph — 12 launches over 6 x 10^7 threads each were 48 ms, nearly all of it threads that returned at once.
__global__ void k_tips_cand_count(const unsigned long long *__restrict__ ignored, uint64_t n, uint64_t n_words, uint32_t *__restrict__ cnt) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_words) return;
  unsigned long long free_bits = ~ignored[w];
  if ((w + 1) * 64 > n) free_bits &= (n & 63) ? ((1ull << (n & 63)) - 1) : ~0ull;
  cnt[w] = (uint32_t)__builtin_popcountll(free_bits);
}
__global__ void k_tips_cand_write(const unsigned long long *__restrict__ ignored, uint64_t n, uint64_t n_words, const uint64_t *__restrict__ off,
                                  uint64_t *__restrict__ cand) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_words) return;
  unsigned long long free_bits = ~ignored[w];
  if ((w + 1) * 64 > n) free_bits &= (n & 63) ? ((1ull << (n & 63)) - 1) : ~0ull;
  uint64_t o = off[w];
  for (; free_bits; free_bits &= free_bits - 1) cand[o++] = w * 64 + (uint64_t)__builtin_ctzll(free_bits);
}

__global__ void k_tips_walk(DevSdbg g, int len, int dir, unsigned long long *__restrict__ ignored, unsigned long long *__restrict__ to_remove,
                            unsigned long long *__restrict__ n_tips, const uint64_t *__restrict__ cand, uint64_t n_cand) {
  const uint64_t ci = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ci >= (cand ? n_cand : g.n)) return;
  const uint64_t id = cand ? cand[ci] : ci;
  if (sd_bit(ignored, id)) return;
  if (dir == 0 ? !sd_outdeg_zero(g, id) : !sd_indeg_zero(g, id)) return;
  uint64_t other = kNull, cur = id;
  bool is_tip = false;
  int steps = 0;  // edges appended to the path behind `id`
  for (int i = 1; i < len; ++i) {
    other = dir == 0 ? sd_unique_prev(g, cur) : sd_unique_next(g, cur);
    if (other == kNull) {
      is_tip = dir == 0 ? sd_indeg_zero(g, cur) : sd_outdeg_zero(g, cur);
      break;
    } else if ((dir == 0 ? sd_unique_next(g, other) : sd_unique_prev(g, other)) == kNull) {
      is_tip = true;
      break;
    } else {
      ++steps;
      cur = other;
    }
  }
  if (!is_tip) return;
  // the path: id, then `steps` unique predecessors / successors (the graph does not change inside a Trim call)
  uint64_t p = id;
  bit_set(to_remove, p);
  for (int s = 0; s < steps; ++s) {
    p = dir == 0 ? sd_unique_prev(g, p) : sd_unique_next(g, p);
    bit_set(to_remove, p);
  }
  atomicAdd(n_tips, 1ull);
  bit_set(ignored, id);
  bit_set(ignored, p);  // path.back()
  if (other != kNull) bit_unset(ignored, other);
}
__global__ void k_tips_apply(unsigned long long *__restrict__ invalid, unsigned long long *__restrict__ to_remove, uint64_t n_words) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_words) {
    invalid[i] |= to_remove[i];
    to_remove[i] = 0;
  }
}

DevSdbg dev_sdbg(mhx_ctx *c, const mhx_sdbg_index_info *info, const char *who) {
  auto buf = [&](int which) -> DevBuf & {
    auto it = c->results.find(which);
    if (it == c->results.end() || !it->second.p) throw Error(std::string(who) + ": run mhx_sdbg_build_index first");
    return it->second;
  };
  DevSdbg g{};
  g.w = buf(MHX_BUF_SDBG_W).as<unsigned long long>();
  g.last = buf(MHX_BUF_SDBG_LAST).as<unsigned long long>();
  g.tip = buf(MHX_BUF_SDBG_TIP).as<unsigned long long>();
  g.invalid = buf(MHX_BUF_SDBG_INVALID).as<unsigned long long>();
  g.n = info->n_items;
  g.w_l2 = buf(MHX_BUF_SDBG_RS_W_L2).as<long long>();
  g.w_l1 = buf(MHX_BUF_SDBG_RS_W_L1).as<uint16_t>();
  g.w_sel = buf(MHX_BUF_SDBG_RS_W_SEL).as<uint32_t>();
  g.last_l2 = buf(MHX_BUF_SDBG_RS_LAST_L2).as<long long>();
  g.last_l1 = buf(MHX_BUF_SDBG_RS_LAST_L1).as<uint16_t>();
  g.last_sel = buf(MHX_BUF_SDBG_RS_LAST_SEL).as<uint32_t>();
  g.num_l1_w = info->num_l1_w;
  g.num_l2_w = info->num_l2_w;
  g.num_l1_b = info->num_l1_bits;
  g.num_l2_b = info->num_l2_bits;
  for (int i = 0; i < 10; ++i) g.w_sel_off[i] = info->w_sel_offset[i];
  for (int i = 0; i < 9; ++i) g.w_count[i] = info->w_char_count[i];
  g.last_count = info->ones_in_last;
  for (int i = 0; i < 6; ++i) {
    g.f[i] = info->f[i];
    g.rank_f[i] = info->rank_f[i];
  }
  g.tip_l2 = buf(MHX_BUF_SDBG_RS_TIP_L2).as<long long>();
  g.tip_l1 = buf(MHX_BUF_SDBG_RS_TIP_L1).as<uint16_t>();
  g.labels = buf(MHX_BUF_SDBG_TIP_LABELS).as<uint32_t>();
  g.lkt = buf(MHX_BUF_SDBG_PREFIX_LKT).as<long long>();
  g.mul = buf(MHX_BUF_SDBG_MUL).as<uint16_t>();
  g.k = info->k;
  g.wpt = info->words_per_tip_label;
  return g;
}

int sdbg_remove_tips(mhx_ctx *c, const mhx_sdbg_index_info *info, int max_tip_len, uint64_t *n_removed) {
  hipStream_t st = c->stream;
  DevSdbg g = dev_sdbg(c, info, "sdbg_remove_tips");
  c->ut_ready = c->ut_owner = false;  // a unitig graph built before this trimming no longer describes the SdBG
  if (n_removed) *n_removed = 0;
  if (!g.n || max_tip_len <= 0) return 0;
  const uint64_t nw = div_ceil(g.n, 64);
  unsigned long long *ignored = c->ws("tips_ignored", nw * 8 + 8).as<unsigned long long>();
  unsigned long long *to_remove = c->ws("tips_remove", nw * 8 + 8).as<unsigned long long>();
  unsigned long long *cnt = c->ws("tips_count", 64).as<unsigned long long>();
  MHX_HIP(hipMemsetAsync(ignored, 0, nw * 8, st));
  MHX_HIP(hipMemsetAsync(to_remove, 0, nw * 8, st));
  MHX_HIP(hipMemsetAsync(cnt, 0, 8, st));
  const unsigned grid = (unsigned)div_ceil(g.n, 256);
  MHX_LAUNCH(c, "tips_init", (double)g.n * 2, hipLaunchKernelGGL(k_tips_init, dim3(grid), dim3(256), 0, st, g, ignored));
  const bool listed = c->opt<Opt::tips_candidate_list>() != 0;
  uint32_t *wcnt = listed ? c->ws("tips_word_cnt", (nw + 1) * 4).as<uint32_t>() : nullptr;
  uint64_t *woff = listed ? c->ws("tips_word_off", (nw + 2) * 8).as<uint64_t>() : nullptr;
  auto walk = [&](int len, int dir) {
    if (!listed) {
      MHX_LAUNCH(c, "tips_walk", (double)g.n, hipLaunchKernelGGL(k_tips_walk, dim3(grid), dim3(256), 0, st, g, len, dir, ignored, to_remove, cnt,
                                                                   (const uint64_t *)nullptr, (uint64_t)0));
      return;
    }
    const unsigned gw = (unsigned)div_ceil(nw, 256);
    uint64_t n_cand = 0;
    MHX_LAUNCH(c, "tips_candidates", (double)nw * 16,
               hipLaunchKernelGGL(k_tips_cand_count, dim3(gw), dim3(256), 0, st, ignored, g.n, nw, wcnt));
    exclusive_scan_u32_u64(c, wcnt, woff, nw, woff + nw + 1);
    MHX_HIP(hipMemcpyAsync(&n_cand, woff + nw + 1, 8, hipMemcpyDeviceToHost, st));
    MHX_HIP(hipStreamSynchronize(st));
    if (!n_cand) return;
    uint64_t *cand = c->ws("tips_cand", n_cand * 8 + 64).as<uint64_t>();
    hipLaunchKernelGGL(k_tips_cand_write, dim3(gw), dim3(256), 0, st, ignored, g.n, nw, woff, cand);
    MHX_LAUNCH(c, "tips_walk", (double)n_cand * 64,
               hipLaunchKernelGGL(k_tips_walk, dim3((unsigned)div_ceil(n_cand, 256)), dim3(256), 0, st, g, len, dir, ignored, to_remove, cnt, cand, n_cand));
  };
  auto trim = [&](int len) {
    walk(len, 0);
    walk(len, 1);
    hipLaunchKernelGGL(k_tips_apply, dim3((unsigned)div_ceil(nw, 256)), dim3(256), 0, st, g.invalid, to_remove, nw);
  };
  for (int len = 2; len < max_tip_len; len *= 2) trim(len);  // sdbg_pruning.cpp:159-166
  trim(max_tip_len);
  MHX_HIP(hipGetLastError());
  unsigned long long h = 0;
  MHX_HIP(hipMemcpyAsync(&h, cnt, 8, hipMemcpyDeviceToHost, st));
  MHX_HIP(hipStreamSynchronize(st));
  if (n_removed) *n_removed = h;
  return 0;
}

}  // namespace mhx
