// List ranking by pointer jumping (Wyllie) with compaction of the still-active elements, shared by the unitig graph's
// construction over SdBG edges (sdbg_unitig.hip) and its Refresh over (vertex, strand) nodes (unitig_clean.hip).
// Every element of a chain learns its chain head and two sums over head..itself in ceil(log2 L) rounds; a round in which
// no element finishes leaves only elements on cycles, whose minimum comes from min-propagation over the same jumps.
// One host synchronisation (the count of elements left) per round.
#pragma once
#include "sdbg_nav.h"

namespace mhx {

namespace {

// one record per element while ranking: the current jump target, the sum / minimum over (anc, i], a second sum over
// (anc, i], the chain head once anc is null.  32 bytes: one gather per jump.
struct Rk {
  uint64_t anc, val, d, head;
};
enum { kSum = 0, kMin = 1 };

__device__ __forceinline__ void push_list(bool take, uint64_t v, uint64_t *__restrict__ list, unsigned long long *__restrict__ cnt) {
  const uint64_t m = __ballot(take);
  if (!m) return;
  const int lane = lane_id();
  const int leader = __builtin_ctzll(m);
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(cnt, (unsigned long long)__builtin_popcountll(m));
  base = __shfl(base, leader);
  if (take) list[base + __builtin_popcountll(m & ((1ull << lane) - 1))] = v;
}

__global__ __launch_bounds__(256) void k_ut_pred(const uint64_t *__restrict__ succ, uint64_t n, uint64_t *__restrict__ pred) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t s = succ[i];
  if (s != kNull) pred[s] = i;
}
// one jump of every listed element: reads rk only, writes nx[t]
template <int MODE>
__global__ __launch_bounds__(256) void k_ut_jump(const Rk *__restrict__ rk, const uint64_t *__restrict__ list, uint64_t n_act, Rk *__restrict__ nx) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_act) return;
  const Rk r = rk[list[t]];
  const Rk a = rk[r.anc];
  Rk o;
  o.anc = a.anc;
  if (MODE == kSum) {
    o.val = r.val + a.val;
    o.d = r.d + a.d;
    o.head = a.anc == kNull ? a.head : r.head;
  } else {
    o.val = r.val < a.val ? r.val : a.val;
    o.d = 0;
    o.head = 0;
  }
  nx[t] = o;
}
// the jumped records back into place; elements whose target is still an element go on to the next round
__global__ __launch_bounds__(256) void k_ut_commit(Rk *__restrict__ rk, const uint64_t *__restrict__ list, uint64_t n_act, const Rk *__restrict__ nx,
                                                  uint64_t *__restrict__ out, unsigned long long *__restrict__ cnt) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool take = false;
  uint64_t i = 0;
  if (t < n_act) {
    i = list[t];
    const Rk o = nx[t];
    rk[i] = o;
    take = o.anc != kNull;
  }
  push_list(take, i, out, cnt);
}
// cycle elements: start min-propagation (val = own index, anc = pred)
__global__ __launch_bounds__(256) void k_ut_cyc_min_init(const uint64_t *__restrict__ pred, const uint64_t *__restrict__ list, uint64_t n_cyc, Rk *__restrict__ rk) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_cyc) return;
  const uint64_t i = list[t];
  rk[i] = Rk{pred[i], i, 0, 0};
}

// the buffers of one ranking and its rounds
struct Ranker {
  mhx_ctx *c;
  const char *stat;  // profile group of the jump kernels
  Rk *rk, *nx;
  uint64_t *list[2];
  unsigned long long *cnt;
  int cur = 0;

  static dim3 grid(uint64_t m) { return dim3((unsigned)div_ceil(m ? m : 1, 256)); }
  uint64_t count() {
    unsigned long long h = 0;
    MHX_HIP(hipMemcpyAsync(&h, cnt, 8, hipMemcpyDeviceToHost, c->stream));
    MHX_HIP(hipStreamSynchronize(c->stream));
    return (uint64_t)h;
  }
  // pointer jumping until done (mode kSum) or until a round finishes no element (only cycles left); returns the elements
  // left in list[cur].  kMin: a fixed number of rounds.
  uint64_t jump_rounds(int mode, uint64_t n_act, int max_rounds) {
    hipStream_t st = c->stream;
    for (int r = 0; n_act && r < max_rounds; ++r) {
      MHX_HIP(hipMemsetAsync(cnt, 0, 8, st));
      if (mode == kSum)
        MHX_LAUNCH(c, stat, (double)n_act * 96, hipLaunchKernelGGL(k_ut_jump<kSum>, grid(n_act), dim3(256), 0, st, rk, list[cur], n_act, nx));
      else
        MHX_LAUNCH(c, stat, (double)n_act * 96, hipLaunchKernelGGL(k_ut_jump<kMin>, grid(n_act), dim3(256), 0, st, rk, list[cur], n_act, nx));
      MHX_LAUNCH(c, stat, (double)n_act * 88,
                 hipLaunchKernelGGL(k_ut_commit, grid(n_act), dim3(256), 0, st, rk, list[cur], n_act, nx, list[cur ^ 1], cnt));
      const uint64_t left = count();
      cur ^= 1;
      if (mode == kSum && left == n_act) return left;  // nothing finished: cycles only
      n_act = left;
    }
    return n_act;
  }
  // the elements a kSum ranking left (list[cur]) are set aside, kept as they are; the rounds after this rotate the other list
  // and `third` (room for n_cyc entries)
  const uint64_t *keep_cycles(uint64_t *third) {
    const uint64_t *cyc = list[cur];
    list[0] = list[cur ^ 1];
    list[1] = third;
    cur = 0;
    return cyc;
  }
  // the minimum index of every cycle the n_cyc listed elements lie on, into rk[i].val (2^rounds >= n_cyc >= any cycle's
  // length).  `cyc` stays as it is (keep_cycles).
  void cycle_minima(const uint64_t *cyc, uint64_t n_cyc, const uint64_t *pred) {
    hipStream_t st = c->stream;
    cur = 0;
    MHX_HIP(hipMemcpyAsync(list[0], cyc, n_cyc * 8, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_ut_cyc_min_init, grid(n_cyc), dim3(256), 0, st, pred, cyc, n_cyc, rk);
    int rounds = 0;
    while ((1ull << rounds) < n_cyc) ++rounds;
    jump_rounds(kMin, n_cyc, rounds);
    cur = 0;
  }
};

}  // namespace

}  // namespace mhx
