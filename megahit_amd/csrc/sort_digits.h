// Digit description shared by the radix sort (sort.hip) and the extraction kernels that pre-compute its histograms.
#pragma once
#include <cstdint>

namespace mhx {

// where a pass's digit lives: up to two bit fields (word index, bit offset, mask); field 2 is the upper part
struct DigitSpec {
  int wi1;
  unsigned bit1, mask1;
  int wi2;
  unsigned bit2, mask2, sh2;  // mask2 == 0: single field
  unsigned prev_mask = 0;     // bits of word wi1 that the earlier passes of the plan have sorted (k_radix_onesweep_u RANK 2)
};
constexpr int kMaxFusedPasses = 16;  // digit histograms taken in one read of the input
struct DigitSpecs {
  DigitSpec d[kMaxFusedPasses];
  int n;
};

// digit of a record held in registers: bits [bit, bit+nbits) of word wi (and wi-1 when straddling)
template <int S>
__device__ __forceinline__ unsigned words_digit(const uint32_t (&w)[S], int wi, unsigned bit, unsigned mask) {
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    if (i == wi) lo = w[i];
    if (i == wi - 1) hi = w[i];
  }
  const uint64_t v = ((uint64_t)hi << 32) | lo;
  return (unsigned)(v >> bit) & mask;
}
template <int S>
__device__ __forceinline__ unsigned words_digit2(const uint32_t (&w)[S], const DigitSpec &ds) {
  unsigned d = words_digit<S>(w, ds.wi1, ds.bit1, ds.mask1);
  if (ds.mask2) d |= words_digit<S>(w, ds.wi2, ds.bit2, ds.mask2) << ds.sh2;
  return d;
}


// Producers of 8-byte items (k_agg_compact, k_s2d_emit) take the digit histograms of the sort that follows from the items they hold in
// registers: an LDS table [kItemHistRows][256] per workgroup, flushed once at its end, as k_radix_hist_all does (sort.hip).
// The digits are kept as shifts and masks of the 64-bit item, one packed word per pass, made once per kernel and held in ONE vector
// register (lane p: pass p; v_readlane hands a pass's word out): indexing the DigitSpecs argument by a loop counter costs a scalar load
// and a wait per pass and item, and the words of all passes in scalar registers cost k_s2d_emit a wavefront per SIMD.
constexpr int kItemHistRows = 8;
struct ItemDigits {
  uint32_t fv;  // lane p: shift 1 | shift 2 << 6 | shift of field 2 within the digit << 12 | mask 1 << 16 | mask 2 << 24 of pass p
  int n;
  __device__ __forceinline__ explicit ItemDigits(const DigitSpecs &specs) : fv(0), n(specs.n) {
    const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
    for (int p = 0; p < kItemHistRows; ++p) {  // word 1 is the low half of the item, word 0 its high half (words_digit<2>)
      const DigitSpec &d = specs.d[p];
      const uint32_t f = ((uint32_t)(1 - d.wi1) * 32u + d.bit1) | (((uint32_t)(1 - d.wi2) * 32u + d.bit2) & 63u) << 6 | (d.sh2 & 15u) << 12 |
                         (d.mask1 & 255u) << 16 | (d.mask2 & 255u) << 24;
      if (lane == p) fv = f;
    }
  }
};
__device__ __forceinline__ void item_hist_add(uint32_t (*h)[256], const ItemDigits &d, uint64_t v) {
#pragma nounroll
  for (int p = 0; p < d.n; ++p) {
    const uint32_t f = __builtin_amdgcn_readlane(d.fv, p);
    uint32_t dig = (uint32_t)(v >> (f & 63u)) & ((f >> 16) & 255u);
    if (f >> 24) dig |= ((uint32_t)(v >> ((f >> 6) & 63u)) & (f >> 24)) << ((f >> 12) & 15u);
    atomicAdd(&h[p][dig], 1u);
  }
}
__device__ __forceinline__ void item_hist_flush(uint32_t (*h)[256], const ItemDigits &specs, unsigned long long *__restrict__ ghist) {  // 256 threads
  for (int p = 0; p < specs.n; ++p) {
    const uint32_t v = h[p][threadIdx.x];
    if (v) atomicAdd(&ghist[p * 256 + threadIdx.x], (unsigned long long)v);
  }
}

}  // namespace mhx
