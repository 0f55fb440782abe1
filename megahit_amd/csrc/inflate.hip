// BGZF read files inflated on the GPU (mhx_bgzf_inflate, mhx_fastx_bgzf_to_records): the host walks the members (bgzf_scan.h, nothing
// inflated), the compressed bytes go to the device, k_bgzf_inflate inflates one block per wavefront (inflate_core.h: the serial symbol
// chain uniform across the wavefront, tables / match copies / stores dealt to the lanes, the window a 32 KiB ring in LDS) and
// k_bgzf_crc checks every block's text against its trailer's CRC32.  The text stays on the device: fastx.hip parses it where it lies.
#include <cstring>
#include <string>

#include "bgzf_scan.h"
#include "dev_prims.h"
#include "inflate_core.h"
#include "mhx_internal.h"

namespace mhx {

static_assert(kBgzfNotGzip == MHX_BGZF_NOT_GZIP && kBgzfFlg == MHX_BGZF_FLG && kBgzfNoBc == MHX_BGZF_NO_BC && kBgzfShortBlock == MHX_BGZF_SHORT_BLOCK &&
                  kBgzfPastEof == MHX_BGZF_PAST_EOF && kBgzfTrailing == MHX_BGZF_TRAILING && kBgzfIsize == MHX_BGZF_ISIZE,
              "bgzf_scan.h and include/mhx.h number the scan's reasons alike");
static_assert(kInfPayloadEnd == MHX_BGZF_PAYLOAD_END && kInfBtype == MHX_BGZF_BTYPE && kInfStoredLen == MHX_BGZF_STORED_LEN &&
                  kInfCodeOver == MHX_BGZF_CODE_OVER && kInfCodeIncomplete == MHX_BGZF_CODE_INCOMPLETE && kInfBadSymbol == MHX_BGZF_BAD_SYMBOL &&
                  kInfDistFar == MHX_BGZF_DIST_FAR && kInfOutOver == MHX_BGZF_OUT_OVER && kInfOutShort == MHX_BGZF_OUT_SHORT && kInfCrc == MHX_BGZF_CRC,
              "inflate_core.h and include/mhx.h number the decoder's reasons alike");
static_assert(sizeof(BgzfBlock) == 32, "the block table is 32 bytes per block");
static_assert(sizeof(InflateState) <= 40 * 1024, "four wavefronts' states fit a CU's 160 KiB of LDS");

// the 64 lanes of the wavefront
struct InflateWave {
  static constexpr uint32_t kLanes = 64;
  __device__ uint32_t lane() const { return (uint32_t)lane_id(); }
  // one wavefront's LDS operations complete in issue order: the fence only pins the order in which they are issued
  __device__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
};

// status: the smallest (block << 8 | reason) over the blocks that failed (all ones: none)
__global__ __launch_bounds__(64) void k_bgzf_inflate(const uint8_t *__restrict__ gz, const BgzfBlock *__restrict__ blocks, uint32_t n_blocks,
                                                     uint8_t *__restrict__ text, unsigned long long *status) {
  __shared__ InflateState S;
  const uint32_t b = blockIdx.x;
  if (b >= n_blocks) return;
  const BgzfBlock bl = blocks[b];
  const uint32_t why = inflate_block(InflateWave{}, S, gz + bl.in_off, bl.in_size, text + bl.out_off, bl.isize);
  if (why != kInfOk && lane_id() == 0) atomicMin(status, (unsigned long long)b << 8 | why);
}

// tabs: the 256 byte entries of the CRC, then the 64 chunk shifts (inflate_core.h).  One wavefront per block, four to a workgroup.
__global__ __launch_bounds__(256) void k_bgzf_crc(const uint8_t *__restrict__ text, const BgzfBlock *__restrict__ blocks, uint32_t n_blocks,
                                                  const uint32_t *__restrict__ tabs, unsigned long long *status) {
  __shared__ uint32_t tab[256 + 64];
  for (uint32_t i = threadIdx.x; i < 256 + 64; i += 256) tab[i] = tabs[i];
  __syncthreads();
  const uint32_t b = blockIdx.x * 4 + threadIdx.x / kWave;
  if (b >= n_blocks) return;
  const BgzfBlock bl = blocks[b];
  uint32_t x = crc_chunk_share(text + bl.out_off, bl.isize, (uint32_t)lane_id(), tab, tab + 256);
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) x ^= __shfl_xor(x, d, kWave);
  if (lane_id() == 0 && crc_finish(x, bl.isize) != bl.crc) atomicMin(status, (unsigned long long)b << 8 | kInfCrc);
}

// gz[0 .. n) -> its text in `text` (n_text + 64 bytes reserved).  out->status 0: inflated and checked; 2: see reason / bad_block.
// Workspaces tag + "gz" / "blocks" (the compressed bytes and the block table stay there until the next call with the tag).
static void bgzf_inflate_into(mhx_ctx *c, const void *gz, uint64_t n, const std::string &tag, DevBuf &text, mhx_bgzf_result *out) {
  hipStream_t st = c->stream;
  memset(out, 0, sizeof *out);
  const BgzfScan scan = bgzf_scan(gz, n);
  if (scan.reason != kBgzfOk) {
    out->status = 2;
    out->reason = scan.reason;
    out->bad_block = scan.bad_block;
    return;
  }
  const uint64_t nb = scan.blocks.size();
  if (nb >= (1ull << 31)) throw Error("bgzf_inflate: more than 2^31 blocks");
  out->n_blocks = nb;
  out->n_text = scan.n_text;
  text.reserve(scan.n_text + 64);
  text.used = scan.n_text;
  if (!nb) return;
  uint8_t *d_gz = c->ws((tag + "gz").c_str(), n + 8).as<uint8_t>();
  upload_pinned(c, d_gz, gz, n);
  BgzfBlock *d_blocks = c->ws((tag + "blocks").c_str(), nb * sizeof(BgzfBlock)).as<BgzfBlock>();
  upload_pinned(c, d_blocks, scan.blocks.data(), nb * sizeof(BgzfBlock));
  uint32_t h_tabs[256 + 64];
  for (uint32_t i = 0; i < 256; ++i) h_tabs[i] = crc_table_entry(i);
  crc_shift_table(h_tabs + 256);
  uint32_t *d_tabs = c->ws("bgzf_crc_tabs", sizeof h_tabs).as<uint32_t>();
  MHX_HIP(hipMemcpyAsync(d_tabs, h_tabs, sizeof h_tabs, hipMemcpyHostToDevice, st));
  unsigned long long *d_status = c->ws("bgzf_status", 64).as<unsigned long long>();
  MHX_HIP(hipMemsetAsync(d_status, 0xFF, 64, st));
  MHX_HIP(hipMemsetAsync(text.as<uint8_t>() + scan.n_text, 0, 64, st));
  unsigned long long h_status = ~0ull;
  auto failed = [&]() {
    MHX_HIP(hipMemcpyAsync(&h_status, d_status, 8, hipMemcpyDeviceToHost, st));
    MHX_HIP(hipStreamSynchronize(st));
    if (h_status == ~0ull) return false;
    out->status = 2;
    out->reason = (uint32_t)(h_status & 0xFF);
    out->bad_block = h_status >> 8;
    return true;
  };
  MHX_LAUNCH(c, "bgzf_inflate", (double)(n + scan.n_text),
             hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)nb), dim3(64), 0, st, d_gz, d_blocks, (uint32_t)nb, text.as<uint8_t>(), d_status));
  if (failed()) return;
  MHX_LAUNCH(c, "bgzf_crc", (double)scan.n_text,
             hipLaunchKernelGGL(k_bgzf_crc, dim3((unsigned)div_ceil(nb, (uint64_t)4)), dim3(256), 0, st, text.as<uint8_t>(), d_blocks, (uint32_t)nb, d_tabs,
                                d_status));
  failed();
}

void bgzf_inflate(mhx_ctx *c, const void *gz, uint64_t n, mhx_bgzf_result *out) {
  DevBuf &text = c->results[MHX_BUF_FASTX_TEXT];
  bgzf_inflate_into(c, gz, n, "bgzf_", text, out);
  if (out->status) text.used = 0;
}

void fastx_bgzf_to_records(mhx_ctx *c, const void *gz1, uint64_t n1, const void *gz2, uint64_t n2, mhx_fastx_result *out) {
  hipStream_t st = c->stream;
  memset(out, 0, sizeof *out);
  const bool paired = gz2 != nullptr;
  // the texts are inflated into the workspaces the parser keeps an uploaded text in
  const void *gz[2] = {gz1, gz2};
  const uint64_t n[2] = {n1, n2};
  const char *d_text[2] = {nullptr, nullptr};
  uint64_t n_text[2] = {0, 0};
  char edge[2][3] = {{0, 0, 0}, {0, 0, 0}};  // a text's first, last and last but one byte
  for (int f = 0; f < (paired ? 2 : 1); ++f) {
    // (both files are scanned before either is inflated: a mate that is not BGZF costs no upload)
    const BgzfScan scan = bgzf_scan(gz[f], n[f]);
    if (scan.reason != kBgzfOk) {
      out->status = 2;
      return;
    }
  }
  for (int f = 0; f < (paired ? 2 : 1); ++f) {
    DevBuf &text = c->ws(f ? "fx2_text" : "fx1_text", 64);
    mhx_bgzf_result r;
    bgzf_inflate_into(c, gz[f], n[f], f ? "bgzf2_" : "bgzf1_", text, &r);
    if (r.status) {
      out->status = 2;
      return;
    }
    d_text[f] = text.as<char>();
    n_text[f] = r.n_text;
    if (r.n_text) {
      MHX_HIP(hipMemcpyAsync(&edge[f][0], d_text[f], 1, hipMemcpyDeviceToHost, st));
      MHX_HIP(hipMemcpyAsync(&edge[f][1], d_text[f] + r.n_text - 1, 1, hipMemcpyDeviceToHost, st));
      if (r.n_text > 1) MHX_HIP(hipMemcpyAsync(&edge[f][2], d_text[f] + r.n_text - 2, 1, hipMemcpyDeviceToHost, st));
      MHX_HIP(hipStreamSynchronize(st));
    }
  }
  fastx_device_to_records(c, d_text[0], n_text[0], edge[0], paired ? d_text[1] : nullptr, n_text[1], edge[1], paired, out);
}

}  // namespace mhx
