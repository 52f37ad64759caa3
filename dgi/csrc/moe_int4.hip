// dgi/csrc/moe_int4.hip — moe_gemm_w4: the grouped expert GEMM of moe_gemm.h over INT4 weight-only
// experts (opt-in, expert_quant="awq").
//
// Storage is Int4Weight's row layout (stream_gemm.h, dgi/ops/int4.py) stacked over experts:
// q [E, N or 2N, K/8] dwords of 8 codes, sz [E, N or 2N, K/128] dwords of one group's fp16 scale and
// zero point.  Rows are independent, so [gate; up] and the expert index are row offsets.  The codes
// reach the MFMA as exact bf16 integers; scale and zero point are folded once per 128-element group
// in fp32 by the core, so no weight is rounded and the epilogue has no scale to apply.
//
// Geometry, a function of K alone (a row's bits do not depend on the row block, on D or on T):
// Int4GroupW's 128-deep steps of one quantisation group each, split between 4 waves when
// K % 512 == 0 and between 2 otherwise (K % 256 == 0 is an even number of steps), as moe_gemm_w8
// chooses.  Int4W's 256-deep step on K % 1024 == 0 measured slower from 4 tokens up and needs up to
// 256 VGPRs (profiles/moe_int4/README.md), so every K takes the 128-deep one.
// A file of its own because the fold's fmas must stay scalar: it is built without packed fp32
// instructions (dgi/build.py), which moe.hip's kernels use.
#include "moe_gemm.h"

namespace {

template <int NW, int MT, bool SWIGLU>
int launch_gemm_w4(const void* x, int ldx, Int4W::Mat w, const int* sorted_slot, const int* block_expert, void* y,
                   int ldy, int P, int N, int K, int kdiv, int nslots, int E, hipStream_t s) {
  constexpr int NT = 1;
  // the w8 launcher's double buffer at both row blocks (registers: profiles/moe_int4/README.md)
  constexpr int D = 2;
  const dim3 grid(N / (16 * NT), P / (16 * MT));
  moe_gemm_kernel<Int4GroupW, NW, MT, NT, D, SWIGLU><<<grid, NW * 64, 0, s>>>(
      (const uint16_t*)x, ldx, w, nullptr, sorted_slot, block_expert, (uint16_t*)y, ldy, N, K, kdiv, nslots, E);
  DGI_CHECK_LAUNCH();
  return 0;
}

template <int NW>
int dispatch_gemm_w4(const void* x, int ldx, Int4W::Mat w, const int* sorted_slot, const int* block_expert,
                     void* y, int ldy, int P, int N, int K, int kdiv, int nslots, int E, int BM, int epi,
                     hipStream_t s) {
#define DGI_MOE_W4(MT, SW) \
  launch_gemm_w4<NW, MT, SW>(x, ldx, w, sorted_slot, block_expert, y, ldy, P, N, K, kdiv, nslots, E, s)
  if (BM == 16) return epi ? DGI_MOE_W4(1, true) : DGI_MOE_W4(1, false);
  return epi ? DGI_MOE_W4(2, true) : DGI_MOE_W4(2, false);
#undef DGI_MOE_W4
}

}  // namespace

// dgi_moe_gemm over INT4 experts: q [E, N or 2N, K/8] int32, sz [E, N or 2N, K/128] int32; the result
// is bf16(sum over groups of scale * sum x (code - zero)) (SwiGLU: silu(gate) * up of the two sums).
extern "C" int dgi_moe_gemm_w4(const void* x, int ldx, const void* q, const void* sz, const int* sorted_slot,
                               const int* block_expert, void* y, int ldy, int P, int N, int K, int kdiv, int nslots,
                               int E, int BM, int epi, hipStream_t s) {
  if (P <= 0 || N <= 0) return 0;
  if (K % 256 || N % 16 || ldx % 8 || K <= 0) return -3;
  if ((BM != 16 && BM != 32) || P % BM || E < 1 || E > kMaxExperts || kdiv < 0 || (epi != 0 && epi != 1)) return -3;
  if (P / 16 > 65535) return -2;
  const Int4W::Mat w{(const uint32_t*)q, (const uint32_t*)sz};
#define DGI_MOE_W4_ARGS x, ldx, w, sorted_slot, block_expert, y, ldy, P, N, K, kdiv, nslots, E, BM, epi, s
  if (K % 512 == 0) return dispatch_gemm_w4<4>(DGI_MOE_W4_ARGS);
  return dispatch_gemm_w4<2>(DGI_MOE_W4_ARGS);
#undef DGI_MOE_W4_ARGS
}
