// dgi/csrc/moe_gemm.h — the grouped expert GEMM kernel, shared by its translation units: moe.hip
// (bf16 and e4m3 experts) and moe_int4.hip (INT4 experts, built without packed fp32 instructions).
#pragma once
#include <math.h>
#include <type_traits>

#include "stream_gemm.h"

namespace {

using namespace dgi;

constexpr int kMaxExperts = 256;

__device__ __forceinline__ float silu(float g) { return g / (1.f + expf(-g)); }

// stream_gemm.h's core over the weights of format F, one K step per group: 64 deep for bf16
// (Bf16W), 128 deep for e4m3 codes (E4m3W, widened in registers as skinny_gemm_fp8.hip does),
// 128 deep for INT4 codes (Int4GroupW: the group fold of skinny_gemm_int4.hip, one group per step).
// Row block blockIdx.y multiplies the 16·MT sorted rows p0.. by expert block_expert[blockIdx.y].
// SWIGLU: W is [E, 2N, K] and the block multiplies rows n0.. of gate and N + n0.. of up.
// E4m3W: scale [E, N or 2N] fp32, one per expert and output channel; the fp32 tile sum is
// multiplied by it (gate and up each by their own row's) before the epilogue's one rounding.
// The other formats do not read scale: INT4 scales are folded per quantisation group by the core.
template <class F, int NW, int MT, int NT, int D, bool SWIGLU>
__global__ __launch_bounds__(NW * 64) void moe_gemm_kernel(
    const uint16_t* __restrict__ X, int ldx, typename F::Mat W, const float* __restrict__ scale,
    const int* __restrict__ sorted_slot, const int* __restrict__ block_expert, uint16_t* __restrict__ Y, int ldy,
    int N, int K, int kdiv, int nslots, int E) {
  constexpr int WT = SWIGLU ? 2 * NT : NT;
  constexpr bool SCALED = std::is_same<F, E4m3W>::value;
  const int e = block_expert[blockIdx.y];
  if (e < 0 || e >= E) return;  // unused row block (workgroup-uniform)
  const int n0 = blockIdx.x * 16 * NT;
  const int p0 = blockIdx.y * 16 * MT;
  const size_t wrows = SWIGLU ? 2 * (size_t)N : (size_t)N;
  stream_gemm<F, NW, MT, WT, NT, 1, D>(
      X, ldx, K,  // host: K % (F::kStep * NW) == 0
      [&](int m) {
        const int slot = sorted_slot[p0 + m];
        if (slot < 0 || slot >= nslots) return -1;  // padding rows read nothing
        // SwiGLU gathers the token's row; the plain epilogue reads act in sorted order
        return kdiv > 0 ? slot / kdiv : p0 + m;
      },
      [&](int t, int r, int g, int w) {
        return F::ptr(W, (size_t)e * wrows + ((t < NT ? 0 : N) + n0 + (t % NT) * 16 + r), K, g, w);
      },
      [&](int mt, int nt, int r, int g, auto tile) {
        f32x4 a = tile(nt);
        f32x4 u = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (SWIGLU) u = tile(NT + nt);
        const int col = n0 + nt * 16 + r;
        if constexpr (SCALED) {
          const float sa = scale[(size_t)e * wrows + col];
          const float su = SWIGLU ? scale[(size_t)e * wrows + N + col] : 0.f;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            a[i] *= sa;
            u[i] *= su;
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int p = p0 + mt * 16 + g * 4 + i;
          const int slot = sorted_slot[p];
          if (slot >= 0 && slot < nslots) {  // padding rows write nothing
            const float val = SWIGLU ? silu(a[i]) * u[i] : a[i];
            Y[(size_t)p * ldy + col] = f32_to_bf16(val);
          }
        }
      });
}

}  // namespace
