// dgi/csrc/skinny_gemm.hip — bf16 weight-streaming GEMM for decode-sized M.
//
// Y[M, N] = X[M, K] · W[N, K]^T (+ bias[N]), bf16 in/out, fp32 accumulate, M <= 32.
//
// The design is stream_gemm.h's.  bf16 weights need no conversion: a K step is 64 deep and the
// lane's 8 + 8 bf16 are the B fragments of two MFMAs as loaded.  The epilogue adds the bias and
// rounds to bf16.
#include "stream_gemm.h"

using namespace dgi;

namespace {

template <int NW, int MT, int NT, int U, int D>
__global__ __launch_bounds__(NW * 64) void skinny_gemm_kernel(
    const uint16_t* __restrict__ X, int ldx, const uint16_t* __restrict__ W,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ Y, int ldy, int M, int K) {
  stream_gemm_dense<Bf16W, NW, MT, NT, U, D>(X, ldx, W, Y, ldy, M, K, [&](f32x4 v, int col) {
    const float b = bias ? bf16_to_f32(bias[col]) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = v[i] + b;
    return v;
  });
}

// NW waves, NT column tiles per wave, groups of U K-steps, ring depth D; NT2 tiles for 17..32 rows
template <int NW, int NT, int U, int D = 2, int NT2 = NT>
int launch(const void* x, int ldx, const void* w, const void* bias, void* y, int ldy, int M, int N, int K,
           hipStream_t s) {
  return launch_stream_dense<Bf16W::kStep, NW, U, NT, NT2>(skinny_gemm_kernel<NW, 1, NT, U, D>,
                                                           skinny_gemm_kernel<NW, 2, NT2, U, D>, M, N, K, s, x, ldx, w,
                                                           bias, y, ldy, M, K);
}

}  // namespace

// cfg selects (waves per workgroup, column tiles per wave, K-steps per group), the ids of
// ops.SKINNY_CFGS (3 and 6 are retired sweep points and return -4); 0 = 4.  Requires K % 1024 == 0 (16 K-steps per group).
extern "C" int dgi_skinny_gemm(const void* x, int ldx, const void* w, const void* bias, void* y, int ldy, int M,
                               int N, int K, int cfg, hipStream_t s) {
  if (M <= 0 || N <= 0) return 0;
  if (M > 32) return -2;
  if (K % 1024 || N % 16 || ldx % 8) return -3;
  // 8 waves x 2 K-steps per group, one column tile per wave: the fastest or
  // within 3 % of it on every 8B / 70B projection shape at M <= 8
  if (cfg == 0) cfg = 4;
  switch (cfg) {
    case 1: return launch<16, 1, 1>(x, ldx, w, bias, y, ldy, M, N, K, s);
    case 2: return launch<8, 2, 2>(x, ldx, w, bias, y, ldy, M, N, K, s);
    case 4: return launch<8, 1, 2>(x, ldx, w, bias, y, ldy, M, N, K, s);
    // four column tiles per wave; two for 17..32 rows (four would spill)
    case 5: return launch<16, 4, 1, 2, 2>(x, ldx, w, bias, y, ldy, M, N, K, s);
    // deeper rings: more bytes in flight per wave for short kernels (o-proj) and long K (down)
    case 7: return launch<8, 1, 1, 4>(x, ldx, w, bias, y, ldy, M, N, K, s);
    case 8: return launch<8, 1, 2, 4>(x, ldx, w, bias, y, ldy, M, N, K, s);
    case 9: return launch<4, 1, 2, 4>(x, ldx, w, bias, y, ldy, M, N, K, s);
    case 10: return launch<4, 1, 1, 8>(x, ldx, w, bias, y, ldy, M, N, K, s);
    case 11: return launch<8, 1, 1, 8>(x, ldx, w, bias, y, ldy, M, N, K, s);
    default: return -4;
  }
}
