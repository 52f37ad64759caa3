// dgi/csrc/skinny_gemm_fp8.hip — W8A16 weight-streaming GEMM for decode-sized M, and the
// fp8 -> bf16 dequantiser behind every shape it does not take.
//
// Y[M, N] = (X[M, K] · Wq[N, K]^T) * scale[N] (+ bias[N]): bf16 X / Y / bias, OCP e4m3
// (``float8_e4m3fn``, not fnuz) weights with one fp32 scale per output channel, fp32
// accumulate, M <= 32.
//
// The design is stream_gemm.h's, with half the weight bytes of bf16: a K step is 128 deep and
// the lane's 32 e4m3 values are widened in registers to four B fragments (E4m3W).  The epilogue
// multiplies the fp32 sum by scale[col], adds the bias and rounds once.
#include "stream_gemm.h"

using namespace dgi;

namespace {

template <int NW, int MT, int NT, int U, int D>
__global__ __launch_bounds__(NW * 64) void skinny_gemm_w8_kernel(
    const uint16_t* __restrict__ X, int ldx, const uint8_t* __restrict__ W, const float* __restrict__ scale,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ Y, int ldy, int M, int K) {
  stream_gemm_dense<E4m3W, NW, MT, NT, U, D>(X, ldx, W, Y, ldy, M, K, [&](f32x4 v, int col) {
    const float sc = scale[col];
    const float b = bias ? bf16_to_f32(bias[col]) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = v[i] * sc + b;
    return v;
  });
}

// NW waves, NT column tiles per wave, groups of U K-steps, ring depth D
template <int NW, int NT, int U, int D>
int launch(const void* x, int ldx, const void* w, const void* scale, const void* bias, void* y, int ldy, int M,
           int N, int K, hipStream_t s) {
  return launch_stream_dense<E4m3W::kStep, NW, U, NT, NT>(skinny_gemm_w8_kernel<NW, 1, NT, U, D>,
                                                          skinny_gemm_w8_kernel<NW, 2, NT, U, D>, M, N, K, s, x, ldx, w,
                                                          scale, bias, y, ldy, M, K);
}

// 16 e4m3 in, 16 bf16 out per thread; K % 16 == 0 keeps a chunk inside one row (one scale)
__global__ __launch_bounds__(256) void dequant_fp8_kernel(const u32x4* __restrict__ Wq,
                                                          const float* __restrict__ scale,
                                                          u32x4* __restrict__ out, long long chunks, int K16) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= chunks) return;
  const float sc = scale[i / K16];
  const u32x4 v = __builtin_nontemporal_load(Wq + i);
  u32x4 o[2];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x2v lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[q], false);
    const f32x2v hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[q], true);
    o[q >> 1][2 * (q & 1)] = pack_bf16x2(lo[0] * sc, lo[1] * sc);
    o[q >> 1][2 * (q & 1) + 1] = pack_bf16x2(hi[0] * sc, hi[1] * sc);
  }
  out[2 * i] = o[0];
  out[2 * i + 1] = o[1];
}

}  // namespace

// cfg selects (waves per workgroup, column tiles per wave, K-steps per group, ring depth);
// 0 = the default.  Requires K % 1024 == 0 (cfg 7: K % 2048) and N % 16 == 0 (cfg 5: N % 32, cfg 8: N % 64);
// a geometry that does not divide the shape returns -5 and launches nothing.
extern "C" int dgi_skinny_gemm_w8(const void* x, int ldx, const void* w, const void* scale, const void* bias,
                                  void* y, int ldy, int M, int N, int K, int cfg, hipStream_t s) {
  if (M <= 0 || N <= 0) return 0;
  if (M > 32) return -2;
  if (K % 1024 || N % 16 || ldx % 8) return -3;
  // 8 waves, one 128-deep step per group, double buffered: the fastest or within 4 % of it on six of
  // the eight 8B / 70B projections at M = 1 (the caller picks wider column tiles for more rows)
  if (cfg == 0) cfg = 2;
  switch (cfg) {
    case 1: return launch<8, 1, 1, 4>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);
    case 2: return launch<8, 1, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);
    case 3: return launch<4, 1, 2, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);
    case 4: return launch<4, 1, 2, 4>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);
    case 5: return launch<8, 2, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);   // N % 32
    case 6: return launch<4, 1, 1, 8>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);
    case 7: return launch<16, 1, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);  // K % 2048
    case 8: return launch<8, 4, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);   // N % 64
    default: return -4;
  }
}

// out[N, K] (bf16) = round(float(Wq[N, K]) * scale[n]); any N, K % 16 == 0.
extern "C" int dgi_dequant_fp8(const void* wq, const void* scale, void* out, int N, int K, hipStream_t s) {
  if (N <= 0 || K <= 0) return 0;
  if (K % 16) return -3;
  const long long chunks = (long long)N * (K / 16);
  const long long blocks = (chunks + 255) / 256;
  if (blocks > 0x7fffffffLL) return -2;
  dequant_fp8_kernel<<<dim3((unsigned)blocks), 256, 0, s>>>((const u32x4*)wq, (const float*)scale, (u32x4*)out,
                                                            chunks, K / 16);
  DGI_CHECK_LAUNCH();
  return 0;
}
