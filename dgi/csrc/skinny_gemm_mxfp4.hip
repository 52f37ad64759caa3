// dgi/csrc/skinny_gemm_mxfp4.hip — W4A16 weight-streaming GEMM for decode-sized M over OCP
// MXFP4 weights, and the mxfp4 -> bf16 dequantiser behind every shape it does not take.
//
// Y[M, N] = X[M, K] · W[N, K]^T (+ bias[N]): bf16 X / Y / bias, fp32 accumulate, M <= 32.
// W is OCP Microscaling FP4: q[N, K/2] bytes of two e2m1 codes (element 2j in the low nibble of
// byte j, 2j+1 in the high one) and scale[N, K/32] e8m0 bytes, one per 32 elements of a row;
// the weight is elem * 2^(scale - 127).
//
// The design is stream_gemm.h's, with half the weight bytes of fp8: a K step is 256 deep and the
// lane's 64 codes are decoded with its two block scales to eight B fragments (Mxfp4W).  Every
// decoded value is exact in bf16 (one mantissa bit times a power of two, a normal number for
// scale codes 2..252), so the kernel's only roundings are the fp32 accumulation order and the
// final bf16 store.  The dequantiser writes the same bf16 values, so both routes of ops.linear
// multiply the same numbers.
//
// Scale codes outside 2..252 are outside the format as this project specifies it: they may
// decode to something else, but no address depends on a code.
#include "stream_gemm.h"

using namespace dgi;

namespace {

template <int NW, int MT, int NT, int U, int D>
__global__ __launch_bounds__(NW * 64) void skinny_gemm_w4_kernel(
    const uint16_t* __restrict__ X, int ldx, const uint8_t* __restrict__ W, const uint8_t* __restrict__ S,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ Y, int ldy, int M, int K) {
  stream_gemm_dense<Mxfp4W, NW, MT, NT, U, D>(X, ldx, Mxfp4W::Mat{W, S}, Y, ldy, M, K, [&](f32x4 v, int col) {
    const float b = bias ? bf16_to_f32(bias[col]) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = v[i] + b;
    return v;
  });
}

// NW waves, NT column tiles per wave, groups of U K-steps, ring depth D (D2 for 17..32 rows).
// The X fragment of a step is twice the fp8 kernel's (8 x u32x4 per row tile), so the ring of the
// two-row-tile instantiations is at most two groups deep, and a single group with four column
// tiles on 8 waves (256 registers per lane): deeper rings spill to scratch there.
template <int NW, int NT, int U, int D, int D2 = D>
int launch(const void* x, int ldx, const void* w, const void* scale, const void* bias, void* y, int ldy, int M,
           int N, int K, hipStream_t s) {
  return launch_stream_dense<Mxfp4W::kStep, NW, U, NT, NT>(skinny_gemm_w4_kernel<NW, 1, NT, U, D>,
                                                           skinny_gemm_w4_kernel<NW, 2, NT, U, D2>, M, N, K, s, x, ldx,
                                                           w, scale, bias, y, ldy, M, K);
}

// 32 codes (16 bytes: exactly one scale block) in, 32 bf16 out per thread.  q [N, K/2] and
// scale [N, K/32] are both contiguous, so chunk i of the flat code array belongs to scale byte i.
__global__ __launch_bounds__(256) void dequant_mxfp4_kernel(const u32x4* __restrict__ Wq,
                                                            const uint8_t* __restrict__ scale,
                                                            u32x4* __restrict__ out, long long chunks) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= chunks) return;
  const float sc = e8m0_to_f32(scale[i]);
  const u32x4 v = __builtin_nontemporal_load(Wq + i);
#pragma unroll
  for (int q = 0; q < 4; ++q) out[4 * i + q] = decode8(v[q], sc);
}

}  // namespace

// cfg selects (waves per workgroup, column tiles per wave, K-steps per group, ring depth);
// 0 = the default.  Requires K % 1024 == 0 (8-wave configs: K % 2048) and N % 16 == 0 (two column
// tiles: N % 32, four: N % 64); a geometry that does not divide the shape returns -5 and launches
// nothing.
extern "C" int dgi_skinny_gemm_w4(const void* x, int ldx, const void* w, const void* scale, const void* bias,
                                  void* y, int ldy, int M, int N, int K, int cfg, hipStream_t s) {
  if (M <= 0 || N <= 0) return 0;
  if (M > 32) return -2;
  if (K % 1024 || N % 16 || ldx % 8) return -3;
  // 4 waves, one 256-deep step per group, double buffered: the one geometry that takes every
  // K % 1024 == 0 (the caller picks among the others per shape)
  if (cfg == 0) cfg = 2;
  switch (cfg) {
    case 1: return launch<4, 1, 1, 4, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);
    case 2: return launch<4, 1, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);
    case 3: return launch<8, 1, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);     // K % 2048
    case 4: return launch<8, 1, 1, 4, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);  // K % 2048
    case 5: return launch<4, 2, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);     // N % 32
    case 6: return launch<8, 2, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);     // N % 32, K % 2048
    case 7: return launch<4, 4, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);     // N % 64
    case 8: return launch<8, 4, 1, 2, 1>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);  // N % 64, K % 2048
    default: return -4;
  }
}

// out[N, K] (bf16) = elem(q[N, K/2]) * 2^(scale[N, K/32] - 127), exactly; any N, K % 32 == 0.
extern "C" int dgi_dequant_mxfp4(const void* wq, const void* scale, void* out, int N, int K, hipStream_t s) {
  if (N <= 0 || K <= 0) return 0;
  if (K % 32) return -3;
  const long long chunks = (long long)N * (K / 32);
  const long long blocks = (chunks + 255) / 256;
  if (blocks > 0x7fffffffLL) return -2;
  dequant_mxfp4_kernel<<<dim3((unsigned)blocks), 256, 0, s>>>((const u32x4*)wq, (const uint8_t*)scale, (u32x4*)out,
                                                              chunks);
  DGI_CHECK_LAUNCH();
  return 0;
}
