// dgi/csrc/skinny_gemm_int4.hip — W4A16 weight-streaming GEMM for decode-sized M over INT4
// weights with a per-group fp16 scale and zero point (the AWQ family), and the int4 -> bf16
// dequantiser behind every shape it does not take.
//
// Y[M, N] = X[M, K] · W[N, K]^T (+ bias[N]): bf16 X / Y / bias, fp32 accumulate, M <= 32.
//   w[n, k] = (code[n, k] - zero[n, k / 128]) * scale[n, k / 128]
// with code and zero in 0..15 and scale a finite fp16.  The storage is the kernel's own, written
// by the loader (dgi/ops/int4.py repacks AWQ tensors into it), not AWQ's:
//   q  [N, K/8] dwords.  Group h of a row (128 elements) is dwords 16h .. 16h + 15; dword
//      16h + 4g + c holds k = 128h + 32c + 8g + j for j = 0..7, element j in nibble
//      (j >> 1) + 4 (j & 1): nibbles 0..3 are j = 0, 2, 4, 6 and nibbles 4..7 are j = 1, 3, 5, 7.
//   sz [N, K/128] dwords.  Low half: the fp16 bits of the scale; high half: 0x4300 + zero, which
//      is 128 + zero as a bf16.
//
// The design is stream_gemm.h's, on its grouped path (Int4W there).  A K step is 256 deep: lane
// group g reads 16 bytes of each of the step's two quantisation groups, so that each of its eight
// dwords is one MFMA B fragment in the natural K order, inside one group.  Nothing is multiplied
// per element: a dword becomes four bf16 pairs 128 + code by a shift and an and-or each (exact),
// the four MFMAs of a group run into a group accumulator, the group's row sums of X come from
// four more MFMAs against a B operand of ones (shared by all column tiles of the wave), and the
// group is folded once in fp32: acc += scale * (acc_g - (128 + zero) * xsum_g).  The weights
// stay exact; the roundings are the fp32 sums (the 128 offset costs about 7 of their 24 bits
// inside one group sum of 128 products), the fold and the final bf16 store.
//
// The dequantiser writes bf16_rn(float(code - zero) * float(scale)): the product of a 5-bit
// integer and an fp16 is exact in fp32, so that value is well defined — but it is a rounded
// weight, which the kernel above never forms.
#include "stream_gemm.h"

using namespace dgi;

namespace {

template <int NW, int MT, int NT, int U, int D>
__global__ __launch_bounds__(NW * 64) void skinny_gemm_i4_kernel(
    const uint16_t* __restrict__ X, int ldx, const uint32_t* __restrict__ W, const uint32_t* __restrict__ SZ,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ Y, int ldy, int M, int K) {
  stream_gemm_dense<Int4W, NW, MT, NT, U, D>(X, ldx, Int4W::Mat{W, SZ}, Y, ldy, M, K, [&](f32x4 v, int col) {
    const float b = bias ? bf16_to_f32(bias[col]) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = v[i] + b;
    return v;
  });
}

// NW waves, NT column tiles per wave, groups of U K-steps, ring depth D (D2 for 17..32 rows).
// The X fragment of a step is the mxfp4 kernel's (8 x u32x4 per row tile), and the group
// accumulators and row sums come on top: the two-row-tile instantiations on 8 waves (256 registers
// per lane) run a single group, and at most two column tiles (NT2), or they spill to scratch.
template <int NW, int NT, int U, int D, int D2 = D, int NT2 = NT>
int launch(const void* x, int ldx, const void* w, const void* sz, const void* bias, void* y, int ldy, int M, int N,
           int K, hipStream_t s) {
  return launch_stream_dense<Int4W::kStep, NW, U, NT, NT2>(skinny_gemm_i4_kernel<NW, 1, NT, U, D>,
                                                           skinny_gemm_i4_kernel<NW, 2, NT2, U, D2>, M, N, K, s, x, ldx,
                                                           w, sz, bias, y, ldy, M, K);
}

// One dword of codes in, 8 bf16 (16 bytes) out per thread.  Dword d of a row: group d / 16, lane
// group (d % 16) / 4, fragment d % 4.
__global__ __launch_bounds__(256) void dequant_int4_kernel(const uint32_t* __restrict__ Wq,
                                                           const uint32_t* __restrict__ SZ,
                                                           uint16_t* __restrict__ out, long long dwords, int K) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= dwords) return;
  const int per_row = K >> 3;
  const long long row = i / per_row;
  const int d = (int)(i - row * per_row);
  const int h = d >> 4, g = (d >> 2) & 3, c = d & 3;
  const uint32_t w = SZ[row * (K >> 7) + h];
  const float sc = (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu));
  const int zero = (int)(w >> 16) - 0x4300;
  const uint32_t codes = __builtin_nontemporal_load(Wq + i);
  u32x4 r;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float lo = (float)((int)((codes >> (4 * p)) & 15u) - zero) * sc;
    const float hi = (float)((int)((codes >> (4 * p + 16)) & 15u) - zero) * sc;
    r[p] = (uint32_t)f32_to_bf16(lo) | ((uint32_t)f32_to_bf16(hi) << 16);
  }
  *reinterpret_cast<u32x4*>(out + row * K + 128 * h + 32 * c + 8 * g) = r;
}

}  // namespace

// cfg selects (waves per workgroup, column tiles per wave, K-steps per group, ring depth);
// 0 = the default.  Requires K % 1024 == 0 (8-wave configs: K % 2048) and N % 16 == 0 (two column
// tiles: N % 32, four: N % 64); a geometry that does not divide the shape returns -5 and launches
// nothing.
extern "C" int dgi_skinny_gemm_i4(const void* x, int ldx, const void* w, const void* sz, const void* bias, void* y,
                                  int ldy, int M, int N, int K, int cfg, hipStream_t s) {
  if (M <= 0 || N <= 0) return 0;
  if (M > 32) return -2;
  if (K % 1024 || N % 16 || ldx % 8) return -3;
  // 4 waves, one 256-deep step per group, double buffered: the one geometry that takes every
  // K % 1024 == 0 (the caller picks among the others per shape)
  if (cfg == 0) cfg = 2;
  switch (cfg) {
    case 1: return launch<4, 1, 1, 4, 2>(x, ldx, w, sz, bias, y, ldy, M, N, K, s);
    case 2: return launch<4, 1, 1, 2>(x, ldx, w, sz, bias, y, ldy, M, N, K, s);
    case 3: return launch<8, 1, 1, 2>(x, ldx, w, sz, bias, y, ldy, M, N, K, s);     // K % 2048
    case 4: return launch<8, 1, 1, 4, 2>(x, ldx, w, sz, bias, y, ldy, M, N, K, s);  // K % 2048
    case 5: return launch<4, 2, 1, 2>(x, ldx, w, sz, bias, y, ldy, M, N, K, s);     // N % 32
    case 6: return launch<8, 2, 1, 2, 1>(x, ldx, w, sz, bias, y, ldy, M, N, K, s);  // N % 32, K % 2048
    case 7: return launch<4, 4, 1, 2>(x, ldx, w, sz, bias, y, ldy, M, N, K, s);     // N % 64
    case 8:  // N % 64, K % 2048; two column tiles at M > 16
      return launch<8, 4, 1, 2, 1, 2>(x, ldx, w, sz, bias, y, ldy, M, N, K, s);
    default: return -4;
  }
}

// out[N, K] (bf16) = bf16_rn(float(code - zero) * float(scale)); any N, K % 128 == 0.
extern "C" int dgi_dequant_int4(const void* wq, const void* sz, void* out, int N, int K, hipStream_t s) {
  if (N <= 0 || K <= 0) return 0;
  if (K % 128) return -3;
  const long long dwords = (long long)N * (K / 8);
  const long long blocks = (dwords + 255) / 256;
  if (blocks > 0x7fffffffLL) return -2;
  dequant_int4_kernel<<<dim3((unsigned)blocks), 256, 0, s>>>((const uint32_t*)wq, (const uint32_t*)sz,
                                                             (uint16_t*)out, dwords, K);
  DGI_CHECK_LAUNCH();
  return 0;
}
