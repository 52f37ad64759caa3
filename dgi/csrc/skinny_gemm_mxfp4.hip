// dgi/csrc/skinny_gemm_mxfp4.hip — W4A16 weight-streaming GEMM for decode-sized M over OCP
// MXFP4 weights, and the mxfp4 -> bf16 dequantiser behind every shape it does not take.
//
// Y[M, N] = X[M, K] · W[N, K]^T (+ bias[N]): bf16 X / Y / bias, fp32 accumulate, M <= 32.
// W is OCP Microscaling FP4: q[N, K/2] bytes of two e2m1 codes (element 2j in the low nibble of
// byte j, 2j+1 in the high one) and scale[N, K/32] e8m0 bytes, one per 32 elements of a row;
// the weight is elem * 2^(scale - 127).
//
// Same skeleton as skinny_gemm_fp8.hip (one workgroup per 16·NT output columns, NW waves
// splitting K, weights straight from HBM to VGPRs with nontemporal 16-byte loads, a register
// ring of D groups of U K-steps, LDS sum of the NW partial tiles, v_mfma_f32_16x16x32_bf16),
// with half the weight bytes again:
//
//  * a K step is 256 deep: lane l still reads 32 contiguous bytes of weight row n0 + (l & 15),
//    now 64 elements = two scale blocks, whose two e8m0 bytes it reads as one 16-bit load;
//  * fragment f (0..7) of lane group g holds k = 256·step + 64g + 8f + j: one dword of codes,
//    decoded by four v_cvt_scalef32_pk_bf16_fp4 (op_sel picks the byte, low nibble first) with
//    the block's scale as fp32 (code << 23).  X is read in the same order, 128 contiguous
//    bytes per lane, step and row tile (from L2);
//  * every decoded value is exact in bf16 (one mantissa bit times a power of two, a normal
//    number for scale codes 2..252), so the kernel's only roundings are the fp32 accumulation
//    order and the final bf16 store.  The dequantiser writes the same bf16 values, so both
//    routes of ops.linear multiply the same numbers.
//
// Scale codes outside 2..252 are outside the format as this project specifies it: they may
// decode to something else, but no address depends on a code.
#include "common.h"

using namespace dgi;

namespace {

// 8 e2m1 codes (one dword) times one fp32 scale -> 8 bf16 (one MFMA operand / 16 bytes)
__device__ __forceinline__ u32x4 decode8(uint32_t codes, float sc) {
  u32x4 r;
  r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, sc, 0));
  r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, sc, 1));
  r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, sc, 2));
  r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, sc, 3));
  return r;
}

__device__ __forceinline__ float e8m0_to_f32(uint32_t code) { return __uint_as_float(code << 23); }

// Fragments of U K-steps: 64 codes and two scales of W per column tile, 8 x 8 bf16 of X per row tile.
template <int MT, int NT, int U>
struct Frag4 {
  u32x4 w[U][NT][2];
  uint32_t s[U][NT];
  u32x4 x[U][MT][8];
};

template <int NW, int MT, int NT, int U, int D>
__global__ __launch_bounds__(NW * 64) void skinny_gemm_w4_kernel(
    const uint16_t* __restrict__ X, int ldx, const uint8_t* __restrict__ W, const uint8_t* __restrict__ S,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ Y, int ldy, int M, int K) {
  __shared__ f32x4 red[NW][MT * NT][64];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int r = lane & 15;
  const int g = lane >> 4;
  const int n0 = blockIdx.x * 16 * NT;
  // host guarantees (K / 256) % (NW * U) == 0: every group is full, no predicates in the stream
  const int ngroups = (K >> 8) / (NW * U);
  // a step is 128 bytes of codes, 8 bytes of scales and 256 elements of X per row
  const uint8_t* wrow = W + (size_t)(n0 + r) * (K >> 1) + g * 32 + (size_t)w * 128;
  const uint8_t* srow = S + (size_t)(n0 + r) * (K >> 5) + g * 2 + (size_t)w * 8;
  const size_t wtile = (size_t)16 * (K >> 1);  // next column tile
  const size_t stile = (size_t)16 * (K >> 5);
  const uint16_t* xrow[MT];
  bool xval[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = mt * 16 + r;
    xval[mt] = m < M;
    xrow[mt] = X + (size_t)(xval[mt] ? m : 0) * ldx + g * 64 + w * 256;
  }
  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto load = [&](Frag4<MT, NT, U>& f, int grp) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t step = (size_t)grp * NW * U + (size_t)u * NW;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const u32x4* p = reinterpret_cast<const u32x4*>(wrow + nt * wtile + step * 128);
        f.w[u][nt][0] = __builtin_nontemporal_load(p);
        f.w[u][nt][1] = __builtin_nontemporal_load(p + 1);
        f.s[u][nt] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(srow + nt * stile + step * 8));
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if (xval[mt]) {
          const u32x4* p = reinterpret_cast<const u32x4*>(xrow[mt] + step * 256);
#pragma unroll
          for (int q = 0; q < 8; ++q) f.x[u][mt][q] = p[q];
        } else {
#pragma unroll
          for (int q = 0; q < 8; ++q) f.x[u][mt][q] = u32x4{0u, 0u, 0u, 0u};
        }
      }
    }
  };
  auto compute = [&](const Frag4<MT, NT, U>& f) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        // the lane's two scale blocks: elements 0..31 (fragments 0-3) and 32..63 (fragments 4-7)
        const float sc[2] = {e8m0_to_f32(f.s[u][nt] & 0xffu), e8m0_to_f32(f.s[u][nt] >> 8)};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const bf16x8 b = as_bf16x8(decode8(f.w[u][nt][q >> 2][q & 3], sc[q >> 2]));
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(f.x[u][mt][q]), b, acc[mt][nt], 0, 0, 0);
        }
      }
  };
  // register ring of D groups: D - 1 in flight ahead of the one being multiplied
  Frag4<MT, NT, U> ring[D];
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (d < ngroups) load(ring[d], d);
  for (int base = 0; base < ngroups; base += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (base + d < ngroups) {  // uniform
        compute(ring[d]);
        if (base + D + d < ngroups) load(ring[d], base + D + d);
      }
    }
  }

#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) red[w][mt * NT + nt][lane] = acc[mt][nt];
  __syncthreads();
  // wave w sums the NW partial tiles of output tiles w, w + NW, ...
  for (int t = w; t < MT * NT; t += NW) {
    f32x4 v = red[0][t][lane];
#pragma unroll
    for (int j = 1; j < NW; ++j) v += red[j][t][lane];
    const int mt = t / NT, nt = t % NT;
    const int col = n0 + nt * 16 + r;
    const float b = bias ? bf16_to_f32(bias[col]) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = mt * 16 + g * 4 + i;
      if (m < M) Y[(size_t)m * ldy + col] = f32_to_bf16(v[i] + b);
    }
  }
}

template <int NW, int MT, int NT, int U, int D>
int launch(const void* x, int ldx, const void* w, const void* scale, const void* bias, void* y, int ldy, int M,
           int N, int K, hipStream_t s) {
  if (N % (16 * NT) || (K / 256) % (NW * U)) return -5;
  skinny_gemm_w4_kernel<NW, MT, NT, U, D><<<dim3(N / (16 * NT)), NW * 64, 0, s>>>(
      (const uint16_t*)x, ldx, (const uint8_t*)w, (const uint8_t*)scale, (const uint16_t*)bias, (uint16_t*)y, ldy,
      M, K);
  DGI_CHECK_LAUNCH();
  return 0;
}

// The X fragment of a step is twice the fp8 kernel's (8 x u32x4 per row tile), so the ring of the
// two-row-tile instantiations (M > 16) is at most two groups deep, and a single group with four
// column tiles on 8 waves (256 registers per lane): deeper rings spill to scratch there.
template <int MT>
int dispatch(int cfg, const void* x, int ldx, const void* w, const void* scale, const void* bias, void* y, int ldy,
             int M, int N, int K, hipStream_t s) {
  constexpr int D4 = MT == 1 ? 4 : 2;
  constexpr int D8 = MT == 1 ? 2 : 1;
  switch (cfg) {
    case 1: return launch<4, MT, 1, 1, D4>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);
    case 2: return launch<4, MT, 1, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);
    case 3: return launch<8, MT, 1, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);   // K % 2048
    case 4: return launch<8, MT, 1, 1, D4>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);  // K % 2048
    case 5: return launch<4, MT, 2, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);   // N % 32
    case 6: return launch<8, MT, 2, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);   // N % 32, K % 2048
    case 7: return launch<4, MT, 4, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);   // N % 64
    case 8: return launch<8, MT, 4, 1, D8>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);   // N % 64, K % 2048
    default: return -4;
  }
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
  return M > 16 ? dispatch<2>(cfg, x, ldx, w, scale, bias, y, ldy, M, N, K, s)
                : dispatch<1>(cfg, x, ldx, w, scale, bias, y, ldy, M, N, K, s);
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
