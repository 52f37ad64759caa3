// dgi/csrc/skinny_gemm_fp8.hip — W8A16 weight-streaming GEMM for decode-sized M, and the
// fp8 -> bf16 dequantiser behind every shape it does not take.
//
// Y[M, N] = (X[M, K] · Wq[N, K]^T) * scale[N] (+ bias[N]): bf16 X / Y / bias, OCP e4m3
// (``float8_e4m3fn``, not fnuz) weights with one fp32 scale per output channel, fp32
// accumulate, M <= 32.
//
// Same shape as skinny_gemm.hip (one workgroup per 16·NT output columns, NW waves splitting
// K, weights straight from HBM to VGPRs with nontemporal 16-byte loads, a register ring of D
// groups of U K-steps, LDS sum of the NW partial tiles), with half the weight bytes:
//
//  * a K step is 128 deep, so lane l still reads 32 contiguous bytes of weight row
//    n0 + (l & 15) and the 4 lane groups still cover a whole 128-byte line of each row;
//  * the 32 e4m3 values are widened in registers to four bf16 B fragments of
//    v_mfma_f32_16x16x32_bf16: v_cvt_pk_f32_fp8 gives two fp32 per instruction and every
//    finite e4m3 value is exact in bf16, so packing the upper halves of the two fp32 words
//    (one v_perm_b32) loses nothing — subnormals and signed zeros included;
//  * fragment f of lane group g holds k = 128·step + 32g + 8f + j, and X is read in the same
//    order (64 contiguous bytes per lane and step, from L2);
//  * the epilogue multiplies the fp32 sum by scale[col], adds the bias and rounds once.
#include "common.h"

using namespace dgi;

namespace {

// Fragments of U K-steps: 32 fp8 of W per column tile, 4 x 8 bf16 of X per row tile.
template <int MT, int NT, int U>
struct Frag8 {
  u32x4 w[U][NT][2];
  u32x4 x[U][MT][4];
};

template <int NW, int MT, int NT, int U, int D>
__global__ __launch_bounds__(NW * 64) void skinny_gemm_w8_kernel(
    const uint16_t* __restrict__ X, int ldx, const uint8_t* __restrict__ W, const float* __restrict__ scale,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ Y, int ldy, int M, int K) {
  __shared__ f32x4 red[NW][MT * NT][64];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int r = lane & 15;
  const int g = lane >> 4;
  const int n0 = blockIdx.x * 16 * NT;
  // host guarantees (K / 128) % (NW * U) == 0: every group is full, no predicates in the stream
  const int ngroups = (K >> 7) / (NW * U);
  const uint8_t* wrow = W + (size_t)(n0 + r) * K + g * 32 + (size_t)w * 128;
  const size_t wtile = (size_t)16 * K;  // next column tile
  const uint16_t* xrow[MT];
  bool xval[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = mt * 16 + r;
    xval[mt] = m < M;
    xrow[mt] = X + (size_t)(xval[mt] ? m : 0) * ldx + g * 32 + w * 128;
  }
  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto load = [&](Frag8<MT, NT, U>& f, int grp) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t off = ((size_t)grp * NW * U + (size_t)u * NW) * 128;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const u32x4* p = reinterpret_cast<const u32x4*>(wrow + nt * wtile + off);
        f.w[u][nt][0] = __builtin_nontemporal_load(p);
        f.w[u][nt][1] = __builtin_nontemporal_load(p + 1);
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if (xval[mt]) {
          const u32x4* p = reinterpret_cast<const u32x4*>(xrow[mt] + off);
#pragma unroll
          for (int q = 0; q < 4; ++q) f.x[u][mt][q] = p[q];
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) f.x[u][mt][q] = u32x4{0u, 0u, 0u, 0u};
        }
      }
    }
  };
  auto compute = [&](const Frag8<MT, NT, U>& f) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          // bytes 8q .. 8q+7 of the lane's 32: words 2(q&1), 2(q&1)+1 of 16-byte half q>>1
          const u32x4& v = f.w[u][nt][q >> 1];
          const bf16x8 b = widen8(v[2 * (q & 1)], v[2 * (q & 1) + 1]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(f.x[u][mt][q]), b, acc[mt][nt], 0, 0, 0);
        }
  };
  // register ring of D groups: D - 1 in flight ahead of the one being multiplied
  Frag8<MT, NT, U> ring[D];
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
  // wave w (< MT*NT) sums the NW partial tiles of output tile w
  if (w >= MT * NT) return;
  f32x4 v = red[0][w][lane];
#pragma unroll
  for (int j = 1; j < NW; ++j) v += red[j][w][lane];
  const int mt = w / NT, nt = w % NT;
  const int col = n0 + nt * 16 + r;
  const float sc = scale[col];
  const float b = bias ? bf16_to_f32(bias[col]) : 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = mt * 16 + g * 4 + i;
    if (m < M) Y[(size_t)m * ldy + col] = f32_to_bf16(v[i] * sc + b);
  }
}

template <int NW, int MT, int NT, int U, int D>
int launch(const void* x, int ldx, const void* w, const void* scale, const void* bias, void* y, int ldy, int M,
           int N, int K, hipStream_t s) {
  static_assert(NW >= MT * NT, "one wave per output tile in the reduction");
  if (N % (16 * NT) || (K / 128) % (NW * U)) return -5;
  skinny_gemm_w8_kernel<NW, MT, NT, U, D><<<dim3(N / (16 * NT)), NW * 64, 0, s>>>(
      (const uint16_t*)x, ldx, (const uint8_t*)w, (const float*)scale, (const uint16_t*)bias, (uint16_t*)y, ldy, M,
      K);
  DGI_CHECK_LAUNCH();
  return 0;
}

template <int MT>
int dispatch(int cfg, const void* x, int ldx, const void* w, const void* scale, const void* bias, void* y, int ldy,
             int M, int N, int K, hipStream_t s) {
  switch (cfg) {
    case 1: return launch<8, MT, 1, 1, 4>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);
    case 2: return launch<8, MT, 1, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);
    case 3: return launch<4, MT, 1, 2, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);
    case 4: return launch<4, MT, 1, 2, 4>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);
    case 5: return launch<8, MT, 2, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);   // N % 32
    case 6: return launch<4, MT, 1, 1, 8>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);
    case 7: return launch<16, MT, 1, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);  // K % 2048
    case 8: return launch<8, MT, 4, 1, 2>(x, ldx, w, scale, bias, y, ldy, M, N, K, s);   // N % 64
    default: return -4;
  }
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
  return M > 16 ? dispatch<2>(cfg, x, ldx, w, scale, bias, y, ldy, M, N, K, s)
                : dispatch<1>(cfg, x, ldx, w, scale, bias, y, ldy, M, N, K, s);
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
