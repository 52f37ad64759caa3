// dgi/csrc/stream_gemm.h — the K-split register-ring core of the weight-streaming GEMMs
// (skinny_gemm.hip, skinny_gemm_fp8.hip, skinny_gemm_mxfp4.hip, and moe_gemm / moe_gemm_w8 in
// moe.hip: the grouped kernel over Bf16W and over E4m3W).
//
// Y[M, N] = X[M, K] · W[N, K]^T for decode-sized M.  At these sizes every projection is a read
// of its weight matrix: the FLOPs are free and the kernel's job is to keep HBM3E streaming.
// hipBLASLt's tiles for M = 1..32 leave most of the ~6 TB/s unused, so the kernel is shaped
// around the weight stream instead of the output tile:
//
//  * one workgroup per 16·NT output columns, NW waves splitting K between them (step s belongs
//    to wave s % NW);
//  * lane l reads 32 contiguous bytes of weight row n0 + (l & 15) per K step: the 4 lane groups
//    cover a full 128-byte line of each of the 16 rows, loaded straight to VGPRs (no LDS round
//    trip — the operand is used once) with nontemporal loads.  A step is as many elements of K
//    as 128 bytes of the weight format hold (Format::kStep);
//  * the format turns the lane's 32 bytes into kStep / 32 B fragments of
//    v_mfma_f32_16x16x32_bf16 (lane holds B[k = 8(l>>4)+j][col l&15]); the K order inside a
//    step is permuted identically for X, which a dot product does not see.  X rows (A
//    fragments, 16 per MFMA, zero for rows that do not exist) come from L2 — X is tiny and
//    every workgroup reads the same bytes;
//  * loads run D - 1 groups of U K-steps ahead of the MFMAs (register ring, D = 2 is the
//    double buffer).  The host guarantees that the steps divide into full groups, so the
//    stream carries no predicates;
//  * the NW partial 16x16 tiles are summed through LDS in wave order and handed to an epilogue.
// MT = 2 handles 17..32 rows with the same weight registers (two A tiles); more than one weight
// tile per wave reuses each X fragment.
//
// Every accumulator sees its MFMAs in K-step order, fragments ascending within a step, and the
// partial tiles are added in wave order: results do not depend on MT, the tile count or D.
//
// Not here: fused_decode.hip.  Its three kernels interleave the norm prologue and a persistent
// tile cursor with the ring; sharing that is a different job.
#pragma once
#include "common.h"

namespace dgi {

// ---- weight formats: kStep elements of K per step, kXFrags = kStep / 32 fragments of X per row
// tile and step, the lane's registers of one step and weight tile (WFrag), and how they load
// and become B operands.  Mat is the matrix as the kernel receives it, Ptr the lane's place in
// one of its rows (lane group g, wave w); rows(p, n, K) is the same place n rows further on.

struct WFrag32 {
  u32x4 v[2];
};
struct NoScales {};

struct Bf16W {
  static constexpr int kStep = 64, kXFrags = 2;
  using Mat = const uint16_t*;
  using Ptr = const uint16_t*;
  using WFrag = WFrag32;
  static __device__ __forceinline__ Ptr ptr(Mat W, size_t row, int K, int g, int w) {
    return W + row * K + g * 16 + (size_t)w * 64;
  }
  static __device__ __forceinline__ Ptr rows(Ptr p, size_t n, int K) { return p + n * K; }
  static __device__ __forceinline__ void load(WFrag& f, Ptr p, size_t step) {
    const u32x4* q = reinterpret_cast<const u32x4*>(p + step * 64);
    f.v[0] = __builtin_nontemporal_load(q);
    f.v[1] = __builtin_nontemporal_load(q + 1);
  }
  static __device__ __forceinline__ NoScales scales(const WFrag&) { return {}; }
  static __device__ __forceinline__ bf16x8 b_operand(const WFrag& f, NoScales, int q) { return as_bf16x8(f.v[q]); }
};

// OCP e4m3, widened in registers: every finite e4m3 value is exact in bf16.  Fragment q of lane
// group g holds k = 128·step + 32g + 8q + j.
struct E4m3W {
  static constexpr int kStep = 128, kXFrags = 4;
  using Mat = const uint8_t*;
  using Ptr = const uint8_t*;
  using WFrag = WFrag32;
  static __device__ __forceinline__ Ptr ptr(Mat W, size_t row, int K, int g, int w) {
    return W + row * K + g * 32 + (size_t)w * 128;
  }
  static __device__ __forceinline__ Ptr rows(Ptr p, size_t n, int K) { return p + n * K; }
  static __device__ __forceinline__ void load(WFrag& f, Ptr p, size_t step) {
    const u32x4* q = reinterpret_cast<const u32x4*>(p + step * 128);
    f.v[0] = __builtin_nontemporal_load(q);
    f.v[1] = __builtin_nontemporal_load(q + 1);
  }
  // bytes 8q .. 8q+7 of the lane's 32: words 2(q&1), 2(q&1)+1 of 16-byte half q>>1
  static __device__ __forceinline__ NoScales scales(const WFrag&) { return {}; }
  static __device__ __forceinline__ bf16x8 b_operand(const WFrag& f, NoScales, int q) {
    const u32x4& v = f.v[q >> 1];
    return widen8(v[2 * (q & 1)], v[2 * (q & 1) + 1]);
  }
};

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

// OCP MXFP4: q [N, K/2] bytes of two e2m1 codes, s [N, K/32] e8m0 bytes.  The lane's 32 bytes are
// 64 elements = two scale blocks, whose two e8m0 bytes it reads as one 16-bit load.  Fragment q
// (0..7) of lane group g holds k = 256·step + 64g + 8q + j: one dword of codes, decoded by four
// v_cvt_scalef32_pk_bf16_fp4 (op_sel picks the byte, low nibble first) with the block's scale.
struct Mxfp4W {
  static constexpr int kStep = 256, kXFrags = 8;
  struct Mat {
    const uint8_t* q;
    const uint8_t* s;
  };
  using Ptr = Mat;
  struct WFrag {
    u32x4 v[2];
    uint32_t s;
  };
  // a step is 128 bytes of codes and 8 bytes of scales per row
  static __device__ __forceinline__ Ptr ptr(Mat W, size_t row, int K, int g, int w) {
    return Ptr{W.q + row * (K >> 1) + g * 32 + (size_t)w * 128, W.s + row * (K >> 5) + g * 2 + (size_t)w * 8};
  }
  static __device__ __forceinline__ Ptr rows(Ptr p, size_t n, int K) {
    return Ptr{p.q + n * (K >> 1), p.s + n * (K >> 5)};
  }
  static __device__ __forceinline__ void load(WFrag& f, Ptr p, size_t step) {
    const u32x4* q = reinterpret_cast<const u32x4*>(p.q + step * 128);
    f.v[0] = __builtin_nontemporal_load(q);
    f.v[1] = __builtin_nontemporal_load(q + 1);
    f.s = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p.s + step * 8));
  }
  // the lane's two scale blocks: low byte for fragments 0-3, high byte for 4-7; both are
  // converted ahead of the step's first decode, not in front of fragment 4's
  struct Scales {
    float v[2];
  };
  static __device__ __forceinline__ Scales scales(const WFrag& f) {
    return Scales{{e8m0_to_f32(f.s & 0xffu), e8m0_to_f32(f.s >> 8)}};
  }
  static __device__ __forceinline__ bf16x8 b_operand(const WFrag& f, const Scales& sc, int q) {
    return as_bf16x8(decode8(f.v[q >> 2][q & 3], sc.v[q >> 2]));
  }
};

// Fragments of U K-steps: W for WT weight tiles, X for MT row tiles.
template <class F, int MT, int WT, int U>
struct StreamFrag {
  typename F::WFrag w[U][WT];
  u32x4 x[U][MT][F::kXFrags];
};

// The core.  WT weight tiles and MT row tiles per wave, hence MT x WT accumulators;
//   xrow(m)           row of X behind local row m (0 .. 16·MT - 1), or < 0 for a row of zeros;
//   wptr(t, r, g, w)  the lane's place (Format::ptr) in the row of W behind column r of weight tile t;
//   epi(mt, ot, r, g, tile)  for each of the MT x OT output tiles, run by one wave: tile(t) is
//             the sum over the waves of accumulator (mt, t); the lane holds rows 4g .. 4g + 3
//             of column r.
// The host guarantees (K / F::kStep) % (NW * U) == 0.  Every wave of the workgroup must call.
template <class F, int NW, int MT, int WT, int OT, int U, int D, class XRow, class WPtr, class Epi>
__device__ __forceinline__ void stream_gemm(const uint16_t* __restrict__ X, int ldx, int K, XRow xrow_of,
                                            WPtr wptr_of, Epi epi) {
  __shared__ f32x4 red[NW][MT * WT][64];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int r = lane & 15;
  const int g = lane >> 4;
  const int ngroups = (K >> __builtin_ctz(F::kStep)) / (NW * U);
  typename F::Ptr wrow[WT];
#pragma unroll
  for (int t = 0; t < WT; ++t) wrow[t] = wptr_of(t, r, g, w);
  const uint16_t* xrow[MT];
  bool xval[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = xrow_of(mt * 16 + r);
    xval[mt] = row >= 0;
    xrow[mt] = X + (size_t)(xval[mt] ? row : 0) * ldx + g * (F::kStep / 4) + w * F::kStep;
  }
  f32x4 acc[MT][WT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < WT; ++t) acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  using Frag = StreamFrag<F, MT, WT, U>;
  auto load = [&](Frag& f, int grp) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t step = (size_t)grp * NW * U + (size_t)u * NW;
#pragma unroll
      for (int t = 0; t < WT; ++t) F::load(f.w[u][t], wrow[t], step);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if (xval[mt]) {
          const u32x4* p = reinterpret_cast<const u32x4*>(xrow[mt] + step * F::kStep);
#pragma unroll
          for (int q = 0; q < F::kXFrags; ++q) f.x[u][mt][q] = p[q];
        } else {  // rows that do not exist read nothing
#pragma unroll
          for (int q = 0; q < F::kXFrags; ++q) f.x[u][mt][q] = u32x4{0u, 0u, 0u, 0u};
        }
      }
    }
  };
  auto compute = [&](const Frag& f) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int t = 0; t < WT; ++t) {
        const auto sc = F::scales(f.w[u][t]);
#pragma unroll
        for (int q = 0; q < F::kXFrags; ++q) {
          const bf16x8 b = F::b_operand(f.w[u][t], sc, q);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(f.x[u][mt][q]), b, acc[mt][t], 0, 0, 0);
        }
      }
  };
  // register ring of D groups: D - 1 in flight ahead of the one being multiplied
  Frag ring[D];
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
    for (int t = 0; t < WT; ++t) red[w][mt * WT + t][lane] = acc[mt][t];
  __syncthreads();
  // wave w finishes output tiles w, w + NW, ...
  for (int o = w; o < MT * OT; o += NW) {
    const int mt = o / OT;
    epi(mt, o % OT, r, g, [&](int t) {
      f32x4 v = red[0][mt * WT + t][lane];
#pragma unroll
      for (int j = 1; j < NW; ++j) v += red[j][mt * WT + t][lane];
      return v;
    });
  }
}

// The dense kernels: rows 0 .. M-1 of X, NT column tiles at n0 + 16·nt, and a per-column
// epilogue fin(v, col) -> f32x4 in front of the row-guarded bf16 store.
template <class F, int NW, int MT, int NT, int U, int D, class Fin>
__device__ __forceinline__ void stream_gemm_dense(const uint16_t* __restrict__ X, int ldx, typename F::Mat W,
                                                  uint16_t* __restrict__ Y, int ldy, int M, int K, Fin fin) {
  const int n0 = blockIdx.x * 16 * NT;
  stream_gemm<F, NW, MT, NT, NT, U, D>(
      X, ldx, K, [&](int m) { return m < M ? m : -1; },
      // one lane base plus a wave-uniform tile offset: one pointer's registers for all NT tiles
      [&](int nt, int r, int g, int w) { return F::rows(F::ptr(W, (size_t)(n0 + r), K, g, w), (size_t)16 * nt, K); },
      [&](int mt, int nt, int r, int g, auto tile) {
        const int col = n0 + nt * 16 + r;
        const f32x4 v = fin(tile(nt), col);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = mt * 16 + g * 4 + i;
          if (m < M) Y[(size_t)m * ldy + col] = f32_to_bf16(v[i]);
        }
      });
}

// Host side of a dense kernel: k1 takes up to 16 rows with NT1 column tiles per wave, k2 up to 32
// with NT2.  -5 and no launch where the geometry does not divide the shape.
template <int kStep, int NW, int U, int NT1, int NT2, class... P, class... A>
int launch_stream_dense(void (*k1)(P...), void (*k2)(P...), int M, int N, int K, hipStream_t s, A... args) {
  const int NT = M > 16 ? NT2 : NT1;
  if (N % (16 * NT) || (K / kStep) % (NW * U)) return -5;
  hipLaunchKernelGGL(M > 16 ? k2 : k1, dim3(N / (16 * NT)), dim3(NW * 64), 0, s, static_cast<P>(args)...);
  DGI_CHECK_LAUNCH();
  return 0;
}

}  // namespace dgi
