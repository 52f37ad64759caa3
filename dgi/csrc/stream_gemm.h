// dgi/csrc/stream_gemm.h — the K-split register-ring core of the weight-streaming GEMMs
// (skinny_gemm.hip, skinny_gemm_fp8.hip, skinny_gemm_mxfp4.hip, skinny_gemm_int4.hip, and
// moe_gemm / moe_gemm_w8 in moe.hip and moe_gemm_w4 in moe_int4.hip: the grouped kernel of
// moe_gemm.h over Bf16W, over E4m3W and over Int4GroupW).
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
// A format whose scale is no power of two cannot put it into the B operand without rounding the
// weight.  Such a format sets kGroupFrags > 0 (Int4W: 4 fragments = one 128-element quantisation
// group): its fragments then take the natural K order (fragment q covers 32 contiguous elements,
// so an MFMA never mixes two groups), each run of kGroupFrags fragments is multiplied into a
// group accumulator of its own, next to the group's row sums of X (the same fragments against a
// B operand of ones, once for all weight tiles), and Format::fold adds the group to the tile's
// accumulator in fp32.  kGroupFrags = 0 is the plain path, unchanged.  Two compile-time flags of a
// grouped format: kNaturalK (false: the lane's bytes stay contiguous, as on the plain path — right
// where a whole step is one group) and kRowSums (false: a format without a zero point issues no
// row-sum MFMAs and folds with fold(acc, group, wfrag, h)).
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
  static constexpr int kStep = 64, kXFrags = 2, kGroupFrags = 0;
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
  static constexpr int kStep = 128, kXFrags = 4, kGroupFrags = 0;
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

// E4m3W's codes with one fp32 scale per 16-row weight tile and 128-deep K step (the 128 x 128 block
// scales of the published FP8 checkpoints, expanded to 16 rows at load): w[n, k] = code[n, k] *
// s[n / 16, k / 128], s [N/16, K/128].  A block scale is no power of two, so it stays out of the B
// operand: a step is one group of the core's grouped path, the codes are widened exactly as
// E4m3W's (same bytes, same K order inside the step), the step's four MFMAs run into a group
// accumulator and fold adds scale * group in fp32.  There is no zero point, hence no row sums.
// The scale of (tile, step) is the same for every lane of the wave: its address is made uniform
// (readfirstlane), so it arrives through the scalar cache, and it is loaded with the step's codes
// into the ring — the fold waits on nothing.
struct E4m3BlockW {
  static constexpr int kStep = 128, kXFrags = 4, kGroupFrags = 4;
  static constexpr bool kNaturalK = false, kRowSums = false;
  struct Mat {
    const uint8_t* q;
    const float* s;
  };
  using Ptr = Mat;
  struct WFrag {
    u32x4 v[2];
    float s;
  };
  // rows n0 .. n0 + 15 of a tile share row >> 4; wave w starts at step w
  static __device__ __forceinline__ Ptr ptr(Mat W, size_t row, int K, int g, int w) {
    const int tile = __builtin_amdgcn_readfirstlane((int)(row >> 4));
    const int w0 = __builtin_amdgcn_readfirstlane(w);
    return Ptr{W.q + row * K + g * 32 + (size_t)w * 128, W.s + (size_t)tile * (K >> 7) + w0};
  }
  static __device__ __forceinline__ Ptr rows(Ptr p, size_t n, int K) {
    return Ptr{p.q + n * K, p.s + (n >> 4) * (K >> 7)};
  }
  static __device__ __forceinline__ void load(WFrag& f, Ptr p, size_t step) {
    const u32x4* q = reinterpret_cast<const u32x4*>(p.q + step * 128);
    f.v[0] = __builtin_nontemporal_load(q);
    f.v[1] = __builtin_nontemporal_load(q + 1);
    f.s = p.s[step];
  }
  static __device__ __forceinline__ bf16x8 b_operand(const WFrag& f, NoScales, int q) {
    const u32x4& v = f.v[q >> 1];
    return widen8(v[2 * (q & 1)], v[2 * (q & 1) + 1]);
  }
  // one explicit fma per accumulator register and step: every instantiation rounds alike
  static __device__ __forceinline__ f32x4 fold(f32x4 acc, f32x4 ag, const WFrag& f, int) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(f.s, ag[i], acc[i]);
    return acc;
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
  static constexpr int kStep = 256, kXFrags = 8, kGroupFrags = 0;
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

// INT4 codes with an fp16 scale and a 4-bit zero point per 128 elements of a row (G = 128):
// w[n, k] = (code - zero[n, k / 128]) * scale[n, k / 128].  The layout is this kernel's own, made
// by the loader (dgi/ops/int4.py): q [N, K/8] dwords of 8 codes and sz [N, K/128] dwords of one
// group's scale and zero point.
//   q   Group h of a row is 16 dwords; dword 4g + c of it holds k = 128h + 32c + 8g + j, j = 0..7,
//       element j in nibble (j >> 1) + 4 (j & 1).  Lane group g reads 16 bytes of each of the
//       step's two groups: together the 128-byte line, and fragment q = 4h + c is one dword whose
//       8 codes lie in a single quantisation group, in the MFMA's natural K order.
//   sz  low half: the scale's fp16 bits; high half: 0x4300 + zero, the bf16 bits of 128 + zero.
// (dword >> 4p) & 0x000F000F | 0x43004300 is the bf16 pair (128 + code[2p], 128 + code[2p+1]),
// exactly: the B operand costs two bit operations per pair and no conversion.  The core's
// grouped path then gives ag = sum x (128 + code) and xs = sum x per group, and fold adds
// scale * (ag - (128 + zero) * xs) = scale * sum x (code - zero) in fp32: the weight is never
// rounded.  Both fmas are explicit, so every instantiation rounds alike.
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

struct Int4W {
  static constexpr int kStep = 256, kXFrags = 8, kGroupFrags = 4;
  static constexpr bool kNaturalK = true, kRowSums = true;
  struct Mat {
    const uint32_t* q;
    const uint32_t* sz;
  };
  using Ptr = Mat;
  struct WFrag {
    u32x4 v[2];
    u32x2 sz;
  };
  // a step is 32 dwords of codes and 2 dwords of scale / zero per row
  static __device__ __forceinline__ Ptr ptr(Mat W, size_t row, int K, int g, int w) {
    return Ptr{W.q + row * (K >> 3) + g * 4 + (size_t)w * 32, W.sz + row * (K >> 7) + (size_t)w * 2};
  }
  static __device__ __forceinline__ Ptr rows(Ptr p, size_t n, int K) {
    return Ptr{p.q + n * (K >> 3), p.sz + n * (K >> 7)};
  }
  static __device__ __forceinline__ void load(WFrag& f, Ptr p, size_t step) {
    const u32x4* q = reinterpret_cast<const u32x4*>(p.q + step * 32);
    f.v[0] = __builtin_nontemporal_load(q);
    f.v[1] = __builtin_nontemporal_load(q + 4);
    f.sz = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p.sz + step * 2));
  }
  static __device__ __forceinline__ bf16x8 ones() {
    return as_bf16x8(u32x4{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u});
  }
  // WF: this format's WFrag or Int4GroupW's (v and sz index alike)
  template <class WF>
  static __device__ __forceinline__ bf16x8 b_operand(const WF& f, NoScales, int q) {
    const uint32_t c = f.v[q >> 2][q & 3];
    u32x4 r;
#pragma unroll
    for (int p = 0; p < 4; ++p) r[p] = ((c >> (4 * p)) & 0x000f000fu) | 0x43004300u;
    return as_bf16x8(r);
  }
  template <class WF>
  static __device__ __forceinline__ f32x4 fold(f32x4 acc, f32x4 ag, f32x4 xs, const WF& f, int h) {
    const uint32_t w = f.sz[h];
    const float sc = (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu));
    const float nz = -__uint_as_float(w & 0xffff0000u);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = __builtin_fmaf(sc, __builtin_fmaf(nz, xs[i], ag[i]), acc[i]);
    return acc;
  }
};

// Int4W's rows read one quantisation group per step: 128 deep, 64 bytes of codes and one sz dword
// per row.  Lane group g reads the 16 contiguous bytes of dwords 4g .. 4g + 3 of group h = step
// (fragment c = dword 4g + c, k = 128·step + 32c + 8g + j); the four lane groups of a row read the
// same sz dword.  A K of any multiple of 256 then has an even step count, which 2 waves always
// divide and 4 do when K % 512 == 0: the grouped expert GEMM's geometry (moe_int4.hip), whose K
// of 768 is three of Int4W's steps.  The operand and the fold are Int4W's.
struct Int4GroupW : Int4W {
  static constexpr int kStep = 128, kXFrags = 4, kGroupFrags = 4;
  struct WFrag {
    u32x4 v[1];
    uint32_t sz[1];
  };
  static __device__ __forceinline__ Ptr ptr(Mat W, size_t row, int K, int g, int w) {
    return Ptr{W.q + row * (K >> 3) + g * 4 + (size_t)w * 16, W.sz + row * (K >> 7) + (size_t)w};
  }
  static __device__ __forceinline__ void load(WFrag& f, Ptr p, size_t step) {
    f.v[0] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p.q + step * 16));
    f.sz[0] = __builtin_nontemporal_load(p.sz + step);
  }
};

// whether a format's fragments take the natural K order (grouped formats say; the plain path never does)
template <class F>
constexpr bool natural_k() {
  if constexpr (F::kGroupFrags > 0) return F::kNaturalK;
  else return false;
}

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
  constexpr bool kGrouped = F::kGroupFrags > 0;
  constexpr bool kNatural = natural_k<F>();
  typename F::Ptr wrow[WT];
#pragma unroll
  for (int t = 0; t < WT; ++t) wrow[t] = wptr_of(t, r, g, w);
  const uint16_t* xrow[MT];
  bool xval[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = xrow_of(mt * 16 + r);
    xval[mt] = row >= 0;
    // lane group g: a quarter of the step (fragments 8 elements apart), or, for a format in the
    // natural K order, its 8 elements of every 32 (fragments 32 apart: the MFMA's own A layout)
    xrow[mt] = X + (size_t)(xval[mt] ? row : 0) * ldx + g * (kNatural ? 8 : F::kStep / 4) + w * F::kStep;
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
          for (int q = 0; q < F::kXFrags; ++q) f.x[u][mt][q] = p[kNatural ? 4 * q : q];
        } else {  // rows that do not exist read nothing
#pragma unroll
          for (int q = 0; q < F::kXFrags; ++q) f.x[u][mt][q] = u32x4{0u, 0u, 0u, 0u};
        }
      }
    }
  };
  auto compute = [&](const Frag& f) {
    if constexpr (kGrouped) {
      constexpr int GF = F::kGroupFrags;
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int h = 0; h < F::kXFrags / GF; ++h) {
          // the group's row sums of X: every column of X · 1 is the sum, so the lane holds rows
          // 4g .. 4g + 3 of it next to the same rows of its accumulators
          f32x4 xs[MT];
          if constexpr (F::kRowSums) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              xs[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int q = h * GF; q < (h + 1) * GF; ++q)
                xs[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(f.x[u][mt][q]), F::ones(), xs[mt], 0, 0, 0);
            }
          }
#pragma unroll
          for (int t = 0; t < WT; ++t) {
            f32x4 ag[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) ag[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = h * GF; q < (h + 1) * GF; ++q) {
              const bf16x8 b = F::b_operand(f.w[u][t], NoScales{}, q);
#pragma unroll
              for (int mt = 0; mt < MT; ++mt)
                ag[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(f.x[u][mt][q]), b, ag[mt], 0, 0, 0);
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              if constexpr (F::kRowSums)
                acc[mt][t] = F::fold(acc[mt][t], ag[mt], xs[mt], f.w[u][t], h);
              else
                acc[mt][t] = F::fold(acc[mt][t], ag[mt], f.w[u][t], h);
            }
          }
        }
    } else {
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
