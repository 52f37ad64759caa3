// dgi/csrc/common.h — shared device helpers for the gfx950 (CDNA4) kernels.
//
// Everything here is written for wave64 / MFMA on MI355X; there is no
// CUDA or multi-platform path.  bf16 values travel as raw 16-bit patterns
// (ushort) through memory and are widened to fp32 in registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dgi {

constexpr int kWave = 64;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short short4v __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

typedef __attribute__((address_space(3))) short4v lds_short4;

__device__ __forceinline__ float bf16_to_f32(uint16_t v) {
  return __uint_as_float(((uint32_t)v) << 16);
}

typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

// Round-to-nearest-even f32 -> bf16.  Written as a (vector) conversion so hipcc
// emits gfx950's v_cvt_pk_bf16_f32 (one VALU op for two values) instead of the
// 5-6 integer ops of a bit-manipulation RNE — the softmax / norm / epilogue
// loops are VALU-issue-bound and pay for every op here.
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  return __builtin_bit_cast(uint16_t, (__bf16)f);
}

__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  const f32x2v v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2v));
}

// 16-byte vector = 8 bf16.
struct __attribute__((aligned(16))) bf16x8_raw { uint32_t w[4]; };

__device__ __forceinline__ void unpack8(const u32x4& v, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(v[i] << 16);
    f[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ u32x4 pack8(const float* f) {
  u32x4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = pack_bf16x2(f[2 * i], f[2 * i + 1]);
  return r;
}

__device__ __forceinline__ bf16x8 as_bf16x8(const u32x4& v) {
  return __builtin_bit_cast(bf16x8, v);
}

// The 256 x 256 GEMM tiles (mfma_gemm.hip, mfma_gemm_fp8.hip): a lane holds rows
// m0 + 128 wm + 16 i + (lane & 15), columns 4 (lane >> 4) + 0..3 of each 16x16 tile.
// Two neighbouring tiles (A, B) are stored as ONE 16-byte store per lane: v_permlane16_swap
// trades A's columns of the odd 16-lane rows for B's columns of the even rows, so lane group
// g ends up with 8 consecutive columns — A 0-7 (g 0), B 0-7 (g 1), A 8-15 (g 2), B 8-15 (g 3) —
// and every row of a store instruction writes 64 contiguous bytes (half the store
// instructions of 8-byte stores; the store tail of a tile's epilogue is issue-bound).
__device__ __forceinline__ void store_pair16(uint16_t* yrow, int n0, int g, const float (&a)[4], const float (&b)[4]) {
  const uint32_t a01 = pack_bf16x2(a[0], a[1]), a23 = pack_bf16x2(a[2], a[3]);
  const uint32_t b01 = pack_bf16x2(b[0], b[1]), b23 = pack_bf16x2(b[2], b[3]);
  const auto s0 = __builtin_amdgcn_permlane16_swap(a01, b01, false, false);
  const auto s1 = __builtin_amdgcn_permlane16_swap(a23, b23, false, false);
  uint4 v;
  v.x = s0[0];
  v.y = s1[0];
  v.z = s0[1];
  v.w = s1[1];
  *(uint4*)(yrow + n0 + 16 * (g & 1) + 4 * (g & 2)) = v;
}

// ---- e4m3 (OCP float8_e4m3fn) helpers: W8A16 weights and the fp8 KV cache.
// Two e4m3 codes of `word` (low or high half) -> two bf16 in one word.
__device__ __forceinline__ uint32_t widen2(uint32_t word, bool hi) {
  const f32x2v f = hi ? __builtin_amdgcn_cvt_pk_f32_fp8((int)word, true)
                      : __builtin_amdgcn_cvt_pk_f32_fp8((int)word, false);
  // upper halves of the two words, f[0] low (v_perm_b32: selector bytes 0-3 index the second
  // source, 4-7 the first); exact: an e4m3 value has 3 mantissa bits, bf16 keeps 7
  return __builtin_amdgcn_perm(__float_as_uint(f[1]), __float_as_uint(f[0]), 0x07060302u);
}

// 8 e4m3 (two words) -> 8 bf16 (one MFMA operand / one 16-byte LDS chunk)
__device__ __forceinline__ u32x4 widen8_u32(uint32_t a, uint32_t b) {
  u32x4 r;
  r[0] = widen2(a, false);
  r[1] = widen2(a, true);
  r[2] = widen2(b, false);
  r[3] = widen2(b, true);
  return r;
}

__device__ __forceinline__ bf16x8 widen8(uint32_t a, uint32_t b) { return as_bf16x8(widen8_u32(a, b)); }

// KV-cache quantiser: code = rne_e4m3(clamp(x * inv_scale, -448, 448)) for 8 values.  The clamp
// is explicit (selects, so a NaN stays a NaN): the conversion's own overflow mode never matters.
__device__ __forceinline__ uint2 quant8_e4m3(const float* x, float inv_scale) {
  float c[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = x[j] * inv_scale;
    v = v > 448.f ? 448.f : v;
    v = v < -448.f ? -448.f : v;
    c[j] = v;
  }
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(c[4], c[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(c[6], c[7], hi, true);
  return uint2{(uint32_t)lo, (uint32_t)hi};
}

// The optional trailing kernel argument of the fp8-KV instantiations (a parameter pack that is
// empty for bf16, so the bf16 kernels keep their argument list).
__device__ __forceinline__ const float* pack_ptr(const float* p) { return p; }
// The sliding-window instantiations of the attention kernels put their window (tokens, > 0) in
// front of it, so the pack is (), (kv_scale), (window) or (window, kv_scale) and the unwindowed
// kernels keep their argument lists too.
__device__ __forceinline__ const float* pack_ptr(int, const float* p) { return p; }
__device__ __forceinline__ int pack_window(int w) { return w; }
__device__ __forceinline__ int pack_window(int w, const float*) { return w; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

}  // namespace dgi

#define DGI_CHECK_LAUNCH() \
  do { hipError_t e__ = hipGetLastError(); if (e__ != hipSuccess) return (int)e__; } while (0)
