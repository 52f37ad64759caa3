// dgi/csrc/qknorm_rope_cache.hip — per-head q/k RMSNorm + RoPE(q,k) + paged KV-cache write (Qwen3).
//
// rope_cache.hip with one addition: every q head and every k head of a token is RMS-normalised
// over its head_dim with a learned [head_dim] gain (q_gain for q heads, k_gain for k heads)
// before it is rotated:
//   n[d] = bf16(float(x[d]) * rsqrt(mean_d(float(x)^2) + eps) * float(gain[d]))     (ops.rmsnorm_ref)
//   then RoPE on float(n) as rope_cache does, bf16, and for e4m3 pages the quantiser of common.h.
// q is rewritten in place, k and v go to the paged cache at slot_mapping[t] (slot < 0: nothing is
// written), v is copied untouched.  Scope: NeoX pairing over the whole head (rd == hd), hd 64 or 128.
//
// One workgroup per token.  hd/8 lanes own a head, each holding one 16-byte chunk in registers:
// the sum of squares is reduced over those lanes by shuffles, and the rotation partner chunk
// (d, d + hd/2) comes from lane ^ (hd/16) by shuffle — no LDS and no second read of the row.
// A 256-thread block covers 256 / (hd/8) heads per pass.
#include "common.h"

using namespace dgi;

// No multiply-add contraction anywhere below: the bf16 and the e4m3 instantiation then do the same
// arithmetic, and the e4m3 pages are exactly the quantiser applied to what the bf16 one stores.
#pragma clang fp contract(off)

template <int HD, bool FP8, typename... S>
__global__ __launch_bounds__(256) void qknorm_rope_cache_kernel(
    uint16_t* __restrict__ qkv, int qkv_stride, const int* __restrict__ positions,
    const float* __restrict__ cos_sin, const uint16_t* __restrict__ q_gain,
    const uint16_t* __restrict__ k_gain, float eps, int nh, int nkv,
    const int* __restrict__ slot_mapping, uint16_t* __restrict__ k_cache,
    uint16_t* __restrict__ v_cache, int block_size, S... kv_inv_scale) {
  constexpr int L = HD / 8;        // lanes per head (a power of two that divides the wave)
  constexpr int HPP = 256 / L;     // heads per pass of the block
  constexpr int HALF = L / 2;      // lane distance of the rotation partner
  const int t = blockIdx.x;
  const int pos = positions[t];
  uint16_t* row = qkv + (size_t)t * qkv_stride;
  const float* cs = cos_sin + (size_t)pos * HD;
  const int slot = slot_mapping ? slot_mapping[t] : -1;
  const int blk = slot >= 0 ? slot / block_size : 0;
  const int off = slot >= 0 ? slot - blk * block_size : 0;
  [[maybe_unused]] const float* inv_scale = nullptr;
  if constexpr (FP8) inv_scale = pack_ptr(kv_inv_scale...);

  const int c = threadIdx.x & (L - 1);     // this lane's chunk of the head: dims [8c, 8c + 8)
  const int hsub = threadIdx.x / L;
  const bool lo = c < HALF;                // first half of the head: out = x cos - partner sin
  // the frequencies of dims 8c..8c+7 and of their partners are the same: (8c mod hd/2) + j
  float cv[8], sv[8];
  {
    const float4* cp = reinterpret_cast<const float4*>(cs + (c & (HALF - 1)) * 8);
    const float4* sp = reinterpret_cast<const float4*>(cs + HD / 2 + (c & (HALF - 1)) * 8);
    *reinterpret_cast<float4*>(cv) = cp[0];
    *reinterpret_cast<float4*>(cv + 4) = cp[1];
    *reinterpret_cast<float4*>(sv) = sp[0];
    *reinterpret_cast<float4*>(sv + 4) = sp[1];
  }

  const int heads = nh + nkv;
  // the trip count is the same for every lane: lanes past the last head take part in the
  // shuffles with zeros and skip only the store
  for (int base = 0; base < heads; base += HPP) {
    const int head = base + hsub;
    const bool live = head < heads;
    u32x4* p = reinterpret_cast<u32x4*>(row + (size_t)head * HD + c * 8);   // q heads then k heads
    u32x4 raw = {0u, 0u, 0u, 0u}, graw = {0u, 0u, 0u, 0u};
    if (live) {
      raw = *p;
      graw = *reinterpret_cast<const u32x4*>((head < nh ? q_gain : k_gain) + c * 8);
    }
    float x[8], g[8];
    unpack8(raw, x);
    unpack8(graw, g);
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += x[j] * x[j];
#pragma unroll
    for (int o = HALF; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    // 1 / sqrt, both correctly rounded, as the reference's rsqrt: where the sum of squares is exact
    // the normalised head equals the reference's bit for bit
    const float r = 1.f / sqrtf(ss * (1.f / HD) + eps);
    float n[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) n[j] = (x[j] * r) * g[j];
    const u32x4 nb = pack8(n);             // the normalised head as bf16, as rmsnorm_ref returns it
    u32x4 pb;
#pragma unroll
    for (int i = 0; i < 4; ++i) pb[i] = (uint32_t)__shfl_xor((int)nb[i], HALF, 64);
    float a[8], b[8], o[8];
    unpack8(nb, a);
    unpack8(pb, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float ac = a[j] * cv[j], bs = b[j] * sv[j];
      o[j] = lo ? ac - bs : ac + bs;
    }
    const u32x4 res = pack8(o);
    if (!live) continue;
    if (head < nh) {
      *p = res;
    } else if (slot >= 0) {
      const int kh = head - nh;
      const size_t e = (((size_t)blk * nkv + kh) * block_size + off) * HD + c * 8;
      if constexpr (FP8) {
        float f[8];
        unpack8(res, f);
        *reinterpret_cast<uint2*>(reinterpret_cast<uint8_t*>(k_cache) + e) = quant8_e4m3(f, inv_scale[kh]);
      } else {
        *reinterpret_cast<u32x4*>(k_cache + e) = res;
      }
    }
  }

  if (slot < 0) return;
  for (int it = threadIdx.x; it < nkv * L; it += 256) {
    const int vh = it / L;
    const int vc = it - vh * L;
    const u32x4 v = *reinterpret_cast<const u32x4*>(row + (size_t)(heads + vh) * HD + vc * 8);
    const size_t e = (((size_t)blk * nkv + vh) * block_size + off) * HD + vc * 8;
    if constexpr (FP8) {
      float f[8];
      unpack8(v, f);
      *reinterpret_cast<uint2*>(reinterpret_cast<uint8_t*>(v_cache) + e) = quant8_e4m3(f, inv_scale[nkv + vh]);
    } else {
      *reinterpret_cast<u32x4*>(v_cache + e) = v;
    }
  }
}

template <int HD>
static int launch_qknorm(void* qkv, int T, int qkv_stride, const int* positions, const float* cos_sin,
                         const void* q_gain, const void* k_gain, float eps, int nh, int nkv,
                         const int* slot_mapping, void* k_cache, void* v_cache, int block_size,
                         const float* kv_inv_scale, hipStream_t s) {
  // kv_inv_scale != nullptr: the caches hold e4m3 codes
  if (kv_inv_scale) {
    qknorm_rope_cache_kernel<HD, true, const float*><<<T, 256, 0, s>>>(
        (uint16_t*)qkv, qkv_stride, positions, cos_sin, (const uint16_t*)q_gain, (const uint16_t*)k_gain, eps,
        nh, nkv, slot_mapping, (uint16_t*)k_cache, (uint16_t*)v_cache, block_size, kv_inv_scale);
  } else {
    qknorm_rope_cache_kernel<HD, false><<<T, 256, 0, s>>>(
        (uint16_t*)qkv, qkv_stride, positions, cos_sin, (const uint16_t*)q_gain, (const uint16_t*)k_gain, eps,
        nh, nkv, slot_mapping, (uint16_t*)k_cache, (uint16_t*)v_cache, block_size);
  }
  DGI_CHECK_LAUNCH();
  return 0;
}

// cos_sin rows are [hd/2 cos | hd/2 sin] (rd == hd, NeoX pairing); q_gain / k_gain are bf16 [hd].
extern "C" int dgi_qknorm_rope_cache(void* qkv, int T, int qkv_stride, const int* positions,
                                     const float* cos_sin, const void* q_gain, const void* k_gain, float eps,
                                     int nh, int nkv, int hd, const int* slot_mapping, void* k_cache,
                                     void* v_cache, int block_size, const float* kv_inv_scale, hipStream_t s) {
  if (hd != 64 && hd != 128) return -2;
  if (qkv_stride % 8 || nh <= 0 || nkv <= 0 || block_size <= 0) return -3;
  if (T == 0) return 0;
  return hd == 128 ? launch_qknorm<128>(qkv, T, qkv_stride, positions, cos_sin, q_gain, k_gain, eps, nh, nkv,
                                        slot_mapping, k_cache, v_cache, block_size, kv_inv_scale, s)
                   : launch_qknorm<64>(qkv, T, qkv_stride, positions, cos_sin, q_gain, k_gain, eps, nh, nkv,
                                       slot_mapping, k_cache, v_cache, block_size, kv_inv_scale, s);
}
