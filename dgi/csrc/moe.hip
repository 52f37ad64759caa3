// dgi/csrc/moe.hip — mixture-of-experts MLP: router, expert-sorted layout, grouped GEMM, combine.
//
// A Qwen3-MoE layer sends every token to k of E SwiGLU experts.  Four kernels, all fixed-grid
// functions of (T, k, E), no host read-back and no atomics, so the block is hipGraph-capturable
// and bit-reproducible:
//
//  * moe_route    one wave per token: E/64 logits per lane, k rounds of wave argmax on the
//                 LOGITS (two distinct logits can round to one fp32 probability), ties to the
//                 lower expert; weights exp(l - max) / sum in fp32.
//  * moe_align    the expert-sorted layout of the T*k slots (slot = t*k + j): workgroup e counts
//                 its slots (first launch), then places them in ascending slot order by ballot /
//                 popcount prefixes (second launch).  Every expert's rows are padded to the GEMM's
//                 row block BM; padding rows carry slot -1, unused row blocks expert -1.
//  * moe_gemm     Y[row block b] = X[rows of b] · W[block_expert[b]]^T on the weight-streaming
//                 core of stream_gemm.h.  The SwiGLU epilogue gathers its A rows through
//                 sorted_slot / k and owns the same column range of gate and of up; the plain
//                 epilogue reads act in sorted order.  At large T an
//                 expert's weights are read once per row block (an LDS-tiled prefill kernel is
//                 future work).
//  * moe_gemm_w8  the same kernel over FP8 weight-only experts (opt-in, expert_quant="fp8"): OCP
//                 e4m3 codes [E, N or 2N, K] with one fp32 scale per expert and output channel,
//                 widened in registers (E4m3W, 128-deep K steps).  The epilogue multiplies the fp32
//                 sum by scale[e, col] (gate and up each by their own) before SwiGLU and the one
//                 rounding.  4 waves split K when K % 512 == 0, else 2: a function of K alone, so
//                 a row's bits do not depend on the row block.
//  * moe_combine  out[t] = bf16(sum_j weights[t, j] * y[inv[t*k + j]]): fp32, j order, no FMA
//                 contraction (the torch reference multiplies, rounds, adds), one final rounding.
#include <limits.h>
#include <math.h>
#include <type_traits>

#include "stream_gemm.h"

using namespace dgi;

namespace {

constexpr int kMaxExperts = 256;
constexpr int kMaxTopK = 16;

// ---------------------------------------------------------------- route
__global__ __launch_bounds__(256) void moe_route_kernel(const void* __restrict__ logits, int is_bf16, int ld, int T,
                                                        int E, int k, int norm, int* __restrict__ ids,
                                                        float* __restrict__ weights) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;  // wave-uniform
  float v[4];
  float m = -INFINITY;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int e = s * 64 + lane;
    float x = -INFINITY;
    if (e < E) {
      x = is_bf16 ? bf16_to_f32(((const uint16_t*)logits)[(size_t)t * ld + e])
                  : ((const float*)logits)[(size_t)t * ld + e];
      if (!(x == x)) x = -INFINITY;  // a NaN logit is never chosen
    }
    v[s] = x;
    m = fmaxf(m, x);
  }
  m = wave_max(m);
  float tot = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (s * 64 + lane < E) tot += expf(v[s] - m);
  tot = wave_sum(tot);
  unsigned taken = 0;
  float myv = 0.f;
  int myid = 0;
  for (int j = 0; j < k; ++j) {
    // this lane's best remaining expert: ascending index, strictly greater replaces
    float bv = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int e = s * 64 + lane;
      if (e < E && !((taken >> s) & 1u) && (bi == INT_MAX || v[s] > bv)) {
        bv = v[s];
        bi = e;
      }
    }
    // wave argmax under the total order (value descending, index ascending): every lane ends equal
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != INT_MAX && (bi == INT_MAX || ov > bv || (ov == bv && oi < bi))) {
        bv = ov;
        bi = oi;
      }
    }
    if (bi != INT_MAX && (bi & 63) == lane) taken |= 1u << (bi >> 6);
    if (lane == j) {
      myv = bv;
      myid = bi;
    }
  }
  const float p = lane < k ? expf(myv - m) : 0.f;
  const float chosen = wave_sum(p);
  const float den = norm ? chosen : tot;
  if (lane < k) {
    ids[(size_t)t * k + lane] = myid;
    weights[(size_t)t * k + lane] = p / den;
  }
}

// ---------------------------------------------------------------- align
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the workgroup (nw waves); sm holds nw ints
__device__ __forceinline__ int block_sum_i(int v, int* sm, int nw) {
  v = wave_sum_i(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = 0;
  for (int i = 0; i < nw; ++i) r += sm[i];
  return r;
}

__global__ __launch_bounds__(256) void moe_count_kernel(const int* __restrict__ ids, int n, int* __restrict__ counts) {
  __shared__ int sm[4];
  const int e = blockIdx.x;
  int c = 0;
  for (int i = threadIdx.x; i < n; i += 256) c += ids[i] == e;
  c = block_sum_i(c, sm, 4);
  if (threadIdx.x == 0) counts[e] = c;
}

constexpr int kAlignThreads = 1024;

__global__ __launch_bounds__(kAlignThreads) void moe_place_kernel(
    const int* __restrict__ ids, int n, int E, int BM, int P, const int* __restrict__ counts,
    int* __restrict__ offsets, int* __restrict__ sorted_slot, int* __restrict__ block_expert, int* __restrict__ inv) {
  constexpr int NWV = kAlignThreads / 64;
  __shared__ int sm[NWV];
  const int e = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  // padded counts: this expert's first row and the end of the used rows
  int pc = 0;
  if (tid < E) pc = (counts[tid] + BM - 1) / BM * BM;
  const int off = block_sum_i(tid < e ? pc : 0, sm, NWV);
  const int total = block_sum_i(pc, sm, NWV);
  const int mine = counts[e];
  const int mine_pad = (mine + BM - 1) / BM * BM;
  if (total > P || off + mine_pad > P) return;  // cannot happen for the P the host computes; never write past it
  // stable placement: 1024 slots per round, position = matches before this slot
  int running = 0;
  for (int base = 0; base < n; base += kAlignThreads) {
    const int i = base + tid;
    const int id = i < n ? ids[i] : -1;
    const bool hit = id == e;
    const unsigned long long b = __ballot(hit);
    __syncthreads();
    if (lane == 0) sm[w] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int j = 0; j < NWV; ++j) {
      const int c = sm[j];
      before += j < w ? c : 0;
      all += c;
    }
    if (hit) {
      const int pos = off + running + before + __popcll(b & ((1ull << lane) - 1ull));
      if (pos < off + mine_pad) {
        sorted_slot[pos] = i;
        inv[i] = pos;
      }
    } else if (e == 0 && i < n && (id < 0 || id >= E)) {
      inv[i] = -1;  // an id no expert owns: its slot contributes nothing
    }
    running += all;
  }
  for (int i = mine + tid; i < mine_pad; i += kAlignThreads) sorted_slot[off + i] = -1;
  for (int b = tid; b < mine_pad / BM; b += kAlignThreads) block_expert[off / BM + b] = e;
  // the unused tail, shared between the workgroups
  for (int i = total + e * kAlignThreads + tid; i < P; i += E * kAlignThreads) sorted_slot[i] = -1;
  for (int b = total / BM + e * kAlignThreads + tid; b < P / BM; b += E * kAlignThreads) block_expert[b] = -1;
  if (tid == 0) {
    offsets[e] = off;
    if (e == 0) offsets[E] = total;
  }
}

// ---------------------------------------------------------------- grouped GEMM
__device__ __forceinline__ float silu(float g) { return g / (1.f + expf(-g)); }

// stream_gemm.h's core over the weights of format F, one K step per group: 64 deep for bf16
// (Bf16W), 128 deep for e4m3 codes (E4m3W, widened in registers as skinny_gemm_fp8.hip does).
// Row block blockIdx.y multiplies the 16·MT sorted rows p0.. by expert block_expert[blockIdx.y].
// SWIGLU: W is [E, 2N, K] and the block multiplies rows n0.. of gate and N + n0.. of up.
// E4m3W: scale [E, N or 2N] fp32, one per expert and output channel; the fp32 tile sum is
// multiplied by it (gate and up each by their own row's) before the epilogue's one rounding.
template <class F, int NW, int MT, int NT, int D, bool SWIGLU>
__global__ __launch_bounds__(NW * 64) void moe_gemm_kernel(
    const uint16_t* __restrict__ X, int ldx, typename F::Mat W, const float* __restrict__ scale,
    const int* __restrict__ sorted_slot, const int* __restrict__ block_expert, uint16_t* __restrict__ Y, int ldy,
    int N, int K, int kdiv, int nslots, int E) {
  constexpr int WT = SWIGLU ? 2 * NT : NT;
  constexpr bool SCALED = !std::is_same<F, Bf16W>::value;
  const int e = block_expert[blockIdx.y];
  if (e < 0 || e >= E) return;  // unused row block (workgroup-uniform)
  const int n0 = blockIdx.x * 16 * NT;
  const int p0 = blockIdx.y * 16 * MT;
  const size_t wrows = SWIGLU ? 2 * (size_t)N : (size_t)N;
  stream_gemm<F, NW, MT, WT, NT, 1, D>(
      X, ldx, K,  // host: K % (F::kStep * NW) == 0
      [&](int m) {
        const int slot = sorted_slot[p0 + m];
        if (slot < 0 || slot >= nslots) return -1;  // padding rows read nothing
        // SwiGLU gathers the token's row; the plain epilogue reads act in sorted order
        return kdiv > 0 ? slot / kdiv : p0 + m;
      },
      [&](int t, int r, int g, int w) {
        return F::ptr(W, (size_t)e * wrows + ((t < NT ? 0 : N) + n0 + (t % NT) * 16 + r), K, g, w);
      },
      [&](int mt, int nt, int r, int g, auto tile) {
        f32x4 a = tile(nt);
        f32x4 u = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (SWIGLU) u = tile(NT + nt);
        const int col = n0 + nt * 16 + r;
        if constexpr (SCALED) {
          const float sa = scale[(size_t)e * wrows + col];
          const float su = SWIGLU ? scale[(size_t)e * wrows + N + col] : 0.f;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            a[i] *= sa;
            u[i] *= su;
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int p = p0 + mt * 16 + g * 4 + i;
          const int slot = sorted_slot[p];
          if (slot >= 0 && slot < nslots) {  // padding rows write nothing
            const float val = SWIGLU ? silu(a[i]) * u[i] : a[i];
            Y[(size_t)p * ldy + col] = f32_to_bf16(val);
          }
        }
      });
}

template <int MT, bool SWIGLU>
int launch_gemm(const void* x, int ldx, const void* w, const int* sorted_slot, const int* block_expert, void* y,
                int ldy, int P, int N, int K, int kdiv, int nslots, int E, hipStream_t s) {
  constexpr int NW = 4, NT = 1;
  constexpr int D = MT == 1 ? 4 : 2;
  const dim3 grid(N / (16 * NT), P / (16 * MT));
  moe_gemm_kernel<Bf16W, NW, MT, NT, D, SWIGLU><<<grid, NW * 64, 0, s>>>(
      (const uint16_t*)x, ldx, (const uint16_t*)w, nullptr, sorted_slot, block_expert, (uint16_t*)y, ldy, N, K, kdiv,
      nslots, E);
  DGI_CHECK_LAUNCH();
  return 0;
}

// e4m3 experts: NW waves split K's 128-deep steps, so NW is a function of K alone (the core's
// results depend on NW, not on MT or D: a row's bits must not change with the row block).
template <int NW, int MT, bool SWIGLU>
int launch_gemm_w8(const void* x, int ldx, const void* q, const float* scale, const int* sorted_slot,
                   const int* block_expert, void* y, int ldy, int P, int N, int K, int kdiv, int nslots, int E,
                   hipStream_t s) {
  constexpr int NT = 1;
  // a double buffer at both row blocks: the deeper ring of the bf16 kernel's MT = 1 was 5-7 % slower
  // here at T = 4 .. 64 (profiles/moe_fp8/README.md)
  constexpr int D = 2;
  const dim3 grid(N / (16 * NT), P / (16 * MT));
  moe_gemm_kernel<E4m3W, NW, MT, NT, D, SWIGLU><<<grid, NW * 64, 0, s>>>(
      (const uint16_t*)x, ldx, (const uint8_t*)q, scale, sorted_slot, block_expert, (uint16_t*)y, ldy, N, K, kdiv,
      nslots, E);
  DGI_CHECK_LAUNCH();
  return 0;
}

template <int NW>
int dispatch_gemm_w8(const void* x, int ldx, const void* q, const float* scale, const int* sorted_slot,
                     const int* block_expert, void* y, int ldy, int P, int N, int K, int kdiv, int nslots, int E,
                     int BM, int epi, hipStream_t s) {
#define DGI_MOE_W8(MT, SW) \
  launch_gemm_w8<NW, MT, SW>(x, ldx, q, scale, sorted_slot, block_expert, y, ldy, P, N, K, kdiv, nslots, E, s)
  if (BM == 16) return epi ? DGI_MOE_W8(1, true) : DGI_MOE_W8(1, false);
  return epi ? DGI_MOE_W8(2, true) : DGI_MOE_W8(2, false);
#undef DGI_MOE_W8
}

// ---------------------------------------------------------------- combine
__global__ __launch_bounds__(256) void moe_combine_kernel(const uint16_t* __restrict__ y, int ldy,
                                                          const int* __restrict__ inv,
                                                          const float* __restrict__ weights,
                                                          uint16_t* __restrict__ out, int k, int H, int P) {
  const int t = blockIdx.x;
  for (int c = threadIdx.x * 8; c < H; c += 256 * 8) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < k; ++j) {
      const int row = inv[(size_t)t * k + j];
      if (row < 0 || row >= P) continue;
      const float wt = weights[(size_t)t * k + j];
      float f[8];
      unpack8(*reinterpret_cast<const u32x4*>(y + (size_t)row * ldy + c), f);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = __fadd_rn(acc[i], __fmul_rn(wt, f[i]));
    }
    *reinterpret_cast<u32x4*>(out + (size_t)t * H + c) = pack8(acc);
  }
}

}  // namespace

// logits [T, E] (row stride ld) bf16 or fp32 -> ids [T, k] int32, weights [T, k] fp32
extern "C" int dgi_moe_route(const void* logits, int is_bf16, int ld, int T, int E, int k, int norm, int* ids,
                             float* weights, hipStream_t s) {
  if (T <= 0) return 0;
  if (E < 1 || E > kMaxExperts || k < 1 || k > kMaxTopK || k > E || ld < E) return -3;
  moe_route_kernel<<<(T + 3) / 4, 256, 0, s>>>(logits, is_bf16, ld, T, E, k, norm, ids, weights);
  DGI_CHECK_LAUNCH();
  return 0;
}

// rows of the sorted layout for n slots over E experts and row blocks of BM
extern "C" int dgi_moe_capacity(int n, int E, int BM) {
  return BM * ((n + BM - 1) / BM + (E < n ? E : n));
}

// ids [n] -> counts [E], offsets [E + 1], sorted_slot [P], block_expert [P / BM], inv [n]
extern "C" int dgi_moe_align(const int* ids, int n, int E, int BM, int P, int* counts, int* offsets,
                             int* sorted_slot, int* block_expert, int* inv, hipStream_t s) {
  if (E < 1 || E > kMaxExperts || (BM != 16 && BM != 32) || n < 1) return -3;
  if (P != dgi_moe_capacity(n, E, BM)) return -2;
  moe_count_kernel<<<E, 256, 0, s>>>(ids, n, counts);
  DGI_CHECK_LAUNCH();
  moe_place_kernel<<<E, kAlignThreads, 0, s>>>(ids, n, E, BM, P, counts, offsets, sorted_slot, block_expert, inv);
  DGI_CHECK_LAUNCH();
  return 0;
}

// epi 0: y [P, N] = x[sorted rows] · w[e]^T, w [E, N, K] (kdiv 0: x is in sorted order)
// epi 1: y [P, N] = silu(x · gate^T) * (x · up^T), w [E, 2N, K] = [gate; up] (kdiv = k: x rows are tokens)
extern "C" int dgi_moe_gemm(const void* x, int ldx, const void* w, const int* sorted_slot, const int* block_expert,
                            void* y, int ldy, int P, int N, int K, int kdiv, int nslots, int E, int BM, int epi,
                            hipStream_t s) {
  if (P <= 0 || N <= 0) return 0;
  if (K % 256 || N % 16 || ldx % 8 || K <= 0) return -3;
  if ((BM != 16 && BM != 32) || P % BM || E < 1 || E > kMaxExperts || kdiv < 0 || (epi != 0 && epi != 1)) return -3;
  if (P / 16 > 65535) return -2;
  if (BM == 16)
    return epi ? launch_gemm<1, true>(x, ldx, w, sorted_slot, block_expert, y, ldy, P, N, K, kdiv, nslots, E, s)
               : launch_gemm<1, false>(x, ldx, w, sorted_slot, block_expert, y, ldy, P, N, K, kdiv, nslots, E, s);
  return epi ? launch_gemm<2, true>(x, ldx, w, sorted_slot, block_expert, y, ldy, P, N, K, kdiv, nslots, E, s)
             : launch_gemm<2, false>(x, ldx, w, sorted_slot, block_expert, y, ldy, P, N, K, kdiv, nslots, E, s);
}

// dgi_moe_gemm over e4m3 experts: q [E, N or 2N, K] OCP e4m3 codes, scale [E, N or 2N] fp32; the
// result is bf16((x · q[e]^T) * scale[e]) (SwiGLU: gate and up scaled before silu(g) * u).
// 4 waves when K % 512 == 0, else 2 (K = 768 is six 128-deep steps).
extern "C" int dgi_moe_gemm_w8(const void* x, int ldx, const void* q, const float* scale, const int* sorted_slot,
                               const int* block_expert, void* y, int ldy, int P, int N, int K, int kdiv, int nslots,
                               int E, int BM, int epi, hipStream_t s) {
  if (P <= 0 || N <= 0) return 0;
  if (K % 256 || N % 16 || ldx % 8 || K <= 0) return -3;
  if ((BM != 16 && BM != 32) || P % BM || E < 1 || E > kMaxExperts || kdiv < 0 || (epi != 0 && epi != 1)) return -3;
  if (P / 16 > 65535) return -2;
  if (K % 512 == 0)
    return dispatch_gemm_w8<4>(x, ldx, q, scale, sorted_slot, block_expert, y, ldy, P, N, K, kdiv, nslots, E, BM, epi,
                               s);
  return dispatch_gemm_w8<2>(x, ldx, q, scale, sorted_slot, block_expert, y, ldy, P, N, K, kdiv, nslots, E, BM, epi, s);
}

// out [T, H] = bf16(sum_j weights[t, j] * y[inv[t*k + j]])
extern "C" int dgi_moe_combine(const void* y, int ldy, const int* inv, const float* weights, void* out, int T, int k,
                               int H, int P, hipStream_t s) {
  if (T <= 0) return 0;
  if (H % 8 || ldy % 8 || k < 1 || k > kMaxTopK) return -3;
  moe_combine_kernel<<<T, 256, 0, s>>>((const uint16_t*)y, ldy, inv, weights, (uint16_t*)out, k, H, P);
  DGI_CHECK_LAUNCH();
  return 0;
}
