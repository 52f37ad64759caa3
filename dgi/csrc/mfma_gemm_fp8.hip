// dgi/csrc/mfma_gemm_fp8.hip — FP8 W8A8 projections for prefill-sized steps:
// the dynamic per-token activation quantiser and an e4m3 x e4m3 MFMA GEMM.
//
//   quant_rows_fp8:  x [M, K] bf16 (row stride ldx)  ->  q [M, K] e4m3, sx [M] fp32
//       amax = max|x[m]|, sx = amax / 448 and inv = 448 / amax (both 1 for a zero row),
//       q = rne_e4m3(clamp(x * inv, -448, 448)); fp32 arithmetic, IEEE divisions.
//   mfma_gemm_fp8:   Y[M, N] = (Xq[M, K] · Wq[N, K]^T) * sx[m] * sw[n] (+ bias[n])
//       e4m3 operands, fp32 scales, bf16 bias and Y, fp32 accumulation.
//
// The GEMM is the simple kernel of mfma_gemm.hip (mfma_gemm_kernel<0, 1>) with one-byte
// operands: an e4m3 row of 128 k is the 128 bytes of that kernel's 64-k bf16 row, so the 256 x 256
// tile, the 512 threads, the two LDS stages of 2 x 32 KB, the 16-byte global_load_lds with the
// source-side chunk swizzle c ^ ((r >> 1) & 7), the XCD-aware tile order and the clamped row tail
// are the same byte for byte.  What differs:
//
//  * K step 128: one v_mfma_scale_f32_16x16x128_f8f6f4 per 16x16 block and K tile (both formats
//    e4m3, every block scale the E8M0 byte 127 = 2^0) — the only FP8 MFMA with twice the bf16 rate.
//  * Fragment: a lane's 32 bytes are 16-byte chunks g and g + 4 of its row (g = lane >> 4), the
//    two chunks the bf16 kernel reads as its k halves, so the conflict-free ds_read_b128 pattern
//    carries over.  X and W fragments follow the same rule and all scales are 1, so every k of
//    the tile meets its partner exactly once whatever the instruction's internal k order is.
//  * Registers: a full fragment set is 4 x 8 (W) + 8 x 8 (X) = 96 dwords next to 128 accumulator
//    dwords, so a second set does not fit at two waves per SIMD.  The wave tile runs as two
//    64-row halves of X: the second half's X reads ride the first half's MFMAs, and the next
//    tile's first-half X reads, W reads and staging loads ride the second half's.
//  * Epilogue: acc * sx[m] * sw[n] (+ bias[n]), packed to bf16, 16-byte stores.
//
// Requirements (checked by the host): N % 256 == 0, K % 128 == 0, ldy % 4 == 0, contiguous Xq
// and Wq.  Any M >= 1.  The quantiser takes K % 16 == 0, ldx % 8 == 0 and any M.
// Non-finite activations are outside the contract: the quantiser's fmaxf drops a NaN from amax
// (the torch reference propagates it to the whole row), and an Inf gives inv = 0 and NaN codes.
#include "common.h"

#include <type_traits>

using namespace dgi;

namespace {

constexpr int kBM = 256;
constexpr int kBK = 128;                       // e4m3 elements = bytes per tile row
constexpr int kTileBytes = kBM * kBK;          // 32 KB: one operand, one stage
constexpr int kStageBytes = 2 * kTileBytes;    // X tile + W tile

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void gbl_void_t;

__device__ __forceinline__ void glds16(const uint8_t* src, char* lds) {
  __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)lds, 16, 0, 0);
}

// ---------------------------------------------------------------------------
// Row quantiser.  WPR waves share a row (1: four rows per 256-thread block, 4: one); a lane
// takes 16 elements per pass (two 16-byte loads, one 16-byte store).  The row is read twice,
// the second time from cache.
template <int WPR>
__global__ __launch_bounds__(256) void quant_rows_fp8_kernel(const uint16_t* __restrict__ X, int ldx,
                                                             uint8_t* __restrict__ Q, float* __restrict__ SX,
                                                             int M, int K) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int t = WPR == 1 ? lane : threadIdx.x;
  const int m = WPR == 1 ? blockIdx.x * 4 + wave : blockIdx.x;
  if (m >= M) return;               // WPR 1 only (whole waves; that kernel has no barrier)
  const uint16_t* x = X + (size_t)m * ldx;
  uint8_t* q = Q + (size_t)m * K;

  float amax = 0.f;
  for (int k = t * 16; k < K; k += WPR * 64 * 16) {
    const u32x4 v0 = *(const u32x4*)(x + k), v1 = *(const u32x4*)(x + k + 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // |bf16| as fp32 bit patterns
      amax = fmaxf(amax, __uint_as_float((v0[e] << 16) & 0x7fffffffu));
      amax = fmaxf(amax, __uint_as_float(v0[e] & 0x7fff0000u));
      amax = fmaxf(amax, __uint_as_float((v1[e] << 16) & 0x7fffffffu));
      amax = fmaxf(amax, __uint_as_float(v1[e] & 0x7fff0000u));
    }
  }
  amax = wave_max(amax);
  if (WPR > 1) {
    if (lane == 0) red[wave] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  }
  const float sx = amax > 0.f ? __fdiv_rn(amax, 448.f) : 1.f;
  const float inv = amax > 0.f ? __fdiv_rn(448.f, amax) : 1.f;
  if (t == 0) SX[m] = sx;

  for (int k = t * 16; k < K; k += WPR * 64 * 16) {
    const u32x4 v0 = *(const u32x4*)(x + k), v1 = *(const u32x4*)(x + k + 8);
    float f[16];
    unpack8(v0, f);
    unpack8(v1, f + 8);
    const uint2 lo = quant8_e4m3(f, inv), hi = quant8_e4m3(f + 8, inv);
    *(uint4*)(q + k) = uint4{lo.x, lo.y, hi.x, hi.y};
  }
}

// ---------------------------------------------------------------------------
// The GEMM (see the file header).  Wave w owns rows 128 (w >> 2) .. + 127 and columns
// 64 (w & 3) .. + 63 of the tile: acc[i][j] is the 16x16 block of rows 16 i, columns 16 j, with W as
// the A operand and X as the B operand, so a lane holds 4 consecutive columns of one row.
__global__ __launch_bounds__(512) void mfma_gemm_fp8_kernel(const uint8_t* __restrict__ X,
                                                             const float* __restrict__ SX,
                                                             const uint8_t* __restrict__ W,
                                                             const float* __restrict__ SW,
                                                             const uint16_t* __restrict__ bias,
                                                             uint16_t* __restrict__ Y, int ldy, int M, int K,
                                                             int tiles_m, int tiles_total) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kStageBytes];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int wm = w >> 2, wn = w & 3;

  // XCD-aware, bijective block -> tile map (blocks b and b + 8 share an XCD)
  const int b = blockIdx.x;
  const int xcd = b & 7, li = b >> 3;
  const int q8 = tiles_total >> 3, r8 = tiles_total & 7;
  const int t = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + li;
  const int tm = t % tiles_m, tn = t / tiles_m;
  const int m0 = tm * kBM;

  // ---- staging map: lane-linear LDS image, swizzled global source
  const int q = tid >> 3;                         // row within each 64-row slab
  const int lc = (tid & 7) ^ ((tid >> 4) & 7);    // logical k-chunk this lane fetches
  // 32-bit lane offsets from the block-uniform bases X + k0 and W + tile row + k0 (the host
  // checks that both operands are below 2 GB)
  unsigned xoff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) xoff[i] = (unsigned)min(m0 + q + i * 64, M - 1) * (unsigned)K + lc * 16;
  const unsigned woff = (unsigned)q * (unsigned)K + lc * 16;
  const uint8_t* const wtile = W + (size_t)tn * 256 * K;
  const size_t wslab = (size_t)64 * K;
  char* const lds_x = smem + w * 1024;               // + stage * kStageBytes + i * 8 KB
  char* const lds_w = smem + kTileBytes + w * 1024;

  auto issue = [&](int kt, int stage) {
    const uint8_t* const xk = X + kt * kBK;
    const uint8_t* const wk = wtile + kt * kBK;
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(xk + xoff[i], lds_x + stage * kStageBytes + i * 8192);
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(wk + i * wslab + woff, lds_w + stage * kStageBytes + i * 8192);
  };

  // ---- fragment read map (bytes inside one operand tile): chunks g and g + 4 of the lane's row
  const int r16 = lane & 15;
  const int g = lane >> 4;
  const int sw = (lane >> 1) & 7;
  const int ph0 = (g ^ sw) * 16;
  const int ph1 = ((4 + g) ^ sw) * 16;
  const int xbase = (wm * 128 + r16) * 128;
  const int wbase = kTileBytes + (wn * 64 + r16) * 128;

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto frag = [&](const char* row) {
    const u32x4 lo = *(const u32x4*)(row + ph0), hi = *(const u32x4*)(row + ph1);
    return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
  };
  // X rows 64 half .. + 63 of the wave tile
  auto read_x = [&](int stage, int half, i32x8* xf) {
    const char* s = smem + stage * kStageBytes + xbase + half * 8192;
#pragma unroll
    for (int i = 0; i < 4; ++i) xf[i] = frag(s + i * 2048);
  };
  auto read_w = [&](int stage, i32x8* wf) {
    const char* s = smem + stage * kStageBytes + wbase;
#pragma unroll
    for (int j = 0; j < 4; ++j) wf[j] = frag(s + j * 2048);
  };
  // column-block-major: W fragment j is dead after its 4 MFMAs
  auto mma = [&](int half, const i32x8* xf, const i32x8* wf) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[half * 4 + i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[j], xf[i], acc[half * 4 + i][j], 0,
                                                                                0, 0, 127, 0, 127);
  };

  i32x8 xa[4], xb[4], wf[4];
  const int nt = K / kBK;
  issue(0, 0);
  if (nt > 1) issue(1, 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  read_w(0, wf);
  read_x(0, 0, xa);

  // One K tile: [second-half X reads | first-half MFMAs], barrier, [next tile's staging loads,
  // first-half X reads and W reads | second-half MFMAs], the memory instructions spread between
  // the MFMAs (sched_group_barrier).  The next W fragment j is read into the registers of the
  // current one once its last MFMA has issued (mma runs column-block-major), so W needs no second
  // register set.  The loop is peeled so each body is one scheduling region.
  auto body = [&](int kt, auto issue_next, auto read_next) {
    const int st = kt & 1;
    read_x(st, 1, xb);
    mma(0, xa, wf);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    // next stage landed: hipcc does not count global_load_lds as an LDS write before a
    // barrier, so the wave's own loads are retired explicitly
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();          // every wave's loads landed; every wave done reading this stage
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (decltype(issue_next)::value) issue(kt + 2, st);
    if constexpr (decltype(read_next)::value) read_x(st ^ 1, 0, xa);
    mma(1, xb, wf);
    if constexpr (decltype(read_next)::value) read_w(st ^ 1, wf);
    if constexpr (decltype(issue_next)::value) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 1);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 1);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
      }
    } else if constexpr (decltype(read_next)::value) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 1);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
      }
    }
    if constexpr (decltype(read_next)::value) {
      // W fragments 0-2 behind the MFMAs of column blocks 1-3, fragment 3 after the last
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 1);
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 1);
      }
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 1);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 1);
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 1);
    }
  };
  using T_ = std::true_type;
  using F_ = std::false_type;
  int kt = 0;
  for (; kt + 2 < nt; ++kt) body(kt, T_{}, T_{});
  if (kt + 1 < nt) body(kt++, F_{}, T_{});
  body(kt, F_{}, F_{});

  // ---- epilogue: acc * sx[m] * sw[n] (+ bias[n]) -> bf16, two column blocks (one 16-byte
  // store per lane and row) at a time so that their scales and bias stay in 16 registers
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int j = 0; j < 4; j += 2) {
    const int n0 = tn * 256 + wn * 64 + j * 16;
    f32x4 sv[2], bv[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int n = n0 + 16 * h + 4 * g;           // the lane's 4 columns of block j + h
      sv[h] = *(const f32x4*)(SW + n);
      bv[h] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (bias) {
        const uint2 bb = *(const uint2*)(bias + n);
        bv[h] = f32x4{__uint_as_float(bb.x << 16), __uint_as_float(bb.x & 0xffff0000u), __uint_as_float(bb.y << 16),
                      __uint_as_float(bb.y & 0xffff0000u)};
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int m = m0 + wm * 128 + i * 16 + r16;
      // the swap partners (lanes l, l ^ 16) hold the same row, so a row past M drops both together
      if (m >= M) continue;
      const float sc = SX[m];
      float x0[4], x1[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        x0[e] = acc[i][j][e] * sc * sv[0][e] + bv[0][e];
        x1[e] = acc[i][j + 1][e] * sc * sv[1][e] + bv[1][e];
      }
      store_pair16(Y + (size_t)m * ldy, n0, g, x0, x1);
    }
  }
}

}  // namespace

// q [M, K] e4m3 (contiguous), sx [M] fp32 <- x [M, K] bf16 with row stride ldx.
extern "C" int dgi_quant_rows_fp8(const void* x, int ldx, void* q, void* sx, int M, int K, hipStream_t s) {
  if (M <= 0 || K <= 0) return 0;
  if (K % 16 || ldx % 8 || ldx < K) return -3;
  if (K <= 2048)
    quant_rows_fp8_kernel<1><<<dim3((M + 3) / 4), 256, 0, s>>>((const uint16_t*)x, ldx, (uint8_t*)q, (float*)sx, M, K);
  else
    quant_rows_fp8_kernel<4><<<dim3(M), 256, 0, s>>>((const uint16_t*)x, ldx, (uint8_t*)q, (float*)sx, M, K);
  DGI_CHECK_LAUNCH();
  return 0;
}

// y [M, N] bf16 (row stride ldy) = (xq [M, K] · wq [N, K]^T) * sx[m] * sw[n] (+ bias[n]); bias may be null.
extern "C" int dgi_mfma_gemm_fp8(const void* xq, const void* sx, const void* wq, const void* sw, const void* bias,
                                 void* y, int ldy, int M, int N, int K, hipStream_t s) {
  if (M <= 0 || N <= 0) return 0;
  if (N % 256 || K % kBK || K <= 0 || ldy % 4 || ldy < N) return -3;
  if ((long long)M * K > 0x7fffffffLL || (long long)N * K > 0x7fffffffLL) return -2;   // 32-bit lane offsets
  const int tiles_m = (M + kBM - 1) / kBM;
  const long long total = (long long)tiles_m * (N / 256);
  if (total > 0x7fffffffLL) return -2;
  mfma_gemm_fp8_kernel<<<dim3((unsigned)total), 512, 0, s>>>((const uint8_t*)xq, (const float*)sx, (const uint8_t*)wq,
                                                             (const float*)sw, (const uint16_t*)bias, (uint16_t*)y,
                                                             ldy, M, K, tiles_m, (int)total);
  DGI_CHECK_LAUNCH();
  return 0;
}
