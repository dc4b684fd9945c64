// Launch side of the generic GEMM (gemm.h): the epilogues, launch_gemm, the tile shapes and their dispatchers, and the
// tile heuristics.  Included by the files that launch gemm_kernel: backbone.hip (3x3 convs, dense layers), conv4.hip
// and conv3s2.hip.
#pragma once
#include "backbone.h"
#include "gemm.h"

namespace vad {

// =====================================================================================================
// GEMM epilogues
// =====================================================================================================
struct EpiConvFwd {  // y = acc + bias (NHWC rows), plus per-block BN partial sums
  static constexpr int SCRATCH = 2 * 4 * 256;
  struct Params { float* y; const float* bias; int C; float* partials; };
  template <class Cfg>
  static __device__ void apply(const Params& P, f32x16 (&acc)[Cfg::TM][Cfg::TN], int m0, int n0, int wm, int wn,
                               int lane, int M, int N, float* lds) {
    float s1[Cfg::TN], s2[Cfg::TN];
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j) {
      s1[j] = s2[j] = 0.f;
      const int col = n0 + acc_col<Cfg>(wn, j, lane);
      const float bj = col < N ? P.bias[col] : 0.f;
#pragma unroll
      for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = m0 + acc_row<Cfg>(wm, i, r, lane);
          if (row < M && col < N) {
            const float v = acc[i][j][r] + bj;
            P.y[(int64_t)row * P.C + col] = v;
            s1[j] += v;
            s2[j] = fmaf(v, v, s2[j]);
          }
        }
      s1[j] += __shfl_xor(s1[j], 32, 64);
      s2[j] += __shfl_xor(s2[j], 32, 64);
    }
    // lds is free: the main loop ended with a barrier
    constexpr int BN = Cfg::BN;
    if (lane < 32) {
#pragma unroll
      for (int j = 0; j < Cfg::TN; ++j) {
        const int c = (wn * Cfg::TN + j) * 32 + lane;
        lds[wm * BN + c] = s1[j];
        lds[Cfg::WM * BN + wm * BN + c] = s2[j];
      }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < BN; c += 256) {
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int w = 0; w < Cfg::WM; ++w) {
        a += lds[w * BN + c];
        b += lds[Cfg::WM * BN + w * BN + c];
      }
      if (n0 + c < N) {
        P.partials[(int64_t)blockIdx.x * 2 * P.C + n0 + c] = a;
        P.partials[(int64_t)blockIdx.x * 2 * P.C + P.C + n0 + c] = b;
      }
    }
  }
};

struct EpiConvDgrad {  // scatter rows of a (parity-class) grid back to the full NHWC input gradient (+ bias)
  static constexpr int SCRATCH = 0;
  struct Params { float* dst; int GA, GB, ra, pa, rb, pb, DH, DW, C; const float* bias; };
  template <class Cfg>
  static __device__ void apply(const Params& P, f32x16 (&acc)[Cfg::TM][Cfg::TN], int m0, int n0, int wm, int wn,
                               int lane, int M, int N, float*) {
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + acc_row<Cfg>(wm, i, r, lane);
        if (row >= M) continue;
        const int img = row / (P.GA * P.GB);
        const int rem = row - img * P.GA * P.GB;
        const int a = rem / P.GB, b = rem - a * P.GB;
        const int64_t base = (((int64_t)img * P.DH + a * P.ra + P.pa) * P.DW + b * P.rb + P.pb) * P.C;
#pragma unroll
        for (int j = 0; j < Cfg::TN; ++j) {
          const int col = n0 + acc_col<Cfg>(wn, j, lane);
          if (col < N) P.dst[base + col] = acc[i][j][r] + (P.bias ? P.bias[col] : 0.f);
        }
      }
  }
};

struct EpiPartial {  // split-K slab: part[z][row][col]
  static constexpr int SCRATCH = 0;
  struct Params { float* part; int64_t ld; };
  template <class Cfg>
  static __device__ void apply(const Params& P, f32x16 (&acc)[Cfg::TM][Cfg::TN], int m0, int n0, int wm, int wn,
                               int lane, int M, int N, float*) {
    float* base = P.part + (int64_t)blockIdx.z * M * P.ld;
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + acc_row<Cfg>(wm, i, r, lane);
        if (row >= M) continue;
#pragma unroll
        for (int j = 0; j < Cfg::TN; ++j) {
          const int col = n0 + acc_col<Cfg>(wn, j, lane);
          if (col < N) base[(int64_t)row * P.ld + col] = acc[i][j][r];
        }
      }
  }
};

struct DenseEpiArgs {
  float* out; int64_t ldc; const float* bias; int relu; int drop; uint64_t h1; uint32_t thr; float dscale;
  int64_t row0; const float* gate; float gscale;
  int gmod;  // gate row = row % gmod when > 0 (the stacked rows of the direct classifier's affine backward)
};

__device__ inline float dense_finish(const DenseEpiArgs& P, int row, int col, float v) {
  if (P.bias) v += P.bias[col];
  if (P.relu) v = relu_nan(v);
  if (P.drop) v = (rng_u24(P.h1, (uint64_t)(P.row0 + row), (uint64_t)col) >= P.thr) ? v * P.dscale : 0.f;
  if (P.gate) v = P.gate[(int64_t)(P.gmod > 0 ? row % P.gmod : row) * P.ldc + col] > 0.f ? v * P.gscale : 0.f;
  return v;
}

struct EpiDense {
  static constexpr int SCRATCH = 0;
  using Params = DenseEpiArgs;
  template <class Cfg>
  static __device__ void apply(const Params& P, f32x16 (&acc)[Cfg::TM][Cfg::TN], int m0, int n0, int wm, int wn,
                               int lane, int M, int N, float*) {
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + acc_row<Cfg>(wm, i, r, lane);
        if (row >= M) continue;
#pragma unroll
        for (int j = 0; j < Cfg::TN; ++j) {
          const int col = n0 + acc_col<Cfg>(wn, j, lane);
          if (col < N) P.out[(int64_t)row * P.ldc + col] = dense_finish(P, row, col, acc[i][j][r]);
        }
      }
  }
};

// scatter the rows of parity-class grids to the NDHWC input gradient, for the class-batched GEMM: class = blockIdx.z, its
// own grid (conv3s2_dgrad; conv4_cls with a depth of 1)
struct EpiConv3DgradCls {
  static constexpr int SCRATCH = 0;
  struct Params {
    float* dst; int imgs; int GD[8], GA[8], GB[8]; int DD, DH, DW, C; const float* bias;
    const float* gate;  // nullable, dst's layout: dst = 0 where !(gate > 0) (the producing ReLU's backward, fused)
    int rev;            // blockIdx.z = 7 - class (the heaviest classes dispatched first); the tables are in z order
  };
  template <class Cfg>
  static __device__ void apply(const Params& P, f32x16 (&acc)[Cfg::TM][Cfg::TN], int m0, int n0, int wm, int wn,
                               int lane, int, int N, float*) {
    const int z = blockIdx.z, cls = P.rev ? 7 - z : z, pd = (cls >> 2) & 1, ph = (cls >> 1) & 1, pw = cls & 1;
    const int GD = P.GD[z], GA = P.GA[z], GB = P.GB[z], per = GD * GA * GB;
    if (per == 0) return;
    // a lane's 16 rows come in 4 runs of 4 consecutive rows (acc_row): the first row of a run is decomposed into
    // (img, a, b, c) by division, the next three by a carrying +1 (the divisions by the class grid were most of the
    // kernel's VALU work: 38 VALU per MFMA)
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row0 = m0 + acc_row<Cfg>(wm, i, 4 * q, lane);
        int img = row0 / per;
        const int rem = row0 - img * per;
        int a = rem / (GA * GB);
        const int r2 = rem - a * GA * GB;
        int b = r2 / GB, c = r2 - b * GB;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (u > 0) {  // row0 + u: c + 1 with carries into b, a, img
            ++c;
            const bool cb = c == GB;
            c = cb ? 0 : c;
            b += cb;
            const bool ca = b == GA;
            b = ca ? 0 : b;
            a += ca;
            const bool ci = a == GD;
            a = ci ? 0 : a;
            img += ci;
          }
          if (img >= P.imgs) continue;
          const int64_t base = ((((int64_t)img * P.DD + 2 * a + pd) * P.DH + 2 * b + ph) * P.DW + 2 * c + pw) * P.C;
          const int r = 4 * q + u;
#pragma unroll
          for (int j = 0; j < Cfg::TN; ++j) {
            const int col = n0 + acc_col<Cfg>(wn, j, lane);
            if (col < N) {
              const float v = acc[i][j][r] + (P.bias ? P.bias[col] : 0.f);
              P.dst[base + col] = (P.gate && !(P.gate[base + col] > 0.f)) ? 0.f : v;
            }
          }
        }
      }
  }
};

// sum_{z < S} p[z * stride] in z order, 8 loads in flight (clamped, unconditional): the slab sums of the split-K
// reduces (a plain loop leaves one dependent load round trip per slab)
__device__ __forceinline__ float slab_sum(const float* __restrict__ p, int S, int64_t stride) {
  float s = 0.f;
  for (int z0 = 0; z0 < S; z0 += 8) {
    float u[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] = p[(int64_t)min(z0 + k, S - 1) * stride];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (z0 + k < S) s += u[k];
  }
  return s;
}

// out = finish(sum of the S split-K slabs part[s][M][N], in order): bias, ReLU, dropout, gate of pe (backbone.hip)
int dense_splitk_reduce(const float* part, int S, int M, int N, const DenseEpiArgs& pe, const int* skip,
                        hipStream_t st);
// slabs [S][R][ld] -> dW (torch [R][C][NT taps]) and, with db, the bias column NT C of each row (conv4.hip)
int taps_wgrad_reduce(const float* part, int S, int R, int C, int NT, float* dW, hipStream_t st, int ld = 0,
                      float* db = nullptr);

// =====================================================================================================
// launch helpers
// =====================================================================================================
template <class Cfg, template <int> class LA, template <int> class LB, class Epi>
static int launch_gemm(const typename LA<Cfg::BM>::Params& pa, const typename LB<Cfg::BN>::Params& pb,
                       const typename Epi::Params& pe, int M, int N, int K, int splits, const int* skip,
                       hipStream_t st, int* used_splits = nullptr) {
  if (M <= 0 || N <= 0) return 0;
  splits = std::max(1, splits);
  int kps = (int)(cdiv(cdiv(K, splits), BK) * BK);
  if (kps <= 0) kps = BK;
  splits = (int)cdiv(K, kps);
  if (splits < 1) splits = 1;
  dim3 grid((unsigned)cdiv(M, Cfg::BM), (unsigned)cdiv(N, Cfg::BN), (unsigned)splits);
  VAD_KLAUNCH((gemm_kernel<Cfg, LA<Cfg::BM>, LB<Cfg::BN>, Epi>), grid, dim3(256), 0, st, pa, pb, pe, M, N, K,
                     kps, skip);
  VAD_LAUNCH_CHECK();
  if (used_splits) *used_splits = splits;
  return 0;
}

using T64x64 = TileCfg<2, 2, 1, 1>;

// runtime-selectable tile shapes for the conv GEMMs (tuning / sweeps); id -> TileCfg
template <class F>
static int with_tile(int id, F&& f) {
  switch (id) {
    case 0: return f(TileCfg<4, 1, 1, 1>{});  // 128 x 32
    case 1: return f(TileCfg<4, 1, 2, 1>{});  // 256 x 32
    case 2: return f(TileCfg<2, 2, 1, 1>{});  //  64 x 64
    case 3: return f(TileCfg<2, 2, 2, 1>{});  // 128 x 64
    case 4: return f(TileCfg<2, 2, 1, 2>{});  //  64 x 128
    case 5: return f(TileCfg<2, 2, 2, 2>{});  // 128 x 128
    case 6: return f(TileCfg<4, 1, 2, 2>{});  // 256 x 64
    case 7: return f(TileCfg<1, 4, 1, 1>{});  //  32 x 128
    case 8: return f(TileCfg<1, 4, 1, 2>{});  //  32 x 256
    case 9: return f(TileCfg<2, 2, 1, 4>{});  //  64 x 256
    default: set_error("unknown tile id"); return 1;
  }
}
inline int tile_bm(int id) {
  static const int bm[10] = {128, 256, 64, 128, 64, 128, 256, 32, 32, 64};
  return (id >= 0 && id < 10) ? bm[id] : 64;
}

// heuristics (fallback when no tile is forced); BM >= 64 keeps the forward BN partial count within bounds
inline int pick_fwd_tile(int M, int N) {
  if (g_conv_fwd_tile >= 0 && tile_bm(g_conv_fwd_tile) >= 64) return g_conv_fwd_tile;
  if (N == 32) return 0;
  return M >= 64 * 1024 ? 3 : 2;
}
inline int pick_dgrad_tile(int M, int N) {
  if (g_conv_dgrad_tile >= 0) return g_conv_dgrad_tile;
  if (N <= 32) return 0;  // (128 x 32: a2's 16-channel input gradient wastes half a tile instead of three quarters)
  return M >= 64 * 1024 ? 3 : 2;
}
inline int pick_wgrad_tile(int M, int N) {
  (void)N;
  if (g_conv_wgrad_tile >= 0) return g_conv_wgrad_tile;
  return M == 32 ? 7 : 2;
}

// one input-gradient GEMM over a (parity-class) grid: the 3x3 convs' GEMM path and conv4_cls's per-class launches
inline int dgrad_launch(const ConvGeom& g, const TapTable& taps, const float* dY, const float* wd, int N,
                        const EpiConvDgrad::Params& pe, hipStream_t st) {
  const int M = g.imgs * g.GA * g.GB, K = taps.ntaps * g.C;
  return with_tile(pick_dgrad_tile(M, N), [&](auto cfg) -> int {
    using C = decltype(cfg);
    VAD_CHECK(gather_fits((int64_t)g.imgs * g.SH * g.SW * g.C), "conv gather: source over 2 GB");
    typename ConvGatherKC<C::BM>::Params pa{dY, g, taps, nullptr, nullptr};
    typename DenseKC<C::BN>::Params pb{wd, K, N, K};
    return launch_gemm<C, ConvGatherKC, DenseKC, EpiConvDgrad>(pa, pb, pe, M, N, K, 1, nullptr, st);
  });
}

}  // namespace vad
