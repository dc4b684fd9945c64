// cad1's 4x4 / stride-2 / padding-1 conv family for gfx950: Conv2d(4, 2, 1) and ConvTranspose2d(4, 2, 1) as implicit
// GEMMs on f32 MFMA (gemm.h), their split-K reduces, and the single-channel ends on the VALU.
#include "gemm_launch.h"

namespace vad {

// =====================================================================================================
// Conv2d(kernel 4, stride 2, padding 1) and ConvTranspose2d(4, 2, 1) as implicit GEMMs over NHWC frames (cad1's
// VideoAutoEncoder, causal_anomaly_detection1.py:129-188): the im2col / col2im columns are never written.
//   conv4_fwd   out[p][n] = sum_{tap, c} src[2a - 1 + ky][2b - 1 + kx][c] wk[n][tap C + c] (+ bias): the 16-tap
//               gather (Conv2d forward; ConvTranspose2d input gradient with src = dY)
//   conv4_cls   the transposed direction, one GEMM per output parity class (py, px): rows 2a + py take ky in {1, 3}
//               (py = 0: source rows a, a - 1) or {0, 2} (py = 1: source rows a + 1, a), 2 x 2 taps scattered to
//               (2a + py, 2b + px) (+ bias) (Conv2d input gradient with src = dY; ConvTranspose2d forward)
//   conv4_wgrad the correlation sum over A's pixels p of A[p][r] src[2a - 1 + ky][2b - 1 + kx][c] into split-K slabs
//               [S][R][16 C] (Conv2d: A = dY, src = X; ConvTranspose2d: A = X, src = dY), summed by
//               conv4_wgrad_reduce into torch's [R][C][4][4] (Conv2d [Co][Ci], ConvTranspose2d [Ci][Co])
// =====================================================================================================
__global__ __launch_bounds__(256) void conv4_prep_kernel(const float* __restrict__ w, int D0, int D1,
                                                         float* __restrict__ wk, float* __restrict__ wc) {
  const int64_t total = (int64_t)D0 * D1 * 16;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int tap = (int)(i % 16), d1 = (int)((i / 16) % D1);
    const int64_t d0 = i / (16 * D1);
    const float v = w[i];
    if (wk) wk[d0 * 16 * D1 + tap * D1 + d1] = v;
    if (wc) {
      const int ky = tap / 4, kx = tap % 4;
      const int py = (ky & 1) ? 0 : 1, px = (kx & 1) ? 0 : 1;  // (odd ky: class row 0)
      const int r = ky >> 1, q = kx >> 1;                      // index among the class's 2 x 2 taps
      wc[((int64_t)(2 * py + px) * D1 + d1) * 4 * D0 + (2 * r + q) * D0 + d0] = v;
    }
  }
}

int conv4_prep(const float* w, int D0, int D1, float* wk, float* wc, hipStream_t st) {
  const int64_t total = (int64_t)D0 * D1 * 16;
  hipLaunchKernelGGL(conv4_prep_kernel, dim3((unsigned)std::min<int64_t>(cdiv(total, 256), 1024)), dim3(256), 0, st, w,
                     D0, D1, wk, wc);
  VAD_LAUNCH_CHECK();
  return 0;
}

// split-K when the tile grid leaves most CUs idle (the decoder's 4x4 / 8x8 frames): slabs [S][M][N] in scratch, summed
// in order (+ bias) by dense_splitk_reduce / conv4_cls_reduce
// (knob "conv4_split_tiles": tile grids smaller than this split K)
static int conv4_splits(int M, int N, int K, int64_t scratch_floats) {
  const int64_t tiles = cdiv(M, 64) * cdiv(N, 64);
  if (tiles >= g_conv4_split_tiles || scratch_floats <= 0) return 1;
  int s = (int)std::min<int64_t>(cdiv(1024, tiles), K / (2 * BK));
  while (s > 1 && (int64_t)s * M * N > scratch_floats) s /= 2;
  return std::max(1, s);
}

int conv4_fwd(const float* src, int NF, int H, int W, int C, const float* wk, const float* bias, int N, float* out,
              hipStream_t st, float* scratch, int64_t scratch_floats) {
  VAD_CHECK(C % 32 == 0 && H % 2 == 0 && W % 2 == 0 && N >= 1, "conv4_fwd: C % 32 == 0, even frames");
  const int OH = H / 2, OW = W / 2;
  const ConvGeom g{NF, OH, OW, 2, 2, H, W, C};
  TapTable taps;
  taps.ntaps = 16;
  for (int k = 0; k < 16; ++k) {
    taps.dh[k] = (int8_t)(k / 4 - 1);
    taps.dw[k] = (int8_t)(k % 4 - 1);
  }
  const int M = NF * OH * OW, K = 16 * C;
  const DenseEpiArgs pe{out, N, bias, 0, 0, 0, 0, 1.f, 0, nullptr, 1.f};
  const int splits = conv4_splits(M, N, K, scratch_floats);
  if (splits > 1) {
    int used = 1;
    VAD_CHECK(gather_fits((int64_t)g.imgs * g.SH * g.SW * g.C), "conv gather: source over 2 GB");
    typename ConvGatherKC<64>::Params pa{src, g, taps, nullptr, nullptr};
    typename DenseKC<64>::Params pb{wk, K, N, K};
    const EpiPartial::Params pp{scratch, N};
    VAD_TRY((launch_gemm<T64x64, ConvGatherKC, DenseKC, EpiPartial>(pa, pb, pp, M, N, K, splits, nullptr, st, &used)));
    return dense_splitk_reduce(scratch, used, M, N, pe, nullptr, st);
  }
  return with_tile(pick_fwd_tile(M, N), [&](auto cfg) -> int {
    using Cf = decltype(cfg);
    VAD_CHECK(gather_fits((int64_t)g.imgs * g.SH * g.SW * g.C), "conv gather: source over 2 GB");
    typename ConvGatherKC<Cf::BM>::Params pa{src, g, taps, nullptr, nullptr};
    typename DenseKC<Cf::BN>::Params pb{wk, K, N, K};
    return launch_gemm<Cf, ConvGatherKC, DenseKC, EpiDense>(pa, pb, pe, M, N, K, 1, nullptr, st);
  });
}

// out[img][2a + py][2b + px][n] = bias[n] + sum over the slabs of part[s][(img SH + a) SW + b][n]
__global__ __launch_bounds__(256) void conv4_cls_reduce_kernel(const float* __restrict__ part, int S, int M, int SH,
                                                               int SW, int N, int py, int px,
                                                               const float* __restrict__ bias, float* __restrict__ out) {
  const int64_t total = (int64_t)M * N;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float v = slab_sum(part + i, S, total);
    const int n = (int)(i % N);
    const int64_t m = i / N;
    const int b = (int)(m % SW);
    const int64_t ia = m / SW;
    const int a = (int)(ia % SH);
    const int64_t img = ia / SH;
    out[((img * 2 * SH + 2 * a + py) * 2 * SW + 2 * b + px) * N + n] = v + (bias ? bias[n] : 0.f);
  }
}

// the four parity classes go to one batched launch (whole K per block, bias in the epilogue) from knob
// "conv4_cls_batch_min" 64 x 64 class tiles up; below it, per-class split-K launches with a reduce each
int conv4_cls(const float* src, int NF, int SH, int SW, int C, const float* wc, const float* bias, int N, float* out,
              hipStream_t st, float* scratch, int64_t scratch_floats) {
  VAD_CHECK(C % 32 == 0 && N >= 1, "conv4_cls: C % 32 == 0");
  const int Mc = NF * SH * SW;
  if (cdiv(Mc, 64) * cdiv(N, 64) * 4 >= g_conv4_cls_batch_min || scratch_floats <= 0) {
    // the four classes in one launch (blockIdx.z = class, the 3-D class-batched GEMM with a depth of 1)
    Conv3ClsGeom g{};
    g.imgs = NF; g.SD = 1; g.SH = SH; g.SW = SW; g.C = C;
    EpiConv3DgradCls::Params pe{};
    pe.dst = out; pe.imgs = NF; pe.DD = 1; pe.DH = 2 * SH; pe.DW = 2 * SW; pe.C = N; pe.bias = bias;
    for (int cls = 0; cls < 4; ++cls) {
      const int py = cls >> 1, px = cls & 1;
      g.GD[cls] = pe.GD[cls] = 1;
      g.GA[cls] = pe.GA[cls] = SH;
      g.GB[cls] = pe.GB[cls] = SW;
      TapTable3& taps = g.taps[cls];
      taps.ntaps = 4;
      for (int r = 0; r < 2; ++r)
        for (int q = 0; q < 2; ++q) {
          taps.dd[2 * r + q] = 0;
          taps.dh[2 * r + q] = (int8_t)(py == 0 ? -r : 1 - r);
          taps.dw[2 * r + q] = (int8_t)(px == 0 ? -q : 1 - q);
        }
    }
    const int K = 4 * C;
    return with_tile(pick_dgrad_tile(Mc, N), [&](auto cfg) -> int {
      using Cf = decltype(cfg);
      VAD_CHECK(gather_fits((int64_t)g.imgs * g.SD * g.SH * g.SW * g.C), "conv gather: source over 2 GB");
      typename ConvGather3ClsKC<Cf::BM>::Params pa{src, g};
      typename DenseKCz<Cf::BN>::Params pb{wc, {}, {}, N};
      for (int c = 0; c < 4; ++c) {
        pb.off[c] = (int64_t)c * N * K;
        pb.kdim[c] = K;
      }
      const dim3 grid((unsigned)cdiv(Mc, Cf::BM), (unsigned)cdiv(N, Cf::BN), 4u);
      VAD_KLAUNCH((gemm_kernel<Cf, ConvGather3ClsKC<Cf::BM>, DenseKCz<Cf::BN>, EpiConv3DgradCls>), grid, dim3(256), 0,
                  st, pa, pb, pe, Mc, N, K, -1, nullptr);
      VAD_LAUNCH_CHECK();
      return 0;
    });
  }
  for (int cls = 0; cls < 4; ++cls) {
    const int py = cls >> 1, px = cls & 1;
    const ConvGeom g{NF, SH, SW, 1, 1, SH, SW, C};
    TapTable taps;
    taps.ntaps = 4;
    for (int r = 0; r < 2; ++r)
      for (int q = 0; q < 2; ++q) {
        taps.dh[2 * r + q] = (int8_t)(py == 0 ? -r : 1 - r);
        taps.dw[2 * r + q] = (int8_t)(px == 0 ? -q : 1 - q);
      }
    const int M = NF * SH * SW, K = 4 * C;
    const int splits = conv4_splits(M, N, K, scratch_floats);
    if (splits > 1) {
      int used = 1;
      VAD_CHECK(gather_fits((int64_t)g.imgs * g.SH * g.SW * g.C), "conv gather: source over 2 GB");
      typename ConvGatherKC<64>::Params pa{src, g, taps, nullptr, nullptr};
      typename DenseKC<64>::Params pb{wc + (int64_t)cls * N * 4 * C, K, N, K};
      const EpiPartial::Params pp{scratch, N};
      VAD_TRY((launch_gemm<T64x64, ConvGatherKC, DenseKC, EpiPartial>(pa, pb, pp, M, N, K, splits, nullptr, st,
                                                                     &used)));
      const int64_t total = (int64_t)M * N;
      hipLaunchKernelGGL(conv4_cls_reduce_kernel, dim3((unsigned)std::min<int64_t>(cdiv(total, 256), 1024)),
                         dim3(256), 0, st, scratch, used, M, SH, SW, N, py, px, bias, out);
      VAD_LAUNCH_CHECK();
      continue;
    }
    const EpiConvDgrad::Params pe{out, SH, SW, 2, py, 2, px, 2 * SH, 2 * SW, N, bias};
    VAD_TRY(dgrad_launch(g, taps, src, wc + (int64_t)cls * N * 4 * C, N, pe, st));
  }
  return 0;
}

int conv4_wgrad(const float* A, int R, const float* src, int C, int NF, int AH, int AW, float* part, int* nsplit,
                int64_t part_cap, int target_blocks, hipStream_t st) {
  VAD_CHECK(C % 4 == 0 && R % 4 == 0, "conv4_wgrad: channel counts % 4 == 0");
  const int M = R, N = 16 * C, K = NF * AH * AW;
  VAD_CHECK((int64_t)M * N <= part_cap, "conv4_wgrad: slab too small");
  return with_tile(pick_wgrad_tile(M, N), [&](auto cfg) -> int {
    using Cf = decltype(cfg);
    const int tiles = (int)(cdiv(M, Cf::BM) * cdiv(N, Cf::BN));
    int splits = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(target_blocks, tiles), cdiv(K, 16 * BK)));
    while ((int64_t)splits * M * N > part_cap && splits > 1) splits /= 2;
    VAD_CHECK(gather_fits((int64_t)K * R), "dense gather: operand over 2 GB");
    typename DenseKM<Cf::BM>::Params pa{A, R, R, K, -1};
    VAD_CHECK(gather_fits((int64_t)NF * 2 * AH * 2 * AW * C), "conv patch: source over 2 GB");
    typename ConvPatchKM<Cf::BN>::Params pb{src, NF, AH, AW, 2, 1, 2 * AH, 2 * AW, C, 4, N, nullptr, nullptr};
    const EpiPartial::Params pe{part, N};
    return launch_gemm<Cf, DenseKM, ConvPatchKM, EpiPartial>(pa, pb, pe, M, N, K, splits, nullptr, st, nsplit);
  });
}

// dW[r][c][tap] = sum over the S slabs, in order, of part[s][r][tap C + c] (NT taps: 16 for the 4x4 convs, 27 for
// the 3-D ones)
// (slab rows of ld floats: the NT C weight columns, then with db the bias column NT C)
__global__ __launch_bounds__(256) void conv4_wgrad_reduce_kernel(const float* __restrict__ part, int S, int R, int C,
                                                                 int NT, int ld, float* __restrict__ dW,
                                                                 float* __restrict__ db) {
  const int W1 = NT * C + (db ? 1 : 0);
  const int64_t total = (int64_t)R * W1, slab = (int64_t)R * ld;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / W1;
    const int col = (int)(i - r * W1);
    const float s = slab_sum(part + r * ld + col, S, slab);
    if (col == NT * C) {
      db[r] = s;
    } else {
      const int c = col % C, tap = col / C;
      dW[(r * C + c) * NT + tap] = s;
    }
  }
}

// the same for many slabs: 64 consecutive entries x 4 slab lanes per block (lane l adds slabs l, l + 4, ... in order
// with 8 loads in flight, coalesced across the 64 entries), the 4 lane sums combined in a fixed order
__global__ __launch_bounds__(256) void conv4_wgrad_reduce_small_kernel(const float* __restrict__ part, int S, int R,
                                                                       int C, int NT, int ld, float* __restrict__ dW,
                                                                       float* __restrict__ db) {
  __shared__ float red[4][64];
  const int W1 = NT * C + (db ? 1 : 0);
  const int64_t total = (int64_t)R * W1, slab = (int64_t)R * ld;
  const int e = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 64 + e;
  const int64_t row = i / W1, col = i - row * W1, pi = row * ld + col;
  float v = 0.f;
  if (i < total) {
    const int n = S > sl ? (S - sl + 3) / 4 : 0;
    for (int k0 = 0; k0 < n; k0 += 8) {
      float u[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) u[q] = part[(int64_t)(sl + 4 * min(k0 + q, n - 1)) * slab + pi];
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (k0 + q < n) v += u[q];
    }
  }
  red[sl][e] = v;
  __syncthreads();
  if (sl == 0 && i < total) {
    const float t = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
    if (col == NT * C) {
      db[row] = t;
    } else {
      const int c = (int)(col % C), tap = (int)(col / C);
      dW[(row * C + c) * NT + tap] = t;
    }
  }
}

// slabs [S][R][ld] -> dW (torch [R][C][taps]) and, with db, the bias column NT C of each row
int taps_wgrad_reduce(const float* part, int S, int R, int C, int NT, float* dW, hipStream_t st, int ld, float* db) {
  if (ld <= 0) ld = NT * C;
  const int64_t total = (int64_t)R * (NT * C + (db ? 1 : 0));
  if (S >= 16) {
    hipLaunchKernelGGL(conv4_wgrad_reduce_small_kernel, dim3((unsigned)cdiv(total, 64)), dim3(256), 0, st, part, S, R, C,
                       NT, ld, dW, db);
    VAD_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL(conv4_wgrad_reduce_kernel, dim3((unsigned)std::min<int64_t>(cdiv(total, 256), 2048)), dim3(256), 0,
                     st, part, S, R, C, NT, ld, dW, db);
  VAD_LAUNCH_CHECK();
  return 0;
}

int conv4_wgrad_reduce(const float* part, int S, int R, int C, float* dW, hipStream_t st) {
  return taps_wgrad_reduce(part, S, R, C, 16, dW, st);
}

// ---------------------------------------------------------------- the single-channel ends (cad1:131, cad1:185)
// conv4_c1_fwd  out[p][n] = sum_tap src[2a - 1 + ky][2b - 1 + kx] w[n][tap] (+ bias[n]), 1-channel NHWC source, 32
//               outputs per pixel on the VALU (Conv2d(1, 32) forward; ConvTranspose2d(32, 1) input gradient with
//               src = dY, w = the [32][1][4][4] weight)
// conv4_c1_tfwd out[2a + py][2b + px] = bias + sum over the class taps and the 32 source channels (ConvTranspose2d(32,
//               1) forward)
// conv4_c1_wgrad slab[block][r][tap] = sum over the block's pixels p of A[p][r] src[2a - 1 + ky][2b - 1 + kx] (r < 32;
//               Conv2d(1, 32): A = dY; ConvTranspose2d(32, 1): A = X, src = dY)
__global__ __launch_bounds__(256) void conv4_c1_fwd_kernel(const float* __restrict__ src, int NF, int H, int W,
                                                           const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float ws[16][32];  // [tap][n]
  __shared__ __attribute__((aligned(16))) float os[256 * 33];  // the block's 256 output rows, written back coalesced
  for (int i = threadIdx.x; i < 512; i += 256) ws[i % 16][i / 16] = w[i];
  const int OH = H / 2, OW = W / 2;
  const int64_t total = (int64_t)NF * OH * OW;
  for (int64_t p0 = blockIdx.x * 256ll; p0 < total; p0 += (int64_t)gridDim.x * 256) {
    __syncthreads();
    const int64_t p = p0 + threadIdx.x;
    if (p < total) {
      const int ox = (int)(p % OW);
      const int64_t r = p / OW;
      const int oy = (int)(r % OH);
      const float* img = src + (r / OH) * H * W;
      float x[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int iy = 2 * oy - 1 + t / 4, ix = 2 * ox - 1 + t % 4;
        x[t] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? img[iy * W + ix] : 0.f;
      }
#pragma unroll
      for (int n4 = 0; n4 < 8; ++n4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(&ws[t][4 * n4]);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = fmaf(x[t], wv[e], acc[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) os[threadIdx.x * 33 + 4 * n4 + e] = acc[e] + (bias ? bias[4 * n4 + e] : 0.f);
      }
    }
    __syncthreads();
    const int64_t nrow = min((int64_t)256, total - p0);
    for (int i = threadIdx.x; i < nrow * 8; i += 256) {  // 8 float4 per output row, consecutive lanes -> consecutive
      const int row = i >> 3, c4 = (i & 7) * 4;
      const f32x4 v = {os[row * 33 + c4], os[row * 33 + c4 + 1], os[row * 33 + c4 + 2], os[row * 33 + c4 + 3]};
      *reinterpret_cast<f32x4*>(out + (p0 + row) * 32 + c4) = v;
    }
  }
}

__global__ __launch_bounds__(256) void conv4_c1_tfwd_kernel(const float* __restrict__ src, int NF, int SH, int SW,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float ws[16][32];  // [tap][source channel]
  for (int i = threadIdx.x; i < 512; i += 256) ws[i % 16][i / 16] = w[i];
  __syncthreads();
  const int OH = 2 * SH, OW = 2 * SW;
  const int64_t total = (int64_t)NF * OH * OW;
  const float b0 = bias ? bias[0] : 0.f;
  for (int64_t p = blockIdx.x * 256ll + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
    const int ox = (int)(p % OW);
    const int64_t r = p / OW;
    const int oy = (int)(r % OH);
    const int64_t img = r / OH;
    const int py = oy & 1, px = ox & 1, a = oy >> 1, b = ox >> 1;
    float acc = 0.f;
#pragma unroll
    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int sy = a + (py == 0 ? -rr : 1 - rr), sx = b + (px == 0 ? -q : 1 - q);
        if (sy < 0 || sy >= SH || sx < 0 || sx >= SW) continue;
        const int ky = py == 0 ? 1 + 2 * rr : 2 * rr, kx = px == 0 ? 1 + 2 * q : 2 * q;
        const float* xs = src + ((img * SH + sy) * SW + sx) * 32;
        const float* wt = ws[ky * 4 + kx];
#pragma unroll
        for (int c4 = 0; c4 < 8; ++c4) {
          const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + 4 * c4);
          const f32x4 wv = *reinterpret_cast<const f32x4*>(wt + 4 * c4);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc = fmaf(xv[e], wv[e], acc);
        }
      }
    out[p] = acc + b0;
  }
}

// conv4_c1_wgrad: a block walks tiles of 256 consecutive A pixels (256 / AW whole rows of one image); the tile's A rows
// (256 x 32) and its 1-channel source halo ((2 TR + 2) x (2 AW + 2)) in LDS, thread (channel r, tap pair) sums over the
// tile's pixels (three LDS reads, two FMAs per pixel)
constexpr int C1_TILE = 256;

// thread = 4 output channels (quad q) x 2 taps (pair p) over one wave's share of the tile's pixel rows (wave w takes
// rows w, w + 4, ...): per pixel one 16-B read of the dY quad and two halo reads feed 8 FMAs; the four waves' sums are
// combined in a fixed order at the end
__global__ __launch_bounds__(256) void conv4_c1_wgrad_kernel(const float* __restrict__ A, const float* __restrict__ src,
                                                             int NF, int AH, int AW, float* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) float as[C1_TILE][32];
  __shared__ float xs[(2 * C1_TILE / 8 + 2) * (2 * 64 + 2)];  // (AW >= 8, AW <= 64)
  __shared__ float red[4][512];
  const int H = 2 * AH, W = 2 * AW, TR = C1_TILE / AW, XW = 2 * AW + 2, XR = 2 * TR + 2;
  const int64_t ntiles = (int64_t)NF * AH / TR;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, q = lane & 7, p = lane >> 3;
  const int k0 = 2 * p, k1 = 2 * p + 1;
  const int o0 = (k0 / 4) * XW + k0 % 4, o1 = (k1 / 4) * XW + k1 % 4;  // tap offsets in the halo
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t img = tile / (AH / TR);
    const int y0 = (int)(tile % (AH / TR)) * TR;  // first A row of the tile
    __syncthreads();
    const float* arow = A + ((img * AH + y0) * (int64_t)AW) * 32;
    for (int i = t; i < C1_TILE * 8; i += 256)
      *reinterpret_cast<f32x4*>(&as[i >> 3][(i & 7) * 4]) = *reinterpret_cast<const f32x4*>(arow + (int64_t)i * 4);
    const float* simg = src + img * (int64_t)H * W;
    for (int i = t; i < XR * XW; i += 256) {
      const int hy = i / XW, hx = i - hy * XW;
      const int iy = 2 * y0 - 1 + hy, ix = hx - 1;
      xs[i] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? simg[(int64_t)iy * W + ix] : 0.f;
    }
    __syncthreads();
    for (int vy = wv; vy < TR; vy += 4) {  // (pixel v = vy * AW + vx, walked without divisions)
      const float* xrow = xs + 2 * vy * XW;
#pragma unroll 4
      for (int vx = 0; vx < AW; ++vx) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(&as[vy * AW + vx][4 * q]);
        const float x0 = xrow[2 * vx + o0], x1 = xrow[2 * vx + o1];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc0[e] = fmaf(a[e], x0, acc0[e]);
          acc1[e] = fmaf(a[e], x1, acc1[e]);
        }
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[wv][(4 * q + e) * 16 + k0] = acc0[e];
    red[wv][(4 * q + e) * 16 + k1] = acc1[e];
  }
  __syncthreads();
  for (int i = t; i < 512; i += 256)
    slab[(int64_t)blockIdx.x * 512 + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}

int conv4_c1_fwd(const float* src, int NF, int H, int W, const float* w, const float* bias, float* out,
                 hipStream_t st) {
  VAD_CHECK(H % 2 == 0 && W % 2 == 0, "conv4_c1_fwd: even frames");
  const int64_t total = (int64_t)NF * (H / 2) * (W / 2);
  hipLaunchKernelGGL(conv4_c1_fwd_kernel, dim3((unsigned)std::min<int64_t>(cdiv(total, 256), 4096)), dim3(256), 0, st,
                     src, NF, H, W, w, bias, out);
  VAD_LAUNCH_CHECK();
  return 0;
}

int conv4_c1_tfwd(const float* src, int NF, int SH, int SW, const float* w, const float* bias, float* out,
                  hipStream_t st) {
  const int64_t total = (int64_t)NF * 4 * SH * SW;
  hipLaunchKernelGGL(conv4_c1_tfwd_kernel, dim3((unsigned)std::min<int64_t>(cdiv(total, 256), 4096)), dim3(256), 0, st,
                     src, NF, SH, SW, w, bias, out);
  VAD_LAUNCH_CHECK();
  return 0;
}

int conv4_c1_wgrad(const float* A, const float* src, int NF, int AH, int AW, float* dW, float* slab,
                   int64_t slab_floats, hipStream_t st) {
  VAD_CHECK(AW >= 8 && AW <= 64 && C1_TILE % AW == 0 && AH % (C1_TILE / AW) == 0,
            "conv4_c1_wgrad: 256 / AW whole rows per tile");
  const int64_t ntiles = (int64_t)NF * AH * AW / C1_TILE;
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>({ntiles, 512, slab_floats / 512}));
  hipLaunchKernelGGL(conv4_c1_wgrad_kernel, dim3((unsigned)blocks), dim3(256), 0, st, A, src, NF, AH, AW, slab);
  VAD_LAUNCH_CHECK();
  return conv4_wgrad_reduce(slab, blocks, 32, 1, dW, st);
}
}  // namespace vad
