// Per-frame CNN kernels for gfx950: conv1 (f32 MFMA, K = 49) and the stem backward, the 3x3 convs' dispatch and their
// implicit-GEMM path on f32 MFMA, train-mode BatchNorm forward/backward, max/adaptive-avg pooling, and the dense-layer
// GEMMs.  The GEMM's launch side is gemm_launch.h; the 4x4 and 3-D stride-2 conv families are conv4.hip / conv3s2.hip.
// Reference semantics: ResNetBackbone (causal_anomaly_detection.py:110-158), nn.BatchNorm2d train mode,
// nn.MaxPool2d(3,2,1), nn.AdaptiveAvgPool2d((4,6)), nn.Linear / ReLU / Dropout stacks (cad:167-179, 525-538).
#include <type_traits>

#include "gemm_launch.h"

namespace vad {

// =====================================================================================================
// conv1: 1 -> 32 channels, 7x7, stride 2, pad 3, as a K=49 (padded to 56) GEMM on f32 MFMA.
// One block = one frame x a band of C1_RB output rows.  The zero-padded input band is staged in LDS; each wave
// walks 32-pixel tiles of the band: lane (i, h) gathers its A operand patch[2*oy+kh][2*ox+kw] straight from LDS
// (k = 8*kk + 4*h + s), its B operand (weights of channel lane&31) lives in 28 registers for the whole block.
// Epilogue: +bias, NHWC store (one 128-B row per pixel), per-block BN partial sums (deterministic).
// =====================================================================================================
constexpr int C1_RB = 6;  // 114 output rows at 227x227 = 19 full bands; 2432 blocks balance over 256 CUs
constexpr int C1_CO = 32;
constexpr int C1_K = 56;  // 49 taps padded to 7 MFMA sub-steps of 8

__global__ __launch_bounds__(256) void conv1_kernel(const float* __restrict__ x, int H, int W,
                                                    const float* __restrict__ w, const float* __restrict__ bias,
                                                    float* __restrict__ y, int OH, int OW, int bands,
                                                    float* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int img = blockIdx.x / bands, band = blockIdx.x % bands;
  const int r0 = band * C1_RB;
  const int PW = 2 * OW + 6;  // padded band width
  const int PH = 2 * C1_RB + 5;
  float* patch = sm;  // [PH][PW]
  const float* xi = x + (int64_t)img * H * W;
  for (int i = threadIdx.x; i < PH * PW; i += 256) {
    const int pr = i / PW, pc = i - pr * PW;
    const int ih = 2 * r0 - 3 + pr, iw = pc - 3;
    patch[i] = (ih >= 0 && ih < H && iw >= 0 && iw < W) ? xi[(int64_t)ih * W + iw] : 0.f;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  // B operand: w[j][k] for k = 8*kk + 4*h + s, zero for k >= 49.  The A operand's patch offset of tap k,
  // (k/7)*PW + k%7, is rebuilt per MFMA from compile-time row/col constants selected by h (no 28-register
  // offset table: 4 instead of 3 waves per SIMD)
  float wr[28];
#pragma unroll
  for (int kk = 0; kk < 7; ++kk)
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const int k = kk * 8 + 4 * h + s4;
      wr[kk * 4 + s4] = k < 49 ? w[j * 49 + k] : 0.f;
    }
  const float bj = bias[j];
  __syncthreads();
  const int rows = min(C1_RB, OH - r0);
  const int npix = rows * OW;
  float s1 = 0.f, s2 = 0.f;
  for (int t0 = wave * 32; t0 < npix; t0 += 4 * 32) {
    // this lane's pixel for the A operand: i = lane & 31
    const int pa = t0 + (lane & 31);
    const int pac = pa < npix ? pa : npix - 1;
    const int oy = pac / OW, ox = pac - oy * OW;
    const float* pp = patch + (2 * oy) * PW + 2 * ox;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int q = 0; q < 28; ++q) {
      const int k0 = (q >> 2) * 8 + (q & 3), k1 = k0 + 4;  // tap of lane half 0 / 1
      const int kr = h ? (k1 < 49 ? k1 / 7 : 0) : (k0 < 49 ? k0 / 7 : 0);
      const int kc = h ? (k1 < 49 ? k1 % 7 : 0) : (k0 < 49 ? k0 % 7 : 0);
      acc = mfma32(pp[kr * PW + kc], wr[q], acc);
    }
    // the band's output pixels are contiguous in NHWC: the store address is linear in pi (no per-element divide)
    float* yb = y + (((int64_t)img * OH + r0) * OW) * C1_CO + j;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int pi = t0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (pi < npix) {
        const float v = acc[r] + bj;
        yb[(int64_t)pi * C1_CO] = v;
        s1 += v;
        s2 = fmaf(v, v, s2);
      }
    }
  }
  s1 += __shfl_xor(s1, 32, 64);
  s2 += __shfl_xor(s2, 32, 64);
  __syncthreads();
  float* red = sm;  // [4 waves][2][32]
  if (lane < 32) {
    red[wave * 64 + lane] = s1;
    red[wave * 64 + 32 + lane] = s2;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int t = threadIdx.x;
    const float v = red[t] + red[64 + t] + red[128 + t] + red[192 + t];
    partials[(int64_t)blockIdx.x * 2 * C1_CO + t] = v;  // [P][2*C]: sums then sums of squares
  }
}

int conv1_num_parts(int NF, int OH) { return NF * (int)cdiv(OH, C1_RB); }

// =====================================================================================================
// Stem backward (only when backbone.conv1 / bn1 train: the module API without apply_memory_efficient_training,
// cad:115-116,145-147; train_model freezes them, cad:592-598)
// =====================================================================================================
// conv1 weight gradient: dW[c][tap] = sum over output pixels of dY[p][c] * xpad[patch_p + tap], as f32 MFMA with
// M = 32 channels, K = pixels (two per MFMA), N = taps (two tiles: 0..31, 32..48).  One block per (frame, band of
// C1_RB output rows), the zero-padded input band staged in LDS as in the forward; the 4 waves take interleaved
// pixel pairs and are combined in a fixed order; each block writes its [32][49] partial to slab[blockIdx.x].
__global__ __launch_bounds__(256) void conv1_wgrad_kernel(const float* __restrict__ x, int H, int W,
                                                          const float* __restrict__ dy, int OH, int OW, int bands,
                                                          float* __restrict__ slab) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int img = blockIdx.x / bands, band = blockIdx.x % bands;
  const int r0 = band * C1_RB;
  const int PW = 2 * OW + 6, PH = 2 * C1_RB + 5;
  float* patch = sm;
  float* red = sm + ((PH * PW + 3) & ~3);  // [4 waves][2 tiles][16][64]
  const float* xi = x + (int64_t)img * H * W;
  for (int i = threadIdx.x; i < PH * PW; i += 256) {
    const int pr = i / PW, pc = i - pr * PW;
    const int ih = 2 * r0 - 3 + pr, iw = pc - 3;
    patch[i] = (ih >= 0 && ih < H && iw >= 0 && iw < W) ? xi[(int64_t)ih * W + iw] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int rows = min(C1_RB, OH - r0), npix = rows * OW;
  const float* dyb = dy + (((int64_t)img * OH + r0) * OW) * C1_CO;
  const int t1 = 32 + j;
  const int off0 = (j / 7) * PW + j % 7;
  const int off1 = t1 < 49 ? (t1 / 7) * PW + t1 % 7 : 0;
  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
  for (int p0 = wave * 2; p0 < npix; p0 += 8) {
    const int p = p0 + h;
    const bool ok = p < npix;
    const int pc = ok ? p : npix - 1;
    const float a = ok ? dyb[(int64_t)pc * C1_CO + j] : 0.f;  // A[c = j][k = h]
    const int oy = pc / OW, ox = pc - oy * OW;
    const float* pp = patch + (2 * oy) * PW + 2 * ox;
    acc0 = mfma32(a, pp[off0], acc0);
    acc1 = mfma32(a, t1 < 49 ? pp[off1] : 0.f, acc1);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    red[((wave * 2 + 0) * 16 + r) * 64 + lane] = acc0[r];
    red[((wave * 2 + 1) * 16 + r) * 64 + lane] = acc1[r];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * 16 * 64; e += 256) {
    const int tile = e / 1024, r = (e / 64) % 16, l = e % 64;
    const float v = (red[((0 * 2 + tile) * 16 + r) * 64 + l] + red[((1 * 2 + tile) * 16 + r) * 64 + l]) +
                    (red[((2 * 2 + tile) * 16 + r) * 64 + l] + red[((3 * 2 + tile) * 16 + r) * 64 + l]);
    const int c = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), tap = tile * 32 + (l & 31);
    if (tap < 49) slab[(int64_t)blockIdx.x * 32 * 49 + c * 49 + tap] = v;
  }
}

// dW (torch [32][1][7][7]) = sum of the blocks' partials, fixed order: 64 elements x 4 slab lanes per block
__global__ __launch_bounds__(256) void conv1_wgrad_reduce_kernel(const float* __restrict__ slab, int S,
                                                                 float* __restrict__ dw) {
  __shared__ float red[4][64];
  const int e = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
  float s0 = 0.f, s1 = 0.f;
  if (e < 32 * 49) {
    int s = g;
    for (; s + 4 < S; s += 8) {
      s0 += slab[(int64_t)s * 32 * 49 + e];
      s1 += slab[(int64_t)(s + 4) * 32 * 49 + e];
    }
    for (; s < S; s += 4) s0 += slab[(int64_t)s * 32 * 49 + e];
  }
  red[g][threadIdx.x & 63] = s0 + s1;
  __syncthreads();
  if (threadIdx.x < 64 && e < 32 * 49)
    dw[e] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

int conv1_wgrad(const float* x, int NF, int H, int W, const float* dy, int OH, int OW, float* slab,
                int64_t slab_cap, float* dw, hipStream_t st) {
  const int bands = (int)cdiv(OH, C1_RB);
  const int S = NF * bands;
  VAD_CHECK((int64_t)S * 32 * 49 <= slab_cap, "conv1_wgrad: slab buffer too small");
  const size_t patch = ((size_t)(2 * C1_RB + 5) * (2 * OW + 6) + 3) & ~(size_t)3;
  const size_t lds = (patch + 4 * 2 * 16 * 64) * sizeof(float);
  VAD_CHECK(lds <= 160 * 1024, "conv1_wgrad: frame too wide for the LDS band");
  hipLaunchKernelGGL(conv1_wgrad_kernel, dim3(S), dim3(256), lds, st, x, H, W, dy, OH, OW, bands, slab);
  VAD_LAUNCH_CHECK();
  hipLaunchKernelGGL(conv1_wgrad_reduce_kernel, dim3((unsigned)cdiv(32 * 49, 64)), dim3(256), 0, st, slab, S, dw);
  VAD_LAUNCH_CHECK();
  return 0;
}

// MaxPool2d(3, 2, 1) backward over relu(bn1(y)): dA[p] = sum of dpool over the (1, 2 or 4) windows whose first
// maximum in scan order (torch CPU max_pool2d's index rule) is p; recomputed from y instead of stored indices.
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ y, const float* __restrict__ stats,
                                                          const float* __restrict__ dpool, int NF, int H, int W,
                                                          int C, int OH, int OW, float* __restrict__ dA) {
  const int nq = C / 4;
  const int64_t total = (int64_t)NF * H * W * nq;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i % nq);
    int64_t p = i / nq;
    const int ix = (int)(p % W);
    p /= W;
    const int iy = (int)(p % H);
    const int img = (int)(p / H);
    const int c = q * 4;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(stats + 2 * C + c);
    const f32x4 sh = *reinterpret_cast<const f32x4*>(stats + 3 * C + c);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int oy0 = max(0, iy / 2), oy1 = min(OH - 1, (iy + 1) / 2);
    const int ox0 = max(0, ix / 2), ox1 = min(OW - 1, (ix + 1) / 2);
    for (int oy = oy0; oy <= oy1; ++oy)
      for (int ox = ox0; ox <= ox1; ++ox) {
        f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int first[4] = {-1, -1, -1, -1};
        for (int dyy = -1; dyy <= 1; ++dyy) {
          const int yy = 2 * oy + dyy;
          if (yy < 0 || yy >= H) continue;
          for (int dxx = -1; dxx <= 1; ++dxx) {
            const int xx = 2 * ox + dxx;
            if (xx < 0 || xx >= W) continue;
            const f32x4 v = *reinterpret_cast<const f32x4*>(y + (((int64_t)img * H + yy) * W + xx) * C + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float z = fmaxf(fmaf(v[e], sc[e], sh[e]), 0.f);
              if (z > best[e]) {
                best[e] = z;
                first[e] = yy * W + xx;
              }
            }
          }
        }
        const f32x4 g = *reinterpret_cast<const f32x4*>(dpool + (((int64_t)img * OH + oy) * OW + ox) * C + c);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (first[e] == iy * W + ix) acc[e] += g[e];
      }
    *reinterpret_cast<f32x4*>(dA + (((int64_t)img * H + iy) * W + ix) * C + c) = acc;
  }
}

int maxpool3s2_bwd(const float* y, const float* stats, const float* dpool, int NF, int H, int W, int C, int OH,
                   int OW, float* dA, hipStream_t st) {
  VAD_CHECK(!g_act_bf16, "stem: the unfused stem keeps fp32 activations");
  VAD_CHECK(OH == (H - 1) / 2 + 1 && OW == (W - 1) / 2 + 1 && C % 4 == 0, "maxpool_bwd: bad dims");
  const int64_t total = (int64_t)NF * H * W * (C / 4);
  const int grid = (int)std::min<int64_t>(cdiv(total, 256), 16384);
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(grid), dim3(256), 0, st, y, stats, dpool, NF, H, W, C, OH, OW, dA);
  VAD_LAUNCH_CHECK();
  return 0;
}

int conv1_fwd(const float* x, int NF, int H, int W, const float* w, const float* b, float* y, int OH, int OW,
              float* partials, int* nparts, hipStream_t st) {
  VAD_CHECK(!g_act_bf16, "stem: the unfused stem keeps fp32 activations");
  VAD_CHECK(OH == (H - 1) / 2 + 1 && OW == (W - 1) / 2 + 1, "conv1: bad output dims");
  const int bands = (int)cdiv(OH, C1_RB);
  const size_t lds = (size_t)(2 * C1_RB + 5) * (2 * OW + 6) * sizeof(float);
  VAD_CHECK(lds <= 160 * 1024, "conv1: frame too wide for the LDS band");
  VAD_KLAUNCH(conv1_kernel, dim3(NF * bands), dim3(256), lds, st, x, H, W, w, b, y, OH, OW, bands, partials);
  VAD_LAUNCH_CHECK();
  *nparts = NF * bands;
  return 0;
}

// =====================================================================================================
// BatchNorm finalize: combine partial sums in double; batch stats, affine folding, running-stat update
// (momentum 0.1, unbiased variance for running_var; nn.BatchNorm2d train semantics).
// =====================================================================================================
template <typename PT>
__global__ __launch_bounds__(256) void bn_finalize_kernel(const PT* __restrict__ partials, int P, int C,
                                                          double count, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* running_mean,
                                                          float* running_var, float momentum, double eps,
                                                          int training, float* __restrict__ stats, int cm) {
  const int c = blockIdx.x;
  double a = 0.0, b = 0.0;
  // partials row-major [P][2C], or column-major [2C][P] (cm: the fused stem's layout, coalesced here)
  const int64_t rs = cm ? 1 : 2 * C, ia = cm ? (int64_t)c * P : c, ib = cm ? (int64_t)(C + c) * P : C + c;
  if (training) {
#pragma unroll 4
    for (int p = threadIdx.x; p < P; p += 256) {
      a += (double)partials[p * rs + ia];
      b += (double)partials[p * rs + ib];
    }
  }
  block_sum2_256(a, b);
  if (threadIdx.x == 0) {
    double mean, var;
    if (training) {
      mean = a / count;
      var = b / count - mean * mean;
      if (var < 0) var = 0;
      running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * mean);
      running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * var * count / (count - 1.0));
    } else {
      mean = running_mean[c];
      var = running_var[c];
    }
    const double invstd = 1.0 / sqrt(var + eps);
    const double scale = (double)gamma[c] * invstd;
    stats[c] = (float)mean;
    stats[C + c] = (float)invstd;
    stats[2 * C + c] = (float)scale;
    stats[3 * C + c] = (float)((double)beta[c] - mean * scale);
  }
}

int bn_finalize(const float* partials, int P, int C, double count, const float* gamma, const float* beta,
                float* running_mean, float* running_var, float momentum, double eps, int training, float* stats,
                hipStream_t st, int cm) {
  hipLaunchKernelGGL(bn_finalize_kernel<float>, dim3(C), dim3(256), 0, st, partials, P, C, count, gamma, beta,
                     running_mean, running_var, momentum, eps, training, stats, cm);
  VAD_LAUNCH_CHECK();
  return 0;
}

int bn_finalize_sums(const double* sums, int C, double count, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, float momentum, double eps, float* stats,
                     hipStream_t st) {
  hipLaunchKernelGGL(bn_finalize_kernel<double>, dim3(C), dim3(256), 0, st, sums, 1, C, count, gamma, beta,
                     running_mean, running_var, momentum, eps, 1, stats, 0);
  VAD_LAUNCH_CHECK();
  return 0;
}

// SyncBatchNorm support: fold a layer's [P][2C] float partials into [2C] double sums (the buffer the caller
// all-reduces across ranks); optionally also writes them as float to a_out / b_out (the local dbeta / dgamma)
__global__ __launch_bounds__(256) void bn_sum_partials_kernel(const float* __restrict__ partials, int P, int C,
                                                              double* __restrict__ sums, float* a_out,
                                                              float* b_out, int cm) {
  const int c = blockIdx.x;
  double a = 0.0, b = 0.0;
  const int64_t rs = cm ? 1 : 2 * C, ia = cm ? (int64_t)c * P : c, ib = cm ? (int64_t)(C + c) * P : C + c;
#pragma unroll 4
  for (int p = threadIdx.x; p < P; p += 256) {
    a += (double)partials[p * rs + ia];
    b += (double)partials[p * rs + ib];
  }
  block_sum2_256(a, b);
  if (threadIdx.x == 0) {
    sums[c] = a;
    sums[C + c] = b;
    if (a_out) a_out[c] = (float)a;
    if (b_out) b_out[c] = (float)b;
  }
}

int bn_sum_partials(const float* partials, int P, int C, double* sums, float* a_out, float* b_out, hipStream_t st,
                    int cm) {
  hipLaunchKernelGGL(bn_sum_partials_kernel, dim3(C), dim3(256), 0, st, partials, P, C, sums, a_out, b_out, cm);
  VAD_LAUNCH_CHECK();
  return 0;
}

// =====================================================================================================
// BatchNorm backward (through the ReLU that follows it):  dZ = dA * [scale*y+shift > 0]
//   reduce: per-channel sum(dZ), sum(dZ*xhat)          -> partials
//   finalize: dgamma = sum(dZ*xhat), dbeta = sum(dZ), k = gamma*invstd, means
//   apply: dY = k * (dZ - mean(dZ) - xhat*mean(dZ*xhat)), plus per-block sum(dY) for the conv bias grad
// Thread layout over [M][C] rows: thread -> (row offset, channel quad); 1024 rows per block.
// =====================================================================================================
// rows per block: 1024, lowered (down to 64) until the grid has >= 1024 blocks.  Callers size partial buffers for
// the worst case ceil(M/64) blocks (CadPlanImpl::carve).
static int bn_rows(int M) {
  int r = 1024;
  while (r > 64 && cdiv(M, r) < 1024) r >>= 1;
  return r;
}

int bn_rows_parts(int M, int C) {
  (void)C;
  return (int)cdiv(M, bn_rows(M));
}

// out: this block's [2C] row (row-major partials), or with cs > 0 element j at out[j * cs] (column-major [2C][P])
__device__ inline void bn_block_reduce_store(float (&v)[2][4], int C, float* out, int64_t cs = 0) {
  // threads sharing a channel quad: tid % (C/4) equal.  Reduce through LDS.
  __shared__ float red[256 * 8];
  const int t = threadIdx.x;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int e = 0; e < 4; ++e) red[(s * 4 + e) * 256 + t] = v[s][e];
  __syncthreads();
  const int nq = C / 4, groups = 256 / nq;
  for (int idx = t; idx < 2 * C; idx += 256) {
    const int s = idx / C, c = idx % C, q = c / 4, e = c % 4;
    float acc = 0.f;
    for (int g = 0; g < groups; ++g) acc += red[(s * 4 + e) * 256 + g * nq + q];
    out[cs ? (int64_t)(s * C + c) * cs : s * C + c] = acc;
  }
}

template <bool AB>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const act_t<AB>* __restrict__ dA,
                                                            const act_t<AB>* __restrict__ y,
                                                            const float* __restrict__ stats, int M, int C,
                                                            float* __restrict__ partials, int BN_ROWS, int cm) {
  const int nq = C / 4, groups = 256 / nq;
  const int q = threadIdx.x % nq, g = threadIdx.x / nq;
  const int c = q * 4;
  const f32x4 mean = *reinterpret_cast<const f32x4*>(stats + c);
  const f32x4 inv = *reinterpret_cast<const f32x4*>(stats + C + c);
  const f32x4 sc = *reinterpret_cast<const f32x4*>(stats + 2 * C + c);
  const f32x4 sh = *reinterpret_cast<const f32x4*>(stats + 3 * C + c);
  float v[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  const int r0 = blockIdx.x * BN_ROWS;
  const int r1 = min(M, r0 + BN_ROWS);
  for (int r = r0 + g; r < r1; r += groups) {
    const f32x4 a = act_f4(act_ld4(dA + (int64_t)r * C + c));
    const f32x4 yy = act_f4(act_ld4(y + (int64_t)r * C + c));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float z = fmaf(yy[e], sc[e], sh[e]);
      const float dz = z > 0.f ? a[e] : 0.f;
      v[0][e] += dz;
      v[1][e] = fmaf(dz, (yy[e] - mean[e]) * inv[e], v[1][e]);
    }
  }
  if (cm) bn_block_reduce_store(v, C, partials + blockIdx.x, gridDim.x);
  else bn_block_reduce_store(v, C, partials + (int64_t)blockIdx.x * 2 * C);
}

int bn_bwd_reduce(const float* dA, const float* y, const float* stats, int M, int C, float* partials, int* nparts,
                  hipStream_t st, int cm) {
  VAD_CHECK(C % 4 == 0 && C <= 1024 && 256 % (C / 4) == 0, "bn_bwd_reduce: unsupported C");
  const int P = bn_rows_parts(M, C);
  if (g_act_bf16)
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<true>, dim3(P), dim3(256), 0, st, reinterpret_cast<const __bf16*>(dA),
                       reinterpret_cast<const __bf16*>(y), stats, M, C, partials, bn_rows(M), cm);
  else
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<false>, dim3(P), dim3(256), 0, st, dA, y, stats, M, C, partials,
                       bn_rows(M), cm);
  VAD_LAUNCH_CHECK();
  *nparts = P;
  return 0;
}

template <typename PT>
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const PT* __restrict__ partials, int P, int C,
                                                              double count, const float* __restrict__ gamma,
                                                              float* __restrict__ stats, float* dgamma,
                                                              float* dbeta, int training, float* dbias, int cm) {
  const int c = blockIdx.x;
  double a = 0.0, b = 0.0;
  // partials row-major [P][2C] or column-major [2C][P] (cm)
  const int64_t rs = cm ? 1 : 2 * C, ia = cm ? (int64_t)c * P : c, ib = cm ? (int64_t)(C + c) * P : C + c;
#pragma unroll 4
  for (int p = threadIdx.x; p < P; p += 256) {
    a += (double)partials[p * rs + ia];
    b += (double)partials[p * rs + ib];
  }
  block_sum2_256(a, b);
  if (threadIdx.x == 0) {
    const double sdz = a, sdzx = b;
    if (dgamma) dgamma[c] = (float)sdzx;
    if (dbeta) dbeta[c] = (float)sdz;
    const double inv = stats[C + c];
    const double k = (double)gamma[c] * inv;
    stats[4 * C + c] = gamma[c] * stats[C + c];
    // eval mode: BN is the affine map of the running stats, no batch-mean terms in its backward
    const double mdz = training ? sdz / count : 0.0, mdzx = training ? sdzx / count : 0.0;
    stats[5 * C + c] = (float)mdz;
    stats[6 * C + c] = (float)mdzx;
    // conv bias grad = sum of dY = k (sum dZ - count mean(dZ)) - k invstd mean(dZ xhat) sum(y - mean); the last
    // sum is zero by the definition of the mean, the first vanishes in training mode up to rounding
    if (dbias) dbias[c] = (float)(k * (sdz - count * mdz));
  }
}

int bn_bwd_finalize(const float* partials, int P, int C, double count, const float* gamma, float* stats,
                    float* dgamma, float* dbeta, int training, hipStream_t st, float* dbias, int cm) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel<float>, dim3(C), dim3(256), 0, st, partials, P, C, count, gamma, stats,
                     dgamma, dbeta, training, dbias, cm);
  VAD_LAUNCH_CHECK();
  return 0;
}

int bn_bwd_finalize_sums(const double* sums, int C, double count, const float* gamma, float* stats, hipStream_t st,
                         float* dbias) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel<double>, dim3(C), dim3(256), 0, st, sums, 1, C, count, gamma, stats,
                     nullptr, nullptr, 1, dbias, 0);
  VAD_LAUNCH_CHECK();
  return 0;
}

// dY = k (dZ - mean(dZ) - xhat mean(dZ xhat)), dZ = dA where relu(fma(y, scale, shift)) > 0.  The body takes plain
// pointers: bn_bwd_apply_kernel adds __restrict__ (distinct buffers), bn_bwd_apply_inplace_kernel does not (the
// training stem's backward applies it in place, dY == dA: every thread reads an element before it writes it)
template <bool AB>
__device__ __forceinline__ void bn_bwd_apply_body(const act_t<AB>* dA, const act_t<AB>* y, const float* stats, int M,
                                                  int C, act_t<AB>* dY, float* bparts, int BN_ROWS) {
  const int nq = C / 4, groups = 256 / nq;
  const int q = threadIdx.x % nq, g = threadIdx.x / nq;
  const int c = q * 4;
  const f32x4 mean = *reinterpret_cast<const f32x4*>(stats + c);
  const f32x4 inv = *reinterpret_cast<const f32x4*>(stats + C + c);
  const f32x4 sc = *reinterpret_cast<const f32x4*>(stats + 2 * C + c);
  const f32x4 sh = *reinterpret_cast<const f32x4*>(stats + 3 * C + c);
  const f32x4 k = *reinterpret_cast<const f32x4*>(stats + 4 * C + c);
  const f32x4 mdz = *reinterpret_cast<const f32x4*>(stats + 5 * C + c);
  const f32x4 mdzx = *reinterpret_cast<const f32x4*>(stats + 6 * C + c);
  float v[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  const int r0 = blockIdx.x * BN_ROWS;
  const int r1 = min(M, r0 + BN_ROWS);
  for (int r = r0 + g; r < r1; r += groups) {
    const f32x4 a = act_f4(act_ld4(dA + (int64_t)r * C + c));
    const f32x4 yy = act_f4(act_ld4(y + (int64_t)r * C + c));
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float z = fmaf(yy[e], sc[e], sh[e]);
      const float dz = z > 0.f ? a[e] : 0.f;
      const float xh = (yy[e] - mean[e]) * inv[e];
      o[e] = k[e] * (dz - mdz[e] - xh * mdzx[e]);
      v[0][e] += o[e];
    }
    act_st4(dY + (int64_t)r * C + c, o);
  }
  if (bparts) bn_block_reduce_store(v, C, bparts + (int64_t)blockIdx.x * 2 * C);
}

template <bool AB>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const act_t<AB>* __restrict__ dA,
                                                           const act_t<AB>* __restrict__ y,
                                                           const float* __restrict__ stats, int M, int C,
                                                           act_t<AB>* __restrict__ dY, float* __restrict__ bparts,
                                                           int BN_ROWS) {
  bn_bwd_apply_body<AB>(dA, y, stats, M, C, dY, bparts, BN_ROWS);
}

__global__ __launch_bounds__(256) void bn_bwd_apply_inplace_kernel(float* dAY, const float* __restrict__ y,
                                                                   const float* __restrict__ stats, int M, int C,
                                                                   int BN_ROWS) {
  bn_bwd_apply_body<false>(dAY, y, stats, M, C, dAY, nullptr, BN_ROWS);
}

typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
struct f32x8v {
  f32x4 lo, hi;
};
__device__ inline void vload8(u32x4v r, float (&v)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[2 * e] = __uint_as_float(r[e] << 16);
    v[2 * e + 1] = __uint_as_float(r[e] & 0xffff0000u);
  }
}
__device__ inline void vload8(const f32x8v& r, float (&v)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = r.lo[e];
    v[4 + e] = r.hi[e];
  }
}
template <typename V>
__device__ inline V vstore8(const float (&v)[8]);
template <>
__device__ inline u32x4v vstore8<u32x4v>(const float (&v)[8]) {
  typedef __bf16 b8 __attribute__((ext_vector_type(8)));
  b8 b;
#pragma unroll
  for (int e = 0; e < 8; ++e) b[e] = (__bf16)v[e];
  return __builtin_bit_cast(u32x4v, b);
}
template <>
__device__ inline f32x8v vstore8<f32x8v>(const float (&v)[8]) {
  f32x8v o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    o.lo[e] = v[e];
    o.hi[e] = v[4 + e];
  }
  return o;
}

int bn_bwd_apply_inplace(float* dAY, const float* y, const float* stats, int M, int C, hipStream_t st) {
  VAD_CHECK(!g_act_bf16, "bn_bwd_apply_inplace: fp32 activations only");
  hipLaunchKernelGGL(bn_bwd_apply_inplace_kernel, dim3(bn_rows_parts(M, C)), dim3(256), 0, st, dAY, y, stats, M, C,
                     bn_rows(M));
  VAD_LAUNCH_CHECK();
  return 0;
}

// Streaming form (no conv-bias partial sums): thread = 8 consecutive channels of a row (16 B per operand in bf16, 32 B in
// fp32), U rows per iteration with every load issued before the arithmetic (the 4-channel row loop above keeps one 8-B
// load per operand in flight per thread and reaches ~3.5 TB/s), grid-stride over the row groups.
template <bool AB, int U>
__global__ __launch_bounds__(256) void bn_bwd_apply_v_kernel(const act_t<AB>* __restrict__ dA,
                                                           const act_t<AB>* __restrict__ y,
                                                           const float* __restrict__ stats, int M, int C,
                                                           act_t<AB>* __restrict__ dY) {
  using V = typename std::conditional<AB, u32x4v, f32x8v>::type;  // 8 channels
  const int tpr = C / 8, rpp = 256 / tpr;                         // threads per row, rows per pass
  const int q = threadIdx.x % tpr, c = q * 8;
  float mean[8], inv[8], sc[8], sh[8], k[8], mdz[8], mdzx[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    mean[e] = stats[c + e];
    inv[e] = stats[C + c + e];
    sc[e] = stats[2 * C + c + e];
    sh[e] = stats[3 * C + c + e];
    k[e] = stats[4 * C + c + e];
    mdz[e] = stats[5 * C + c + e];
    mdzx[e] = stats[6 * C + c + e];
  }
  const int64_t step = (int64_t)gridDim.x * rpp * U;
  for (int64_t r0 = ((int64_t)blockIdx.x * U) * rpp + threadIdx.x / tpr; r0 < M; r0 += step) {
    V a[U], yy[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = min(r0 + (int64_t)u * rpp, (int64_t)M - 1);
      a[u] = *reinterpret_cast<const V*>(dA + r * C + c);
      yy[u] = *reinterpret_cast<const V*>(y + r * C + c);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = r0 + (int64_t)u * rpp;
      if (r >= M) break;
      float af[8], yf[8], o[8];
      vload8(a[u], af);
      vload8(yy[u], yf);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float dz = fmaf(yf[e], sc[e], sh[e]) > 0.f ? af[e] : 0.f;
        const float xh = (yf[e] - mean[e]) * inv[e];
        o[e] = k[e] * (dz - mdz[e] - xh * mdzx[e]);
      }
      *reinterpret_cast<V*>(dY + r * C + c) = vstore8<V>(o);
    }
  }
}

int bn_bwd_apply(const float* dA, const float* y, const float* stats, int M, int C, float* dY, float* bias_partials,
                 int* nparts, hipStream_t st) {
  const int P = bn_rows_parts(M, C);
  if (!bias_partials && C % 8 == 0 && C >= 8 && C <= 2048 && 256 % (C / 8) == 0) {
    const int U = g_bn_apply_u == 8 ? 8 : (g_bn_apply_u == 2 ? 2 : 4);
    const int rpp = 256 / (C / 8);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(M, (int64_t)rpp * U), g_bn_apply_blocks));
#define VAD_BNA(AB, UU, T)                                                                                            \
  hipLaunchKernelGGL((bn_bwd_apply_v_kernel<AB, UU>), dim3(blocks), dim3(256), 0, st, reinterpret_cast<const T*>(dA), \
                     reinterpret_cast<const T*>(y), stats, M, C, reinterpret_cast<T*>(dY))
    if (g_act_bf16) {
      if (U == 8) VAD_BNA(true, 8, __bf16);
      else if (U == 2) VAD_BNA(true, 2, __bf16);
      else VAD_BNA(true, 4, __bf16);
    } else {
      if (U == 8) VAD_BNA(false, 8, float);
      else if (U == 2) VAD_BNA(false, 2, float);
      else VAD_BNA(false, 4, float);
    }
#undef VAD_BNA
    VAD_LAUNCH_CHECK();
    *nparts = 0;
    return 0;
  }
  if (g_act_bf16)
    hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, dim3(P), dim3(256), 0, st, reinterpret_cast<const __bf16*>(dA),
                       reinterpret_cast<const __bf16*>(y), stats, M, C, reinterpret_cast<__bf16*>(dY), bias_partials,
                       bn_rows(M));
  else
    hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, dim3(P), dim3(256), 0, st, dA, y, stats, M, C, dY, bias_partials,
                       bn_rows(M));
  VAD_LAUNCH_CHECK();
  *nparts = P;
  return 0;
}

// =====================================================================================================
// MaxPool 3x3 s2 p1 over relu(bn1(y)) (the frozen stem: forward only).
// =====================================================================================================
__global__ __launch_bounds__(256) void maxpool_kernel(const float* __restrict__ y, const float* __restrict__ stats,
                                                      int NF, int H, int W, int C, float* __restrict__ out, int OH,
                                                      int OW) {
  const int nq = C / 4;
  const int64_t total = (int64_t)NF * OH * OW * nq;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i % nq);
    int64_t p = i / nq;
    const int ox = (int)(p % OW);
    p /= OW;
    const int oy = (int)(p % OH);
    const int img = (int)(p / OH);
    const int c = q * 4;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(stats + 2 * C + c);
    const f32x4 sh = *reinterpret_cast<const f32x4*>(stats + 3 * C + c);
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int dy = -1; dy <= 1; ++dy) {
      const int iy = 2 * oy + dy;
      if (iy < 0 || iy >= H) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int ix = 2 * ox + dx;
        if (ix < 0 || ix >= W) continue;
        const f32x4 v = *reinterpret_cast<const f32x4*>(y + (((int64_t)img * H + iy) * W + ix) * C + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], fmaxf(fmaf(v[e], sc[e], sh[e]), 0.f));
      }
    }
    *reinterpret_cast<f32x4*>(out + (((int64_t)img * OH + oy) * OW + ox) * C + c) = m;
  }
}

int maxpool3s2_bnrelu(const float* y, const float* stats, int NF, int H, int W, int C, float* out, int OH, int OW,
                      hipStream_t st) {
  VAD_CHECK(!g_act_bf16, "stem: the unfused stem keeps fp32 activations");
  VAD_CHECK(OH == (H - 1) / 2 + 1 && OW == (W - 1) / 2 + 1 && C % 4 == 0, "maxpool: bad dims");
  const int64_t total = (int64_t)NF * OH * OW * (C / 4);
  const int grid = (int)std::min<int64_t>(cdiv(total, 256), 8192);
  hipLaunchKernelGGL(maxpool_kernel, dim3(grid), dim3(256), 0, st, y, stats, NF, H, W, C, out, OH, OW);
  VAD_LAUNCH_CHECK();
  return 0;
}

// =====================================================================================================
// AdaptiveAvgPool2d((4,6)) on relu(bn(y)) + flatten (c*24 + i*6 + j) + mean over T, and its backward.
// torch bins: start = floor(i*In/Out), end = ceil((i+1)*In/Out).
// =====================================================================================================
__device__ inline int ap_start(int i, int in, int out) { return (i * in) / out; }
__device__ inline int ap_end(int i, int in, int out) { return ((i + 1) * in + out - 1) / out; }

// AdaptiveAvgPool2d((4, 6)) of relu(bn(y)) and its mean over the clip (cad:560-568) in one pass: thread (clip b, bin
// (i, j), channel c) walks the bin's pixels of the T images in (t, row, column) order -- loads in chunks of 16 from
// clamped addresses, so a chunk costs one memory round trip -- and writes each image's bin mean and the clip mean
// (same summation order as a per-image pass followed by a mean over T)
template <bool AB>
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const act_t<AB>* __restrict__ y,
                                                          const float* __restrict__ stats, int T, int H, int W, int C,
                                                          float* __restrict__ feats, float* __restrict__ pooled) {
  const int b = blockIdx.y, i = blockIdx.z / 6, j = blockIdx.z % 6;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float sc = stats[2 * C + c], sh = stats[3 * C + c];
  const int h0 = ap_start(i, H, 4), h1 = ap_end(i, H, 4), w0 = ap_start(j, W, 6), w1 = ap_end(j, W, 6);
  const int wn = w1 - w0, n = (h1 - h0) * wn, total = T * n;
  const float fn = (float)n;
  const act_t<AB>* yb = y + (int64_t)b * T * H * W * C + c;
  float cur = 0.f, pool = 0.f;
  int curt = 0;
  for (int base = 0; base < total; base += 16) {
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int q = min(base + k, total - 1), t = q / n, p = q - t * n;
      const int hh = h0 + p / wn, ww = w0 + p % wn;
      v[k] = act_ld(yb + (((int64_t)t * H + hh) * W + ww) * C);
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int q = base + k;
      if (q < total) {
        const int t = q / n;
        if (t != curt) {
          const float f = cur / fn;
          feats[((int64_t)b * T + curt) * C * 24 + c * 24 + i * 6 + j] = f;
          pool += f;
          curt = t;
          cur = 0.f;
        }
        cur += fmaxf(fmaf(v[k], sc, sh), 0.f);
      }
    }
  }
  const float f = cur / fn;
  feats[((int64_t)b * T + curt) * C * 24 + c * 24 + i * 6 + j] = f;
  pool += f;
  pooled[(int64_t)b * C * 24 + c * 24 + i * 6 + j] = pool / (float)T;
}

int avgpool_fwd(const float* y, const float* stats, int B, int T, int H, int W, int C, float* feats, float* pooled,
                hipStream_t st) {
  const dim3 grid((unsigned)cdiv(C, 256), B, 24);
  if (g_act_bf16)
    VAD_KLAUNCH(avgpool_fwd_kernel<true>, grid, dim3(256), 0, st, reinterpret_cast<const __bf16*>(y), stats, T, H, W,
                C, feats, pooled);
  else
    VAD_KLAUNCH(avgpool_fwd_kernel<false>, grid, dim3(256), 0, st, y, stats, T, H, W, C, feats, pooled);
  VAD_LAUNCH_CHECK();
  return 0;
}

// one block per (image, output row hh): thread c spreads the bins covering row hh over the W pixels of the row
// (1024 blocks at config 2 instead of one 64-pixel loop per channel over 128 blocks).  coef != null: the clip-mean
// gradient is dpooled[b] + coef[b] dpooled_c[b] (the direct classifier's affine backward, mlp.h DirMidArgs)
template <bool AB>
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const float* __restrict__ dfeat,
                                                          const float* __restrict__ dpooled,
                                                          const float* __restrict__ dpooled_c,
                                                          const float* __restrict__ coef, int B, int T, int H,
                                                          int W, int C, act_t<AB>* __restrict__ dA) {
  const int img = blockIdx.x, hh = blockIdx.y;
  const int b = img / T;
  const float invT = 1.f / (float)T;
  const float cb = coef ? coef[b] : 0.f;
  for (int c = threadIdx.x; c < C; c += 256) {
    float g[4][6];  // (up to 4 row bins cover hh when H < 4)
    int ni = 0, iv[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (hh >= ap_start(i, H, 4) && hh < ap_end(i, H, 4)) iv[ni++] = i;
    for (int q = 0; q < ni; ++q) {
      const int i = iv[q];
      const float hn = (float)(ap_end(i, H, 4) - ap_start(i, H, 4));
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        float v = dfeat ? dfeat[(int64_t)img * C * 24 + c * 24 + i * 6 + j] : 0.f;
        if (dpooled) {
          const int64_t o = (int64_t)b * C * 24 + c * 24 + i * 6 + j;
          v += (coef ? fmaf(cb, dpooled_c[o], dpooled[o]) : dpooled[o]) * invT;
        }
        g[q][j] = v / (hn * (float)(ap_end(j, W, 6) - ap_start(j, W, 6)));
      }
    }
    for (int ww = 0; ww < W; ++ww) {
      float s = 0.f;
      for (int q = 0; q < ni; ++q)
#pragma unroll
        for (int j = 0; j < 6; ++j)
          if (ww >= ap_start(j, W, 6) && ww < ap_end(j, W, 6)) s += g[q][j];
      act_st(dA + (((int64_t)img * H + hh) * W + ww) * C + c, s);
    }
  }
}

int avgpool_bwd(const float* dfeat, const float* dpooled, int B, int T, int H, int W, int C, float* dA,
                hipStream_t st, const float* dpooled_c, const float* coef) {
  VAD_CHECK(!coef || (dpooled && dpooled_c), "avgpool_bwd: the affine form needs both parts");
  const dim3 grid((unsigned)(B * T), (unsigned)H);
  if (g_act_bf16)
    VAD_KLAUNCH(avgpool_bwd_kernel<true>, grid, dim3(256), 0, st, dfeat, dpooled, dpooled_c, coef, B, T, H, W, C,
                reinterpret_cast<__bf16*>(dA));
  else
    VAD_KLAUNCH(avgpool_bwd_kernel<false>, grid, dim3(256), 0, st, dfeat, dpooled, dpooled_c, coef, B, T, H, W, C, dA);
  VAD_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void dense_splitk_reduce_kernel(const float* __restrict__ part, int S, int M, int N,
                                                                  DenseEpiArgs P, const int* skip) {
  if (skip && *skip == 0) return;
  const int64_t total = (int64_t)M * N;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float s = slab_sum(part + i, S, total);
    const int row = (int)(i / N), col = (int)(i % N);
    P.out[(int64_t)row * P.ldc + col] = dense_finish(P, row, col, s);
  }
}

int dense_splitk_reduce(const float* part, int S, int M, int N, const DenseEpiArgs& pe, const int* skip,
                        hipStream_t st) {
  const int64_t total = (int64_t)M * N;
  hipLaunchKernelGGL(dense_splitk_reduce_kernel, dim3((unsigned)std::min<int64_t>(cdiv(total, 256), 1024)), dim3(256),
                     0, st, part, S, M, N, pe, skip);
  VAD_LAUNCH_CHECK();
  return 0;
}

// weight grad of a Linear: part[S][N][K+1] -> dW[N][K], db[N]
__global__ __launch_bounds__(256) void dense_wgrad_reduce_kernel(const float* __restrict__ part, int S, int N, int K,
                                                                 float* __restrict__ dW, float* __restrict__ db,
                                                                 const int* skip) {
  if (skip && *skip == 0) return;
  const int64_t ld = K + 1;
  const int64_t total = (int64_t)N * ld;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float s = slab_sum(part + i, S, total);
    const int row = (int)(i / ld), col = (int)(i % ld);
    if (col < K) dW[(int64_t)row * K + col] = s;
    else if (db) db[row] = s;
  }
}

// =====================================================================================================
// 3x3 convs
// =====================================================================================================
static void fwd_taps(TapTable& t) {
  t.ntaps = 9;
  for (int k = 0; k < 9; ++k) {
    t.dh[k] = (int8_t)(k / 3 - 1);
    t.dw[k] = (int8_t)(k % 3 - 1);
  }
}

// dgrad parity classes.  stride 1: one class, all taps, src offset = 1 - k.  stride 2: class (ph,pw) uses
// taps kh with (ph+1-kh) even, src offset (ph+1-kh)/2.
struct DgradClass {
  int ph, pw, nrt, nct;
  int kh[2], dh[2], kw[2], dw[2];
};
static int dgrad_classes(int stride, DgradClass* cls) {
  if (stride == 1) return 0;
  int n = 0;
  for (int ph = 0; ph < 2; ++ph)
    for (int pw = 0; pw < 2; ++pw) {
      DgradClass c{};
      c.ph = ph; c.pw = pw; c.nrt = c.nct = 0;
      for (int k = 0; k < 3; ++k) {
        if (((ph + 1 - k) & 1) == 0) { c.kh[c.nrt] = k; c.dh[c.nrt] = (ph + 1 - k) / 2; ++c.nrt; }
        if (((pw + 1 - k) & 1) == 0) { c.kw[c.nct] = k; c.dw[c.nct] = (pw + 1 - k) / 2; ++c.nct; }
      }
      cls[n++] = c;
    }
  return n;
}

// dgrad weight images: stride 1 and the stride-2 patch kernel -> Wd[ci][t=kh*3+kw][co]; stride-2 GEMM path -> per
// class, concatenated, Wd_c[ci][ri*nct+cj][co] for taps (kh[ri], kw[cj]).
__global__ void conv3_prep_kernel(const float* __restrict__ w, int Ci, int Co, int classes, float* __restrict__ wf,
                                  float* __restrict__ wd) {
  const int64_t total = (int64_t)Co * Ci * 9;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int t = (int)(i % 9);
    const int ci = (int)((i / 9) % Ci);
    const int co = (int)(i / (9 * Ci));
    const float v = w[i];
    wf[((int64_t)co * 9 + t) * Ci + ci] = v;
    const int kh = t / 3, kw = t % 3;
    if (!classes) {
      wd[((int64_t)ci * 9 + t) * Co + co] = v;
    } else {
      // class (ph,pw): kh valid iff (ph+1-kh) even -> ph = (kh+1)&1; its index among the class's row taps
      const int ph = (kh + 1) & 1, pw = (kw + 1) & 1;
      const int ri = (ph == 0) ? 0 : (kh == 0 ? 0 : 1);
      const int cj = (pw == 0) ? 0 : (kw == 0 ? 0 : 1);
      const int nrt = ph == 0 ? 1 : 2, nct = pw == 0 ? 1 : 2;
      int64_t off = 0;  // classes in order (0,0),(0,1),(1,0),(1,1)
      for (int c = 0; c < ph * 2 + pw; ++c) {
        const int r = (c >> 1) == 0 ? 1 : 2, q = (c & 1) == 0 ? 1 : 2;
        off += (int64_t)r * q * Ci * Co;
      }
      wd[off + ((int64_t)ci * (nrt * nct) + ri * nct + cj) * Co + co] = v;
    }
  }
}

// (PrepTab and conv3_image_store, the one routine that writes a layer's images: weight_images.h)
__global__ void conv3_prep_all_kernel(const PrepTab t) {
  const int64_t total = t.end[t.n - 1];
  for (int64_t g = blockIdx.x * 256ll + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    int l = 0;
    while (g >= t.end[l]) ++l;
    const int64_t i = g - (l ? t.end[l - 1] : 0);
    conv3_image_store(t, l, i, t.w[l][i]);
  }
}

// The one rule for which kernel family a pass of a layer runs on, in order of preference.  The
// launchers switch on it; conv3_path, conv3_act_bf16_ok, conv3_dgrad_w3_wanted and the prep table's classes are read
// off it.  The f32 families take no bf16 activations: under bf16 storage a pass nothing else takes has no kernel.
Conv3Kernel conv3_choose(const Conv3Layer& L, Conv3Pass pass, const char** why) {
  using K = Conv3Kernel;
  const bool f32 = !g_act_bf16;
  const char* no_f32 = nullptr;
  auto none = [&](const char* reason) { if (why) *why = reason; return K::None; };
  switch (pass) {
    case Conv3Pass::Fwd:
      if (bfc_supported(L, true)) return K::BfNative;
      if (L.Ci % 32 != 0) return none("conv3_fwd: Ci must be a multiple of 32");
      no_f32 = "conv3_fwd: bf16 activations need the split kernels";
      // (the patch grid may exceed ceil(M/64) BN partial blocks on tiny images: those stay on the GEMM path)
      if (!g_conv_patch || conv3_patch_blocks(L.NF, L.OH, L.OW) > cdiv((int64_t)L.NF * L.OH * L.OW, 64)) break;
      if (conv3_x3_supported(L, true)) return K::SplitX3;
      if (f32 && conv3_patch_supported(L, true)) return K::PatchF32;
      break;
    case Conv3Pass::Dgrad:
      if (L.Co % 32 != 0) return none("conv3_dgrad: Co must be a multiple of 32");
      if (bfc_supported(L, false)) return K::BfNative;
      no_f32 = "conv3_dgrad: bf16 activations need the split kernels";
      if (!g_conv_patch) break;
      if (conv3_x3_supported(L, false)) return K::SplitX3;
      if (!conv3_patch_supported(L, false)) break;  // (stride 2: the split kernel too)
      if (conv3_x3_dgrad_s2_supported(L)) return K::SplitS2;
      if (f32) return K::PatchF32;
      break;
    case Conv3Pass::Wgrad:
      if (bfc_wgrad_supported(L)) return K::BfNative;
      no_f32 = "conv3_wgrad: bf16 activations need the split kernels";
      if (!g_conv_wgrad_patch) break;
      if (x3_wgrad_tr_supported(L)) return K::SplitTr;
      if (conv3_wgrad_x3_supported(L)) return K::SplitX3;
      if (f32 && conv3_wgrad_patch_supported(L) && (L.stride == 1 || g_conv_wgrad_patch == 2)) return K::PatchF32;
      break;
  }
  return f32 ? K::GemmF32 : none(no_f32);
}

int conv3_prep_table(int n, const float* const* w, const Conv3Layer* L, float* const* wf, float* const* wd,
                     __bf16* const* w3, PrepTab* out) {
  VAD_CHECK(n >= 1 && n <= 8, "conv3_prep_weights_all: 1..8 layers");
  PrepTab t{};
  t.n = n;
  t.bf16 = g_conv_bf16 && g_act_bf16;
  int64_t acc = 0;
  for (int l = 0; l < n; ++l) {
    t.w[l] = w[l];
    t.wf[l] = wf[l];
    t.wd[l] = wd[l];
    t.w3[l] = w3 ? w3[l] : nullptr;
    VAD_CHECK(!t.w3[l] || L[l].Co % 16 == 0, "conv3_prep_weights_all: pre-split Wd needs Co % 16 == 0");
    t.Ci[l] = L[l].Ci;
    t.Co[l] = L[l].Co;
    t.classes[l] = L[l].stride == 2 && conv3_choose(L[l], Conv3Pass::Dgrad) == Conv3Kernel::GemmF32;
    acc += (int64_t)L[l].Co * L[l].Ci * 9;
    t.end[l] = acc;
  }
  *out = t;
  return 0;
}

int conv3_prep_run(const PrepTab& t, hipStream_t st) {
  const int64_t acc = t.end[t.n - 1];
  hipLaunchKernelGGL(conv3_prep_all_kernel, dim3((unsigned)std::min<int64_t>(cdiv(acc, 256), 4096)), dim3(256), 0, st,
                     t);
  VAD_LAUNCH_CHECK();
  return 0;
}

int conv3_prep_weights_all(int n, const float* const* w, const Conv3Layer* L, float* const* wf, float* const* wd,
                           hipStream_t st, __bf16* const* w3) {
  PrepTab t;
  VAD_TRY(conv3_prep_table(n, w, L, wf, wd, w3, &t));
  return conv3_prep_run(t, st);
}

int conv3_prep_weights(const float* w, const Conv3Layer& L, float* wf, float* wd, hipStream_t st) {
  return conv3_prep_weights_all(1, &w, &L, &wf, &wd, st);
}

int conv3_fwd(const Conv3Layer& L, const float* src, const float* src_stats, const float* wf, const float* bias,
              float* y, float* partials, int* nparts, hipStream_t st, int* parts_cm) {
  if (parts_cm) *parts_cm = 0;
  const char* why = nullptr;
  switch (conv3_choose(L, Conv3Pass::Fwd, &why)) {
    case Conv3Kernel::BfNative:  // (config 4): column-major partials
      if (parts_cm) *parts_cm = 1;
      return bfc_fwd(L, reinterpret_cast<const __bf16*>(src), src_stats, conv3_bf16_image(wf, L), bias,
                     reinterpret_cast<__bf16*>(y), partials, conv3_patch_blocks(L.NF, L.OH, L.OW) * 2 * L.Co, nparts,
                     st);
    case Conv3Kernel::SplitX3: return conv3_x3_fwd(L, src, src_stats, wf, bias, y, partials, nparts, st, parts_cm);
    case Conv3Kernel::PatchF32: return conv3_patch_fwd(L, src, src_stats, wf, bias, y, partials, nparts, st);
    case Conv3Kernel::GemmF32: break;
    default: VAD_CHECK(false, why ? why : "conv3: no kernel for this pass");
  }
  ConvGeom g{L.NF, L.OH, L.OW, L.stride, L.stride, L.IH, L.IW, L.Ci};
  TapTable taps;
  fwd_taps(taps);
  const int M = L.NF * L.OH * L.OW, N = L.Co, K = 9 * L.Ci;
  EpiConvFwd::Params pe{y, bias, L.Co, partials};
  const int id = pick_fwd_tile(M, N);
  return with_tile(id, [&](auto cfg) -> int {
    using C = decltype(cfg);
    VAD_CHECK(gather_fits((int64_t)g.imgs * g.SH * g.SW * g.C), "conv gather: source over 2 GB");
    typename ConvGatherKC<C::BM>::Params pa{src, g, taps, src_stats ? src_stats + 2 * L.Ci : nullptr,
                                            src_stats ? src_stats + 3 * L.Ci : nullptr};
    typename DenseKC<C::BN>::Params pb{wf, K, N, K};
    VAD_TRY((launch_gemm<C, ConvGatherKC, DenseKC, EpiConvFwd>(pa, pb, pe, M, N, K, 1, nullptr, st)));
    *nparts = (int)cdiv(M, C::BM);
    return 0;
  });
}

int conv3_dgrad(const Conv3Layer& L, const float* dY, const float* wd, float* dX, hipStream_t st,
                const BnBwdFuse* f, const __bf16* w3) {
  const int N = L.Ci;
  if (f) *f->nparts = 0;
  const char* why = nullptr;
  switch (conv3_choose(L, Conv3Pass::Dgrad, &why)) {
    case Conv3Kernel::BfNative:
      return bfc_dgrad(L, reinterpret_cast<const __bf16*>(dY), conv3_bf16_image(wd, L), reinterpret_cast<__bf16*>(dX),
                       st, f);
    case Conv3Kernel::SplitX3: return conv3_x3_dgrad(L, dY, wd, dX, st, f);
    case Conv3Kernel::SplitS2: return conv3_x3_dgrad_s2(L, dY, wd, dX, st, f, w3);
    case Conv3Kernel::PatchF32: return conv3_patch_dgrad(L, dY, wd, dX, st);
    case Conv3Kernel::GemmF32: break;  // (stride 2: the per-class Wd image, conv3_prep_table)
    default: VAD_CHECK(false, why ? why : "conv3: no kernel for this pass");
  }
  if (L.stride == 1) {
    ConvGeom g{L.NF, L.IH, L.IW, 1, 1, L.OH, L.OW, L.Co};
    TapTable taps;
    taps.ntaps = 9;
    for (int k = 0; k < 9; ++k) {
      taps.dh[k] = (int8_t)(1 - k / 3);
      taps.dw[k] = (int8_t)(1 - k % 3);
    }
    EpiConvDgrad::Params pe{dX, L.IH, L.IW, 1, 0, 1, 0, L.IH, L.IW, L.Ci};
    return dgrad_launch(g, taps, dY, wd, N, pe, st);
  }
  DgradClass cls[4];
  const int nc = dgrad_classes(2, cls);
  int64_t off = 0;
  for (int ci = 0; ci < nc; ++ci) {
    const DgradClass& c = cls[ci];
    const int GA = (L.IH - c.ph + 1) / 2, GB = (L.IW - c.pw + 1) / 2;
    ConvGeom g{L.NF, GA, GB, 1, 1, L.OH, L.OW, L.Co};
    TapTable taps;
    taps.ntaps = c.nrt * c.nct;
    for (int r = 0; r < c.nrt; ++r)
      for (int q = 0; q < c.nct; ++q) {
        taps.dh[r * c.nct + q] = (int8_t)c.dh[r];
        taps.dw[r * c.nct + q] = (int8_t)c.dw[q];
      }
    EpiConvDgrad::Params pe{dX, GA, GB, 2, c.ph, 2, c.pw, L.IH, L.IW, L.Ci};
    VAD_TRY(dgrad_launch(g, taps, dY, wd + off, N, pe, st));
    off += (int64_t)taps.ntaps * L.Ci * L.Co;
  }
  return 0;
}

bool conv3_act_bf16_ok(const Conv3Layer& L, bool dgrad) {
  ActStorage abf(1);  // (under bf16 storage the chooser offers only the families that take it)
  return conv3_choose(L, Conv3Pass::Fwd) != Conv3Kernel::None &&
         (!dgrad || conv3_choose(L, Conv3Pass::Dgrad) != Conv3Kernel::None) &&
         conv3_choose(L, Conv3Pass::Wgrad) != Conv3Kernel::None;
}

bool conv3_dgrad_w3_wanted(const Conv3Layer& L) {
  return g_dgrad_s2_w3 && !g_conv_bf16 && conv3_choose(L, Conv3Pass::Dgrad) == Conv3Kernel::SplitS2;
}

int conv3_path(const Conv3Layer& L, int kind) {
  const Conv3Kernel k = conv3_choose(L, Conv3Pass(kind));
  if (k == Conv3Kernel::BfNative) return 2;
  const bool split = k == Conv3Kernel::SplitX3 || k == Conv3Kernel::SplitS2 || k == Conv3Kernel::SplitTr;
  return split ? (g_conv_bf16 ? 1 : 6) : 0;  // 0: the f32 families (and None: nothing runs)
}

// target grid of a weight gradient nothing else runs beside (the last layer's; 512 / 1024 measured no faster)
constexpr int WGRAD_ALONE_BLOCKS = 448;

int conv3_wgrad(const Conv3Layer& L, const float* dY, const float* src, const float* src_stats, float* partial,
                int* nsplit, int64_t partial_cap, hipStream_t st, bool alone) {
  const char* why = nullptr;
  switch (conv3_choose(L, Conv3Pass::Wgrad, &why)) {
    case Conv3Kernel::BfNative:
      return bfc_wgrad(L, reinterpret_cast<const __bf16*>(dY), reinterpret_cast<const __bf16*>(src), src_stats,
                       partial, nsplit, partial_cap, st);
    case Conv3Kernel::SplitTr:
      return x3_wgrad_tr(L, dY, src, src_stats, partial, nsplit, partial_cap, alone ? WGRAD_ALONE_BLOCKS : 0, st);
    case Conv3Kernel::SplitX3:
      return conv3_wgrad_x3(L, dY, src, src_stats, partial, nsplit, partial_cap,
                            alone ? WGRAD_ALONE_BLOCKS : g_conv_wgrad_patch_blocks, st);
    case Conv3Kernel::PatchF32:
      return conv3_wgrad_patch(L, dY, src, src_stats, partial, nsplit, partial_cap, g_conv_wgrad_patch_blocks, st);
    case Conv3Kernel::GemmF32: break;
    default: VAD_CHECK(false, why ? why : "conv3: no kernel for this pass");
  }
  const int M = L.Co, N = 9 * L.Ci, K = L.NF * L.OH * L.OW;
  return with_tile(pick_wgrad_tile(M, N), [&](auto cfg) -> int {
    using C = decltype(cfg);
    const int tiles = (int)(cdiv(M, C::BM) * cdiv(N, C::BN));
    int splits = (int)std::max<int64_t>(
        1, std::min<int64_t>(cdiv(g_conv_wgrad_blocks, tiles), cdiv(K, (int64_t)g_conv_wgrad_min_ktiles * BK)));
    while ((int64_t)splits * M * N > partial_cap && splits > 1) splits /= 2;
    VAD_CHECK(gather_fits((int64_t)K * L.Co), "dense gather: operand over 2 GB");
    typename DenseKM<C::BM>::Params pa{dY, L.Co, L.Co, K, -1};
    VAD_CHECK(gather_fits((int64_t)L.NF * L.IH * L.IW * L.Ci), "conv patch: source over 2 GB");
    typename ConvPatchKM<C::BN>::Params pb{src, L.NF, L.OH, L.OW, L.stride, 1, L.IH, L.IW, L.Ci, 3, N,
                                           src_stats ? src_stats + 2 * L.Ci : nullptr,
                                           src_stats ? src_stats + 3 * L.Ci : nullptr};
    EpiPartial::Params pe{partial, N};
    return launch_gemm<C, DenseKM, ConvPatchKM, EpiPartial>(pa, pb, pe, M, N, K, splits, nullptr, st, nsplit);
  });
}

// Split-K slab reduction of the conv weight gradient.  Block = 256/SL float4 columns x SL split lanes; lane sl sums
// slabs sl, sl + SL, ... in order with 8 loads in flight (unconditional, from clamped slab indices), and the SL lanes
// of a column are combined through LDS in a fixed order.  SL = the smallest of 1, 2, 4, 8, 16 that leaves each lane
// <= 16 slabs (the wide layers have 12-48 slabs: one lane per column reads them all; the 32-channel layers up to
// 512: 16 lanes) -- a fixed function of S, so the summation order is fixed per layer.  Slab layout [S][co][t*Ci + ci];
// dW is torch [co][ci][kh][kw].  Extra blocks after the first wblocks reduce the conv bias (one block per channel).
template <int SL>
__global__ __launch_bounds__(256) void conv3_wgrad_reduce_kernel(const float* __restrict__ part, int S, int Co, int Ci,
                                                                 const float* __restrict__ bparts, int NB,
                                                                 float* __restrict__ dW, float* __restrict__ db,
                                                                 int wblocks) {
  constexpr int NCOL = 256 / SL;
  __shared__ f32x4 red[SL > 1 ? SL : 1][NCOL + 1];
  const int64_t ldp = 9 * Ci;
  const int64_t total = (int64_t)Co * ldp;
  if ((int)blockIdx.x >= wblocks) {  // conv bias: one block per channel, 256-way strided sum + tree
    const int c = blockIdx.x - wblocks;
    float s = 0.f;
    for (int p = threadIdx.x; p < NB; p += 256) s += bparts[(int64_t)p * 2 * Co + c];
    s = wave_sum(s);
    __shared__ float r0[4];
    if ((threadIdx.x & 63) == 0) r0[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) db[c] = (r0[0] + r0[1]) + (r0[2] + r0[3]);
    return;
  }
  const int e = threadIdx.x % NCOL, sl = threadIdx.x / NCOL;
  const int64_t i = ((int64_t)blockIdx.x * NCOL + e) * 4;  // total % 4 == 0 (Ci % 4 == 0)
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f};
  if (i < total) {
    const int n = S > sl ? (S - sl + SL - 1) / SL : 0;
    for (int k0 = 0; k0 < n; k0 += 8) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = *reinterpret_cast<const f32x4*>(part + (int64_t)(sl + SL * min(k0 + u, n - 1)) * total + i);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k0 + u < n) a0 += v[u];
    }
  }
  f32x4 s = a0;
  if constexpr (SL > 1) {
    red[sl][e] = a0;
    __syncthreads();
    if (sl != 0) return;
    // pairwise tree over the SL lanes, fixed order
    f32x4 q[SL];
#pragma unroll
    for (int u = 0; u < SL; ++u) q[u] = red[u][e];
#pragma unroll
    for (int w = 1; w < SL; w <<= 1)
#pragma unroll
      for (int u = 0; u < SL; u += 2 * w) q[u] += q[u + w];
    s = q[0];
  }
  if (i < total) {
    const int64_t co = i / ldp, r = i - co * ldp;
    const int t = (int)(r / Ci), ci = (int)(r - (int64_t)t * Ci);
#pragma unroll
    for (int u = 0; u < 4; ++u) dW[(co * Ci + ci + u) * 9 + t] = s[u];
  }
}

int conv3_wgrad_reduce(const Conv3Layer& L, const float* partial, int nsplit, const float* bias_partials,
                       int nbias_parts, float* dW, float* db, hipStream_t st) {
  const int64_t total = (int64_t)L.Co * L.Ci * 9;
  VAD_CHECK(L.Ci % 4 == 0, "conv3_wgrad_reduce: Ci % 4");
  int sl = 1;
  while (sl < 16 && cdiv(nsplit, sl) > 16) sl *= 2;
  const int wblocks = (int)cdiv(total, 4 * (256 / sl));
  const int bblocks = db ? L.Co : 0;
  const dim3 grid((unsigned)(wblocks + bblocks));
  switch (sl) {
    case 1: VAD_KLAUNCH(conv3_wgrad_reduce_kernel<1>, grid, dim3(256), 0, st, partial, nsplit, L.Co, L.Ci, bias_partials, nbias_parts, dW, db, wblocks); break;
    case 2: VAD_KLAUNCH(conv3_wgrad_reduce_kernel<2>, grid, dim3(256), 0, st, partial, nsplit, L.Co, L.Ci, bias_partials, nbias_parts, dW, db, wblocks); break;
    case 4: VAD_KLAUNCH(conv3_wgrad_reduce_kernel<4>, grid, dim3(256), 0, st, partial, nsplit, L.Co, L.Ci, bias_partials, nbias_parts, dW, db, wblocks); break;
    case 8: VAD_KLAUNCH(conv3_wgrad_reduce_kernel<8>, grid, dim3(256), 0, st, partial, nsplit, L.Co, L.Ci, bias_partials, nbias_parts, dW, db, wblocks); break;
    default: VAD_KLAUNCH(conv3_wgrad_reduce_kernel<16>, grid, dim3(256), 0, st, partial, nsplit, L.Co, L.Ci, bias_partials, nbias_parts, dW, db, wblocks); break;
  }
  VAD_LAUNCH_CHECK();
  return 0;
}

// =====================================================================================================
// dense layers
// =====================================================================================================
// Few-row layers (M <= 16: the direct classifier runs on the B clips of a rank, cad:568-570) are bound by the weight
// read and by launch latency, not by FLOPs: they use row-streaming kernels instead of the MFMA GEMM tiles, whose K
// loop over 64-row tiles would leave most of the chip idle.
constexpr int kSkinnyRows = 16;
static bool skinny_ok(int M, int K) { return M >= 1 && M <= kSkinnyRows && K % 4 == 0; }

// Y[m][n] = finish(sum_k X[m][k] W[n][k]): a block owns 4 output columns; its 512 threads stride over K in float4
// steps (coalesced W rows, X from L2) with the loads of up to 4 steps in flight, then the 4*MR partial sums are
// combined through LDS in a fixed order.
template <int MR>
__global__ __launch_bounds__(512) void skinny_fwd_kernel(const float* __restrict__ X, int M, int K,
                                                         const float* __restrict__ W, int N, DenseEpiArgs P) {
  constexpr int NT = 512, NO = 4 * MR, G = NT / NO, U = 4;
  __shared__ float red[NT][NO + 1];
  const int tid = threadIdx.x, n0 = blockIdx.x * 4, K4 = K / 4;
  float acc[4][MR];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[c][m] = 0.f;
  // (all loads unconditional from clamped addresses, out-of-range terms zeroed afterwards: a predicated load makes the
  // compiler wait for the previous one, i.e. one memory round trip per load)
  for (int kb = 0; kb < K4; kb += NT * U) {
    f32x4 w[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k4 = min(kb + u * NT + tid, K4 - 1);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        w[u][c] = *reinterpret_cast<const f32x4*>(W + (int64_t)min(n0 + c, N - 1) * K + 4 * k4);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k4 = kb + u * NT + tid;
      if (k4 >= K4) break;
      f32x4 xv[MR];
#pragma unroll
      for (int m = 0; m < MR; ++m) xv[m] = *reinterpret_cast<const f32x4*>(X + (int64_t)min(m, M - 1) * K + 4 * k4);
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const f32x4 x = m < M ? xv[m] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[c][m] = fmaf(x[3], w[u][c][3], fmaf(x[2], w[u][c][2], fmaf(x[1], w[u][c][1], fmaf(x[0], w[u][c][0], acc[c][m]))));
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int m = 0; m < MR; ++m) red[tid][c * MR + m] = acc[c][m];
  __syncthreads();
  const int o = tid / G, part = tid % G;
  float v = 0.f;
  for (int r = part; r < NT; r += G) v += red[r][o];
#pragma unroll
  for (int off = 1; off < G; off <<= 1) v += __shfl_xor(v, off, 64);
  const int c = o / MR, m = o % MR;
  if (part == 0 && m < M && n0 + c < N) P.out[(int64_t)m * P.ldc + n0 + c] = dense_finish(P, m, n0 + c, v);
}

// dX[m][k] = gate(sum_n dY[m][n] W[n][k]): a block owns 64 consecutive k (one per lane), its 16 waves split N (up to 32
// W loads in flight per lane); dY is staged in LDS as [n][MR] (broadcast reads), the waves are combined in a fixed order
// (wave q + wave q + 8, then the 8 pair sums in order: an 8-wave combine buffer, so 16 rows fit N <= 512 in 64 KB).
template <int MR>
__global__ __launch_bounds__(1024) void skinny_dgrad_kernel(const float* __restrict__ dY, int M, int N,
                                                            const float* __restrict__ W, int K, DenseEpiArgs P,
                                                            const int* skip) {
  if (skip && *skip == 0) return;
  constexpr int NW = 16, U = 32;  // (a wave's whole n range in one batch of loads when N <= 512)
  extern __shared__ __attribute__((aligned(16))) float dsm[];  // [N][MR] then [NW / 2][MR][64]
  float* dys = dsm;
  float* red = dsm + (int64_t)N * MR;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i0 = 0; i0 < N * MR; i0 += 4 * 64 * NW) {  // 4 clamped loads in flight per thread, zeroed after
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = min(i0 + u * 64 * NW + tid, N * MR - 1), n = i / MR, m = i % MR;
      v[u] = dY[(int64_t)min(m, M - 1) * N + n];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * 64 * NW + tid;
      if (i < N * MR) dys[i] = i % MR < M ? v[u] : 0.f;
    }
  }
  __syncthreads();
  const int k = blockIdx.x * 64 + lane;
  const int nq = (N + NW - 1) / NW, nb = wave * nq, ne = min(N, nb + nq);
  float acc[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) acc[m] = 0.f;
  if (k < K) {
    for (int n0 = nb; n0 < ne; n0 += U) {
      float w[U];
#pragma unroll
      for (int u = 0; u < U; ++u) w[u] = W[(int64_t)min(n0 + u, ne - 1) * K + k];  // (clamped: see skinny_fwd)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (n0 + u >= ne) break;
#pragma unroll
        for (int m4 = 0; m4 < MR; m4 += 4) {
          const f32x4 d = *reinterpret_cast<const f32x4*>(dys + (n0 + u) * MR + m4);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[m4 + e] = fmaf(d[e], w[u], acc[m4 + e]);
        }
      }
    }
  }
  if (wave >= NW / 2) {
#pragma unroll
    for (int m = 0; m < MR; ++m) red[((wave - NW / 2) * MR + m) * 64 + lane] = acc[m];
  }
  __syncthreads();
  if (wave < NW / 2) {
#pragma unroll
    for (int m = 0; m < MR; ++m) red[(wave * MR + m) * 64 + lane] += acc[m];
  }
  __syncthreads();
  if (wave == 0 && k < K) {
    for (int m = 0; m < M; ++m) {
      float v = 0.f;
#pragma unroll
      for (int q = 0; q < NW / 2; ++q) v += red[(q * MR + m) * 64 + lane];
      P.out[(int64_t)m * P.ldc + k] = dense_finish(P, m, k, v);
    }
  }
}

// dW[n][k] = sum_m dY[m][n] X[m][k] (written), db[n] = sum_m dY[m][n]: a thread owns 4 columns n x one float4 of k.
__global__ __launch_bounds__(256) void skinny_wgrad_kernel(const float* __restrict__ dY, int M, int N,
                                                           const float* __restrict__ X, int K, float* __restrict__ dW,
                                                           float* __restrict__ db, const int* skip) {
  if (skip && *skip == 0) return;
  const int k4 = blockIdx.x * 256 + threadIdx.x, n0 = blockIdx.y * 4;
  if (db && blockIdx.x == 0 && threadIdx.x < 4 && n0 + (int)threadIdx.x < N) {
    float s = 0.f;
    for (int m = 0; m < M; ++m) s += dY[(int64_t)m * N + n0 + threadIdx.x];
    db[n0 + threadIdx.x] = s;
  }
  if (k4 >= K / 4) return;
  f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int m = 0; m < M; ++m) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(X + (int64_t)m * K + 4 * k4);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float d = n0 + c < N ? dY[(int64_t)m * N + n0 + c] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[c][e] = fmaf(d, x[e], acc[c][e]);
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (n0 + c < N) *reinterpret_cast<f32x4*>(dW + (int64_t)(n0 + c) * K + 4 * k4) = acc[c];
}

int dense_fwd(const float* X, int M, int K, const float* W, const float* b, int N, float* Y, const DenseAct& act,
              float* scratch, int64_t scratch_floats, hipStream_t st, int max_splits) {
  using C = T64x64;
  DenseEpiArgs pe{Y, N, b, act.relu, act.drop, act.h1, act.thr, act.dscale, act.row0, nullptr, 1.f};
  if (skinny_ok(M, K)) {
    const dim3 grid((unsigned)cdiv(N, 4));
    if (M <= 8) VAD_KLAUNCH(skinny_fwd_kernel<8>, grid, dim3(512), 0, st, X, M, K, W, N, pe);
    else VAD_KLAUNCH(skinny_fwd_kernel<16>, grid, dim3(512), 0, st, X, M, K, W, N, pe);
    VAD_LAUNCH_CHECK();
    return 0;
  }
  DenseKC<C::BM>::Params pa{X, K, M, K};
  DenseKC<C::BN>::Params pb{W, K, N, K};
  const int tiles = (int)(cdiv(M, C::BM) * cdiv(N, C::BN));
  int splits = (int)std::min<int64_t>(cdiv(256, tiles), cdiv(K, 4 * BK));
  if (max_splits > 0) splits = std::min(splits, max_splits);
  while (splits > 1 && (int64_t)splits * M * N > scratch_floats) splits /= 2;
  if (splits <= 1) return launch_gemm<C, DenseKC, DenseKC, EpiDense>(pa, pb, pe, M, N, K, 1, nullptr, st);
  EpiPartial::Params pp{scratch, N};
  int used = 1;
  VAD_TRY((launch_gemm<C, DenseKC, DenseKC, EpiPartial>(pa, pb, pp, M, N, K, splits, nullptr, st, &used)));
  return dense_splitk_reduce(scratch, used, M, N, pe, nullptr, st);
}

int dense_fwd_splitk(const float* X, int M, int K, const float* W, int N, float* scratch, int64_t scratch_floats,
                     int* nsplit, hipStream_t st) {
  using C = T64x64;
  DenseKC<C::BM>::Params pa{X, K, M, K};
  DenseKC<C::BN>::Params pb{W, K, N, K};
  const int tiles = (int)(cdiv(M, C::BM) * cdiv(N, C::BN));
  int splits = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(256, tiles), cdiv(K, 4 * BK)));
  while (splits > 1 && (int64_t)splits * M * N > scratch_floats) splits /= 2;
  VAD_CHECK((int64_t)M * N <= scratch_floats, "dense_fwd_splitk: scratch too small");
  EpiPartial::Params pp{scratch, N};
  return launch_gemm<C, DenseKC, DenseKC, EpiPartial>(pa, pb, pp, M, N, K, splits, nullptr, st, nsplit);
}

int dense_dgrad(const float* dY, int M, int N, const float* W, int K, float* dX, const float* gate, float gscale,
                const int* skip, hipStream_t st, int gate_rows, float* scratch, int64_t scratch_floats) {
  // dX[m][k] = sum_n dY[m][n] W[n][k]: A = dY (KC over n), B(row k, red n) = W[n][k] (KM, ld K)
  using C = T64x64;
  DenseEpiArgs pe{dX, K, nullptr, 0, 0, 0, 0, 1.f, 0, gate, gscale, gate_rows};
  if (skinny_ok(M, N) && (int64_t)(N + 512) * (M <= 8 ? 8 : 16) * 4 <= 65536) {  // dY + combine buffer in LDS
    const dim3 grid((unsigned)cdiv(K, 64));
    if (M <= 8)
      VAD_KLAUNCH(skinny_dgrad_kernel<8>, grid, dim3(1024), sizeof(float) * (N * 8 + 8 * 8 * 64), st, dY, M, N,
                         W, K, pe, skip);
    else
      VAD_KLAUNCH(skinny_dgrad_kernel<16>, grid, dim3(1024), sizeof(float) * (N * 16 + 8 * 16 * 64), st, dY, M,
                         N, W, K, pe, skip);
    VAD_LAUNCH_CHECK();
    return 0;
  }
  DenseKC<C::BM>::Params pa{dY, N, M, N};
  VAD_CHECK(gather_fits((int64_t)N * K), "dense gather: operand over 2 GB");
  DenseKM<C::BN>::Params pb{W, K, K, N, -1};
  // few output tiles and a long reduction (e.g. cad1's Linear(64, 2048) input gradient: one tile, N = 2048): split-K
  // slabs in scratch when the caller gives one, summed in order with the gate by dense_splitk_reduce
  const int64_t tiles = cdiv(M, C::BM) * cdiv(K, C::BN);
  if (scratch && tiles < 64 && N >= 8 * BK) {
    int splits = (int)std::min<int64_t>(cdiv(256, tiles), N / (4 * BK));
    while (splits > 1 && (int64_t)splits * M * K > scratch_floats) splits /= 2;
    if (splits > 1) {
      int used = 1;
      EpiPartial::Params pp{scratch, K};
      VAD_TRY((launch_gemm<C, DenseKC, DenseKM, EpiPartial>(pa, pb, pp, M, K, N, splits, skip, st, &used)));
      return dense_splitk_reduce(scratch, used, M, K, pe, skip, st);
    }
  }
  return launch_gemm<C, DenseKC, DenseKM, EpiDense>(pa, pb, pe, M, K, N, 1, skip, st);
}

int dense_wgrad(const float* dY, int M, int N, const float* X, int K, float* dW, float* db, float* scratch,
                int64_t scratch_floats, const int* skip, hipStream_t st, int target_blocks) {
  // GEMM rows = out feature n, cols = in feature k (+ ones column for the bias), reduction over m
  using C = T64x64;
  if (skinny_ok(M, K)) {
    hipLaunchKernelGGL(skinny_wgrad_kernel, dim3((unsigned)cdiv(K / 4, 256), (unsigned)cdiv(N, 4)), dim3(256), 0, st, dY,
                       M, N, X, K, dW, db, skip);
    VAD_LAUNCH_CHECK();
    return 0;
  }
  const int GN = K + 1;
  VAD_CHECK(gather_fits((int64_t)M * N) && gather_fits((int64_t)M * K), "dense gather: operand over 2 GB");
  DenseKM<C::BM>::Params pa{dY, N, N, M, -1};
  DenseKM<C::BN>::Params pb{X, K, K, M, K};
  const int tiles = (int)(cdiv(N, C::BM) * cdiv(GN, C::BN));
  int splits = (int)std::min<int64_t>(std::max<int64_t>(1, cdiv(target_blocks, tiles)), cdiv(M, 4 * BK));
  while (splits > 1 && (int64_t)splits * N * GN > scratch_floats) splits /= 2;
  VAD_CHECK((int64_t)N * GN <= scratch_floats, "dense_wgrad: scratch too small");
  EpiPartial::Params pp{scratch, GN};
  int used = 1;
  VAD_TRY((launch_gemm<C, DenseKM, DenseKM, EpiPartial>(pa, pb, pp, N, GN, M, splits, skip, st, &used)));
  const int64_t total = (int64_t)N * GN;
  hipLaunchKernelGGL(dense_wgrad_reduce_kernel, dim3((unsigned)std::min<int64_t>(cdiv(total, 256), 2048)), dim3(256),
                     0, st, scratch, used, N, K, dW, db, skip);
  VAD_LAUNCH_CHECK();
  return 0;
}

}  // namespace vad
