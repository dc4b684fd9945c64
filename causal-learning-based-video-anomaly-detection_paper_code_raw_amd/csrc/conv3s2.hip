// a2's Conv3d(3, stride 2, padding 1) family for gfx950 as implicit GEMMs on f32 MFMA (gemm.h), and the column sums of
// a2's bias gradients.
#include "gemm_launch.h"

namespace vad {

// =====================================================================================================
// Conv3d(kernel 3, stride 2, padding 1) as implicit GEMMs over NDHWC volumes (a2's conv3d_2 / conv3d_3,
// avenue_training_script2.py:20-21): no im2col / col2im columns.
//   conv3s2_fwd    out[p][n] = act(sum_{tap, c} src[2a - 1 + kd][2b - 1 + kh][2c - 1 + kw][c] wk[n][tap C + c] + bias)
//   conv3s2_dgrad  the input gradient as 8 parity-class GEMMs over dY: along each dim an even input index takes k = 1
//                  (dY index = its half), an odd one k = 0 (half + 1) and k = 2 (half); scattered to (2a + pd, ...)
//   conv3s2_wgrad  split-K correlation dY x patch3(src) into slabs, summed into torch's [Co][Ci][27] layout
// Weight images (conv3s2_prep) of torch [Co][Ci][27]: wk [Co][27 Ci]; wc = the 8 class images [Ci][nt Co] back to back
// (class cls = 4 pd + 2 ph + pw, nt = its tap count 1 / 2 / 4 / 8, taps d-major over the per-dim lists).
// =====================================================================================================

__global__ __launch_bounds__(256) void conv3s2_prep_kernel(const float* __restrict__ w, int Co, int Ci,
                                                           float* __restrict__ wk, float* __restrict__ wc) {
  const int64_t total = (int64_t)Co * Ci * 27;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    conv3s2_prep_elem(w, Co, Ci, wk, wc, i);
}

int conv3s2_prep(const float* w, int Co, int Ci, float* wk, float* wc, hipStream_t st) {
  const int64_t total = (int64_t)Co * Ci * 27;
  hipLaunchKernelGGL(conv3s2_prep_kernel, dim3((unsigned)std::min<int64_t>(cdiv(total, 256), 1024)), dim3(256), 0, st,
                     w, Co, Ci, wk, wc);
  VAD_LAUNCH_CHECK();
  return 0;
}

constexpr int CONV3S2_FWD_BLOCKS = 512;  // split K until the grid reaches this many blocks
int conv3s2_fwd(const float* src, int NF, int D, int H, int W, int C, const float* wk, const float* bias, int N,
                int relu, float* out, hipStream_t st, float* scratch, int64_t scratch_floats) {
  VAD_CHECK(C % 4 == 0 && N >= 1, "conv3s2_fwd: C % 4 == 0");
  const int OD = (D - 1) / 2 + 1, OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  ConvGeom3 g{NF, OD, OH, OW, 2, 2, 2, D, H, W, C};
  TapTable3 taps;
  taps.ntaps = 27;
  for (int t = 0; t < 27; ++t) {
    taps.dd[t] = (int8_t)(t / 9 - 1);
    taps.dh[t] = (int8_t)((t / 3) % 3 - 1);
    taps.dw[t] = (int8_t)(t % 3 - 1);
  }
  const int M = NF * OD * OH * OW, K = 27 * C;
  const DenseEpiArgs pe{out, N, bias, relu, 0, 0, 0, 1.f, 0, nullptr, 1.f};
  return with_tile(pick_fwd_tile(M, N), [&](auto cfg) -> int {
    using Cf = decltype(cfg);
    VAD_CHECK(gather_fits((int64_t)g.imgs * g.SD * g.SH * g.SW * g.C), "conv gather: source over 2 GB");
    typename ConvGather3KC<Cf::BM>::Params pa{src, g, taps};
    typename DenseKC<Cf::BN>::Params pb{wk, K, N, K};
    // (conv3d_3 at B = 32: 64 output tiles of 27 K slices each -- split K four ways, slabs summed in order by
    // dense_splitk_reduce, which applies the bias and the ReLU)
    const int tiles = (int)(cdiv(M, Cf::BM) * cdiv(N, Cf::BN));
    int splits = (int)std::min<int64_t>(cdiv(CONV3S2_FWD_BLOCKS, tiles), cdiv(K, 4 * BK));
    while (splits > 1 && (int64_t)splits * M * N > scratch_floats) splits /= 2;
    if (!scratch || splits <= 1) return launch_gemm<Cf, ConvGather3KC, DenseKC, EpiDense>(pa, pb, pe, M, N, K, 1, nullptr, st);
    EpiPartial::Params pp{scratch, N};
    int used = 1;
    VAD_TRY((launch_gemm<Cf, ConvGather3KC, DenseKC, EpiPartial>(pa, pb, pp, M, N, K, splits, nullptr, st, &used)));
    return dense_splitk_reduce(scratch, used, M, N, pe, nullptr, st);
  });
}

int conv3s2_dgrad(const float* dy, int NF, int Co, const float* wc, int Ci, float* dx, int D, int H, int W,
                  hipStream_t st, const float* gate) {
  VAD_CHECK(Co % 4 == 0, "conv3s2_dgrad: Co % 4 == 0");
  const int OD = (D - 1) / 2 + 1, OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  // the 8 parity classes in one launch (blockIdx.z = 7 - class: the 8-tap class first, the 1-tap class last, so the
  // longest blocks are dispatched first; each block's K loop stops at its class's own taps x Co)
  Conv3ClsGeom g{};
  g.imgs = NF; g.SD = OD; g.SH = OH; g.SW = OW; g.C = Co;
  typename DenseKCz<64>::Params pb0{};
  EpiConv3DgradCls::Params pe{};
  pe.dst = dx; pe.imgs = NF; pe.DD = D; pe.DH = H; pe.DW = W; pe.C = Ci; pe.gate = gate; pe.rev = 1;
  int64_t off = 0;
  int Mmax = 0;
  for (int cls = 0; cls < 8; ++cls) {
    const int pd = (cls >> 2) & 1, ph = (cls >> 1) & 1, pw = cls & 1, nt = c3_nt(cls), z = 7 - cls;
    g.GD[z] = pe.GD[z] = std::max(0, (D - pd + 1) / 2);
    g.GA[z] = pe.GA[z] = std::max(0, (H - ph + 1) / 2);
    g.GB[z] = pe.GB[z] = std::max(0, (W - pw + 1) / 2);
    Mmax = std::max(Mmax, NF * g.GD[z] * g.GA[z] * g.GB[z]);
    TapTable3& taps = g.taps[z];
    taps.ntaps = nt;
    const int nh = 1 + ph, nw = 1 + pw;
    for (int t = 0; t < nt; ++t) {
      const int id = t / (nh * nw), ih = (t / nw) % nh, iw = t % nw;
      // even parity: k = 1, offset 0; odd: k = 0 -> offset +1, k = 2 -> offset 0
      taps.dd[t] = (int8_t)(pd == 0 ? 0 : (id == 0 ? 1 : 0));
      taps.dh[t] = (int8_t)(ph == 0 ? 0 : (ih == 0 ? 1 : 0));
      taps.dw[t] = (int8_t)(pw == 0 ? 0 : (iw == 0 ? 1 : 0));
    }
    pb0.off[z] = off;
    pb0.kdim[z] = nt * Co;
    off += (int64_t)nt * Ci * Co;
  }
  if (Mmax == 0) return 0;
  const int K = 8 * Co;
  return with_tile(pick_dgrad_tile(Mmax, Ci), [&](auto cfg) -> int {
    using Cf = decltype(cfg);
    VAD_CHECK(gather_fits((int64_t)g.imgs * g.SD * g.SH * g.SW * g.C), "conv gather: source over 2 GB");
    typename ConvGather3ClsKC<Cf::BM>::Params pa{dy, g};
    typename DenseKCz<Cf::BN>::Params pb{wc, {}, {}, Ci};
    for (int c = 0; c < 8; ++c) {
      pb.off[c] = pb0.off[c];
      pb.kdim[c] = pb0.kdim[c];
    }
    const dim3 grid((unsigned)cdiv(Mmax, Cf::BM), (unsigned)cdiv(Ci, Cf::BN), 8u);
    VAD_KLAUNCH((gemm_kernel<Cf, ConvGather3ClsKC<Cf::BM>, DenseKCz<Cf::BN>, EpiConv3DgradCls>), grid, dim3(256), 0, st,
                pa, pb, pe, Mmax, Ci, K, -1, nullptr);
    VAD_LAUNCH_CHECK();
    return 0;
  });
}

int conv3s2_wgrad(const float* dy, int Co, const float* src, int Ci, int NF, int D, int H, int W, float* dW,
                  float* part, int64_t part_cap, int target_blocks, hipStream_t st, float* db) {
  VAD_CHECK(Ci % 4 == 0 && Co % 4 == 0, "conv3s2_wgrad: channel counts % 4 == 0");
  const int OD = (D - 1) / 2 + 1, OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  // (db: the bias gradient = dY's column sums, as one more GEMM column of ones beside the 27 Ci patch columns)
  const int M = Co, N = 27 * Ci + (db ? 1 : 0), K = NF * OD * OH * OW;
  VAD_CHECK((int64_t)M * N <= part_cap, "conv3s2_wgrad: slab too small");
  int used = 1;
  VAD_TRY(with_tile(pick_wgrad_tile(M, N), [&](auto cfg) -> int {
    using Cf = decltype(cfg);
    const int tiles = (int)(cdiv(M, Cf::BM) * cdiv(N, Cf::BN));
    int splits = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(target_blocks, tiles), cdiv(K, 8 * BK)));
    while ((int64_t)splits * M * N > part_cap && splits > 1) splits /= 2;
    VAD_CHECK(gather_fits((int64_t)K * Co), "dense gather: operand over 2 GB");
    typename DenseKM<Cf::BM>::Params pa{dy, Co, Co, K, -1};
    VAD_CHECK(gather_fits((int64_t)NF * D * H * W * Ci), "conv patch: source over 2 GB");
    typename ConvPatch3KM<Cf::BN>::Params pb{src, NF, OD, OH, OW, 2, 2, 2, 1, D, H, W, Ci, 27 * Ci, db ? 1 : 0};
    const EpiPartial::Params pe{part, N};
    return launch_gemm<Cf, DenseKM, ConvPatch3KM, EpiPartial>(pa, pb, pe, M, N, K, splits, nullptr, st, &used);
  }));
  return taps_wgrad_reduce(part, used, Co, Ci, 27, dW, st, N, db);
}

// db[n] = sum over the M rows of x[m][n], fixed order, two passes: block b sums the rows of its contiguous range with
// 256 / N row lanes per column (coalesced rows), lanes combined by a fixed tree -> part[b][n]; then one block adds the
// block sums in order (double).  N divides 256.
__global__ __launch_bounds__(256) void col_sum_part_kernel(const float* __restrict__ x, int64_t M, int N, int64_t rows,
                                                           double* __restrict__ part) {
  __shared__ double red[256];
  const int n = threadIdx.x % N, lane = threadIdx.x / N, lanes = 256 / N;
  const int64_t r0 = (int64_t)blockIdx.x * rows, r1 = min(M, r0 + rows);
  double s = 0.0;
#pragma unroll 4
  for (int64_t m = r0 + lane; m < r1; m += lanes) s += (double)x[m * N + n];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = lanes / 2; o > 0; o >>= 1) {
    if (lane < o) red[threadIdx.x] += red[threadIdx.x + o * N];
    __syncthreads();
  }
  if (lane == 0) part[(int64_t)blockIdx.x * N + n] = red[n];
}
// 256 / N lanes per column each add a strided subset of the P block sums (loads independent, in flight together),
// then the same fixed tree as the first pass
__global__ __launch_bounds__(256) void col_sum_fin_kernel(const double* __restrict__ part, int P, int N,
                                                          float* __restrict__ db) {
  __shared__ double red[256];
  const int n = threadIdx.x % N, lane = threadIdx.x / N, lanes = 256 / N;
  double s = 0.0;
#pragma unroll 8
  for (int p = lane; p < P; p += lanes) s += part[(int64_t)p * N + n];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = lanes / 2; o > 0; o >>= 1) {
    if (lane < o) red[threadIdx.x] += red[threadIdx.x + o * N];
    __syncthreads();
  }
  if (lane == 0) db[n] = (float)red[n];
}

int col_sum(const float* x, int64_t M, int N, float* db, double* scratch, hipStream_t st) {
  VAD_CHECK(N >= 1 && N <= 256 && 256 % N == 0, "col_sum: N divides 256");
  const int64_t rows = std::max<int64_t>(256 / N, cdiv(M, 256));
  const int P = (int)cdiv(M, rows);
  hipLaunchKernelGGL(col_sum_part_kernel, dim3((unsigned)P), dim3(256), 0, st, x, M, N, rows, scratch);
  VAD_LAUNCH_CHECK();
  hipLaunchKernelGGL(col_sum_fin_kernel, dim3(1), dim3(256), 0, st, scratch, P, N, db);
  VAD_LAUNCH_CHECK();
  return 0;
}
}  // namespace vad
