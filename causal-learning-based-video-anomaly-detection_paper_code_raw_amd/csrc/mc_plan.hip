// minicausal_vad_complete3.py (config 1): SimpleVideoAnomalyDetector (mc:25-102) train/eval step and the
// StableTrainer update (mc:249-330) as one device plan.
//
//   forward   3 x [im2col3d -> f32 MFMA GEMM (torch Conv3d weight as-is) -> BN3d partial sums -> bn_finalize
//             (batch stats, running stats) -> fused BN+ReLU+MaxPool3d] -> AdaptiveAvgPool3d(1) -> classifier kernel
//             (Dropout .5 / .3 from the keyed RNG, Linear/ReLU x2, Linear, sigmoid) + BCE + finiteness status
//   backward  classifier kernel (BCE/sigmoid/ReLU/dropout backward, classifier weight grads over the batch)
//             -> avg-pool backward -> per stage: MaxPool3d gather backward -> BN3d backward (reduce / finalize /
//             apply) -> weight+bias grad GEMM over the saved im2col columns -> input-grad GEMM + col2im
//   update    (optim.h) per-slot squared norms (float64) and finiteness -> grad norm, clip to max_norm only when the
//             norm exceeds clip_above (mc:304-306) -> Adam with coupled L2 weight decay (torch.optim.Adam semantics)
// Status word (losses[3]): 0 = skipped before backward (non-finite outputs or loss, mc:281-291), 1 = counted but
// not stepped (non-finite grads: zero_grad() then a no-op step, mc:296-301), 2 = stepped.
#include <cmath>
#include <string>
#include <vector>

#include "../../include/vad.h"
#include "backbone.h"
#include "conv3d.h"
#include "group_table.h"
#include "optim.h"
#include "plan_util.h"

namespace vad {

constexpr int MC_CO[3] = {8, 16, 32};
constexpr int MC_POOL[3][3] = {{1, 2, 2}, {2, 2, 2}, {2, 2, 2}};
constexpr int MC_FC[4] = {32, 16, 8, 1};
constexpr int MC_MAXB = 1024;

struct McLayout : FlatLayout {
  int conv_w[3], conv_b[3], bn_w[3], bn_b[3], fc_w[3], fc_b[3], rm[3], rv[3];
  explicit McLayout(int C) {
    int ci = C;
    for (int s = 0; s < 3; ++s) {
      const std::string c = "features." + std::to_string(4 * s), b = "features." + std::to_string(4 * s + 1);
      conv_w[s] = add(c + ".weight", (int64_t)MC_CO[s] * ci * 27);
      conv_b[s] = add(c + ".bias", MC_CO[s]);
      bn_w[s] = add(b + ".weight", MC_CO[s]);
      bn_b[s] = add(b + ".bias", MC_CO[s]);
      rm[s] = add_buf(b + ".running_mean", MC_CO[s]);
      rv[s] = add_buf(b + ".running_var", MC_CO[s]);
      ci = MC_CO[s];
    }
    const int fidx[3] = {1, 4, 6};
    for (int i = 0; i < 3; ++i) {
      const std::string f = "classifier." + std::to_string(fidx[i]);
      fc_w[i] = add(f + ".weight", (int64_t)MC_FC[i + 1] * MC_FC[i]);
      fc_b[i] = add(f + ".bias", MC_FC[i + 1]);
    }
    finish();
  }
};

// ------------------------------------------------------------------ classifier head
struct McHeadArgs {
  int B, training;
  int64_t clip0;
  const float* feats;  // [B][32]
  const float *W1, *b1, *W2, *b2, *W3, *b3;
  float *fd, *h1, *h1d, *h2, *o;  // saved activations
  float* scores;                  // [B]
  const float* labels;            // [B] nullable
  float* losses;                  // [4]
  int32_t* flags;                 // [4] nullable
  uint64_t hA, hB;                // dropout keys (mc classifier.0 / classifier.3)
  uint32_t thrA, thrB;
  float sA, sB;
};

__global__ __launch_bounds__(256) void mc_head_fwd_kernel(McHeadArgs a) {
  __shared__ float red[256];
  __shared__ int bad[256];
  float lsum = 0.f;
  int nonfin = 0;
  for (int b = threadIdx.x; b < a.B; b += 256) {
    const int64_t row = a.clip0 + b;
    float f[32], h1[16], h2[8];
    for (int c = 0; c < 32; ++c) {
      float v = a.feats[b * 32 + c];
      if (a.training) v = rng_u24(a.hA, (uint64_t)row, (uint64_t)c) >= a.thrA ? v * a.sA : 0.f;
      f[c] = v;
      a.fd[b * 32 + c] = v;
    }
    for (int k = 0; k < 16; ++k) {
      float z = a.b1[k];
      for (int c = 0; c < 32; ++c) z = fmaf(a.W1[k * 32 + c], f[c], z);
      z = relu_nan(z);
      a.h1[b * 16 + k] = z;
      if (a.training) z = rng_u24(a.hB, (uint64_t)row, (uint64_t)k) >= a.thrB ? z * a.sB : 0.f;
      h1[k] = z;
      a.h1d[b * 16 + k] = z;
    }
    for (int j = 0; j < 8; ++j) {
      float z = a.b2[j];
      for (int k = 0; k < 16; ++k) z = fmaf(a.W2[j * 16 + k], h1[k], z);
      h2[j] = relu_nan(z);
      a.h2[b * 8 + j] = h2[j];
    }
    float z = a.b3[0];
    for (int j = 0; j < 8; ++j) z = fmaf(a.W3[j], h2[j], z);
    const float o = 1.f / (1.f + expf(-z));
    a.o[b] = o;
    a.scores[b] = o;
    if (!isfinite(o)) nonfin = 1;
    if (a.labels) {
      // torch BCELoss: -(y * max(log(o), -100) + (1 - y) * max(log1p(-o), -100))
      const float y = a.labels[b];
      lsum += -(y * fmaxf(logf(o), -100.f) + (1.f - y) * fmaxf(log1pf(-o), -100.f));
    }
  }
  red[threadIdx.x] = lsum;
  bad[threadIdx.x] = nonfin;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[threadIdx.x] += red[threadIdx.x + s];
      bad[threadIdx.x] |= bad[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float loss = red[0] / (float)a.B;
    const bool ok = !bad[0] && (!a.labels || isfinite(loss));
    a.losses[0] = a.labels ? loss : 0.f;
    a.losses[1] = 0.f;
    a.losses[2] = 0.f;
    a.losses[3] = ok ? 2.f : 0.f;
    if (a.flags) a.flags[0] = ok ? 2 : 0;
  }
}

struct McHeadBwdArgs {
  McHeadArgs f;
  const float* d_scores;  // nullable: BCE of the forward's labels
  float *gW1, *gb1, *gW2, *gb2, *gW3, *gb3;
  float *dz1, *dz2, *dz3;  // scratch [B][16], [B][8], [B]
  float* dfeat;            // [B][32]
};

__global__ __launch_bounds__(256) void mc_head_bwd_kernel(McHeadBwdArgs a) {
  const McHeadArgs& f = a.f;
  const int B = f.B;
  for (int b = threadIdx.x; b < B; b += 256) {
    const int64_t row = f.clip0 + b;
    const float o = f.o[b];
    float dout;
    if (a.d_scores) {
      dout = a.d_scores[b];
    } else {
      // torch binary_cross_entropy_backward (mean): (o - y) / max((1 - o) * o, 1e-12) / B
      dout = (o - f.labels[b]) / fmaxf((1.f - o) * o, 1e-12f) / (float)B;
    }
    const float dz3 = dout * (1.f - o) * o;
    a.dz3[b] = dz3;
    float dz2[8];
    for (int j = 0; j < 8; ++j) {
      dz2[j] = f.h2[b * 8 + j] > 0.f ? dz3 * f.W3[j] : 0.f;
      a.dz2[b * 8 + j] = dz2[j];
    }
    float dz1[16];
    for (int k = 0; k < 16; ++k) {
      float d = 0.f;
      for (int j = 0; j < 8; ++j) d = fmaf(dz2[j], f.W2[j * 16 + k], d);
      if (f.training) d = rng_u24(f.hB, (uint64_t)row, (uint64_t)k) >= f.thrB ? d * f.sB : 0.f;
      dz1[k] = f.h1[b * 16 + k] > 0.f ? d : 0.f;
      a.dz1[b * 16 + k] = dz1[k];
    }
    for (int c = 0; c < 32; ++c) {
      float d = 0.f;
      for (int k = 0; k < 16; ++k) d = fmaf(dz1[k], f.W1[k * 32 + c], d);
      if (f.training) d = rng_u24(f.hA, (uint64_t)row, (uint64_t)c) >= f.thrA ? d * f.sA : 0.f;
      a.dfeat[b * 32 + c] = d;
    }
  }
  __syncthreads();
  // classifier weight grads: fixed-order sums over the batch, one thread per weight element
  constexpr int N3 = 8 + 1, N2 = 8 * 16 + 8, N1 = 16 * 32 + 16;
  for (int e = threadIdx.x; e < N3 + N2 + N1; e += 256) {
    float s = 0.f;
    if (e < 8) {
      for (int b = 0; b < B; ++b) s = fmaf(a.dz3[b], f.h2[b * 8 + e], s);
      a.gW3[e] = s;
    } else if (e < N3) {
      for (int b = 0; b < B; ++b) s += a.dz3[b];
      a.gb3[0] = s;
    } else if (e < N3 + 128) {
      const int q = e - N3, j = q / 16, k = q % 16;
      for (int b = 0; b < B; ++b) s = fmaf(a.dz2[b * 8 + j], f.h1d[b * 16 + k], s);
      a.gW2[q] = s;
    } else if (e < N3 + N2) {
      const int j = e - N3 - 128;
      for (int b = 0; b < B; ++b) s += a.dz2[b * 8 + j];
      a.gb2[j] = s;
    } else if (e < N3 + N2 + 512) {
      const int q = e - N3 - N2, k = q / 32, c = q % 32;
      for (int b = 0; b < B; ++b) s = fmaf(a.dz1[b * 16 + k], f.fd[b * 32 + c], s);
      a.gW1[q] = s;
    } else {
      const int k = e - N3 - N2 - 512;
      for (int b = 0; b < B; ++b) s += a.dz1[b * 16 + k];
      a.gb1[k] = s;
    }
  }
}

__global__ void mc_nbt_kernel(int64_t* nbt, int n) {
  if (threadIdx.x < n) nbt[threadIdx.x] += 1;
}

// ------------------------------------------------------------------ the plan
struct McPlanImpl {
  int B, C, T, H, W;
  McLayout LY;
  Conv3dGeom g[3];
  Vol5 conv_out[3], pooled_vol[3];
  int64_t ws_bytes = 0;
  float *params = nullptr, *grads = nullptr, *bufs = nullptr, *m = nullptr, *v = nullptr;
  int64_t* nbt = nullptr;
  int32_t* steps = nullptr;
  // workspace
  float *cols[3], *y[3], *pooled[3], *stats[3], *wf[3], *wd[3], *xin;
  float *parts, *bparts, *feats, *fd, *h1, *h1d, *h2, *o, *dz1, *dz2, *dz3, *dfeat, *dpool, *dA, *dY, *dcols;
  float *scratch, *labels_copy, *losses;
  AdamWs aws{};
  int32_t* flags = nullptr;
  int64_t parts_floats = 0, scratch_floats = 0;
  // per-call state
  int training = 1, direct_fwd = 0;
  uint64_t seed = 0, step = 0;
  int64_t clip0 = 0;
  bool have_labels = false;
  bool win_dirty = false;  // the activations are a windows call's: no backward until the next clip forward

  McPlanImpl(int B_, int C_, int T_, int H_, int W_) : B(B_), C(C_), T(T_), H(H_), W(W_), LY(C_) {
    Vol5 in{B, C, T, H, W};
    for (int s = 0; s < 3; ++s) {
      g[s] = conv3d_geom(in, MC_CO[s], 3, 1, 1, 1, 1);
      conv_out[s] = g[s].out();
      pooled_vol[s] = {B, MC_CO[s], conv_out[s].D / MC_POOL[s][0], conv_out[s].H / MC_POOL[s][1],
                       conv_out[s].W / MC_POOL[s][2]};
      in = pooled_vol[s];
    }
  }
  float* P(int s) const { return params + LY.slots[s].offset; }
  float* G(int s) const { return grads + LY.slots[s].offset; }
  float* RM(int s) const { return bufs + LY.bufs[LY.rm[s]].offset; }
  float* RV(int s) const { return bufs + LY.bufs[LY.rv[s]].offset; }

  void carve(Ws& w) {
    int64_t max_y = 0, max_pool = 0, max_dcols = 0;
    parts_floats = 1024;
    for (int s = 0; s < 3; ++s) {
      const int64_t V = conv_out[s].voxels(), Co = MC_CO[s];
      cols[s] = w.take<float>(g[s].rows() * g[s].K());
      y[s] = w.take<float>(V * Co);
      pooled[s] = w.take<float>(pooled_vol[s].numel());
      stats[s] = w.take<float>(BN_STATS_PER_C * Co);
      max_y = std::max(max_y, V * Co);
      max_pool = std::max(max_pool, pooled_vol[s].numel());
      if (s > 0) max_dcols = std::max(max_dcols, g[s].rows() * g[s].K());
      parts_floats = std::max<int64_t>(parts_floats, std::max<int64_t>(bn_fwd_partials_blocks(V), cdiv(V, 64)) * 2 * Co);
    }
    for (int s = 0; s < 3; ++s) {
      const int64_t n = (int64_t)MC_CO[s] * g[s].in.C * 27;
      wf[s] = w.take<float>(n);
      wd[s] = w.take<float>(n);
    }
    xin = w.take<float>(g[0].in.numel());  // (the forward input, kept for the direct weight gradient)
    max_pool = std::max(max_pool, g[1].in.numel());
    max_pool = std::max(max_pool, g[2].in.numel());
    parts = w.take<float>(parts_floats);
    bparts = w.take<float>(parts_floats);
    feats = w.take<float>((int64_t)B * 32);
    fd = w.take<float>((int64_t)B * 32);
    h1 = w.take<float>((int64_t)B * 16);
    h1d = w.take<float>((int64_t)B * 16);
    h2 = w.take<float>((int64_t)B * 8);
    o = w.take<float>(B);
    dz1 = w.take<float>((int64_t)B * 16);
    dz2 = w.take<float>((int64_t)B * 8);
    dz3 = w.take<float>(B);
    dfeat = w.take<float>((int64_t)B * 32);
    dpool = w.take<float>(max_pool);
    dA = w.take<float>(max_y);
    dY = w.take<float>(max_y);
    dcols = w.take<float>(std::max<int64_t>(max_dcols, 1));
    scratch_floats = 8ll << 20;
    scratch = w.take<float>(scratch_floats);
    labels_copy = w.take<float>(B);
    losses = w.take<float>(4);
    aws.carve(w);
  }

  McHeadArgs head_args() const {
    McHeadArgs a{};
    a.B = B;
    a.training = training;
    a.clip0 = clip0;
    a.feats = feats;
    a.W1 = P(LY.fc_w[0]); a.b1 = P(LY.fc_b[0]);
    a.W2 = P(LY.fc_w[1]); a.b2 = P(LY.fc_b[1]);
    a.W3 = P(LY.fc_w[2]); a.b3 = P(LY.fc_b[2]);
    a.fd = fd; a.h1 = h1; a.h1d = h1d; a.h2 = h2; a.o = o;
    a.labels = have_labels ? labels_copy : nullptr;
    a.losses = losses;
    a.flags = flags;
    a.hA = rng_h1(seed, S_MC_DROP1, step);
    a.hB = rng_h1(seed, S_MC_DROP2, step);
    a.thrA = drop_threshold(0.5);
    a.thrB = drop_threshold(0.3);
    a.sA = 1.0f / (float)(1.0 - 0.5);
    a.sB = 1.0f / (float)(1.0 - 0.3);
    return a;
  }

  bool direct(int s) const { return conv3d_direct_supported(g[s].in.C, MC_CO[s]); }

  int forward(const float* x, float* scores, hipStream_t st) {
    // direct convs (conv3d_direct.hip) keep the input for the weight gradient instead of the im2col columns
    direct_fwd = direct(0) && direct(1) && direct(2);
    win_dirty = false;
    if (direct_fwd)
      VAD_HIP(hipMemcpyAsync(xin, x, g[0].in.numel() * sizeof(float), hipMemcpyDeviceToDevice, st));
    for (int s = 0; s < 3; ++s) {
      const int Co = MC_CO[s];
      const int64_t V = conv_out[s].voxels();
      const float* src = s == 0 ? x : pooled[s - 1];
      const Strides5 str = s == 0 ? ncdhw_strides(g[0].in) : ndhwc_strides(g[s].in);
      if (direct_fwd) {
        VAD_TRY(conv3d_direct_prep(P(LY.conv_w[s]), Co, g[s].in.C, wf[s], wd[s], st));
        VAD_TRY(conv3d_direct_fwd(src, str, g[s].in, wf[s], Co, P(LY.conv_b[s]), y[s], st));
      } else {
        VAD_TRY(im2col3d(src, str, g[s], nullptr, nullptr, 0, cols[s], st));
        VAD_TRY(dense_fwd(cols[s], (int)g[s].rows(), g[s].K(), P(LY.conv_w[s]), P(LY.conv_b[s]), Co, y[s],
                          DenseAct{}, scratch, scratch_floats, st));
      }
      int np = 0;
      if (training) VAD_TRY(bn_fwd_partials(y[s], V, Co, parts, &np, st));
      VAD_TRY(bn_finalize(parts, np, Co, (double)V, P(LY.bn_w[s]), P(LY.bn_b[s]), RM(s), RV(s), 0.1f, 1e-5f,
                          training, stats[s], st));
      VAD_TRY(maxpool3d_fwd(y[s], stats[s], 1, conv_out[s], MC_POOL[s][0], MC_POOL[s][1], MC_POOL[s][2], pooled[s],
                            st));
    }
    VAD_TRY(adaptive_avgpool3d_fwd(pooled[2], nullptr, 0, pooled_vol[2], 1, 1, 1, feats, st));
    VAD_TRY(head(scores, st));
    if (training && nbt) {
      hipLaunchKernelGGL(mc_nbt_kernel, dim3(1), dim3(64), 0, st, nbt, 3);
      VAD_LAUNCH_CHECK();
    }
    return 0;
  }

  // The first nw clips of the plan as windows of a video or ring (vad_mc_windows_forward), eval semantics: the forward
  // above with training = 0 on nw clips, conv 1 reading the frames in place.  The running statistics, the counters,
  // the plan's loss and status words and its per-call state are left alone (the classifier's three loss words go to
  // the BatchNorm partials scratch, which nothing reads in eval mode); the activations are overwritten, so a backward
  // is refused until the next clip forward (win_dirty).
  int check_windows() const {
    VAD_CHECK(direct(0) && direct(1) && direct(2),
              "vad_mc_windows_forward: windows are read by the direct 3-D convs only (knob conv3d_direct = 1 and at most "
              "16 input channels); the im2col path has no windows form");
    return 0;
  }

  int forward_windows(const WinSrc& src, int nw, float* scores, hipStream_t st) {
    VAD_TRY(check_windows());
    win_dirty = true;
    for (int s = 0; s < 3; ++s) {
      const int Co = MC_CO[s];
      Vol5 in = g[s].in, co = conv_out[s];
      in.N = co.N = nw;
      VAD_TRY(conv3d_direct_prep(P(LY.conv_w[s]), Co, in.C, wf[s], wd[s], st));
      if (s == 0) VAD_TRY(conv3d_direct_fwd_windows(src, in, wf[s], Co, P(LY.conv_b[s]), y[s], st));
      else VAD_TRY(conv3d_direct_fwd(pooled[s - 1], ndhwc_strides(in), in, wf[s], Co, P(LY.conv_b[s]), y[s], st));
      VAD_TRY(bn_finalize(parts, 0, Co, (double)co.voxels(), P(LY.bn_w[s]), P(LY.bn_b[s]), RM(s), RV(s), 0.1f, 1e-5f, 0,
                          stats[s], st));
      VAD_TRY(maxpool3d_fwd(y[s], stats[s], 1, co, MC_POOL[s][0], MC_POOL[s][1], MC_POOL[s][2], pooled[s], st));
    }
    Vol5 pv = pooled_vol[2];
    pv.N = nw;
    VAD_TRY(adaptive_avgpool3d_fwd(pooled[2], nullptr, 0, pv, 1, 1, 1, feats, st));
    McHeadArgs a = head_args();
    a.B = nw;
    a.training = 0;
    a.labels = nullptr;
    a.flags = nullptr;
    a.losses = parts;
    a.scores = scores;
    hipLaunchKernelGGL(mc_head_fwd_kernel, dim3(1), dim3(256), 0, st, a);
    VAD_LAUNCH_CHECK();
    return 0;
  }

  // everything behind the average pool, on the plan's feature rows: the classifier (Dropout x2 from the keyed RNG),
  // the BCE and the status words (vad_mc_head_forward runs this alone)
  int head(float* scores, hipStream_t st) {
    McHeadArgs a = head_args();
    a.scores = scores;
    hipLaunchKernelGGL(mc_head_fwd_kernel, dim3(1), dim3(256), 0, st, a);
    VAD_LAUNCH_CHECK();
    return 0;
  }

  int backward(const float* d_scores, hipStream_t st) {
    VAD_CHECK(d_scores || have_labels, "vad_mc_backward: no labels in the forward and no d_scores");
    VAD_CHECK(!win_dirty, "vad_mc_backward: vad_mc_windows_forward has overwritten this plan's activations since its "
                          "last forward");
    VAD_TRY(backward_head(d_scores, st));
    return backward_convs(st);
  }

  // the head's share of the backward: up to and including dfeat and the six classifier gradients
  // (vad_mc_head_backward runs this alone)
  int backward_head(const float* d_scores, hipStream_t st) {
    McHeadBwdArgs hb{};
    hb.f = head_args();
    hb.d_scores = d_scores;
    hb.gW1 = G(LY.fc_w[0]); hb.gb1 = G(LY.fc_b[0]);
    hb.gW2 = G(LY.fc_w[1]); hb.gb2 = G(LY.fc_b[1]);
    hb.gW3 = G(LY.fc_w[2]); hb.gb3 = G(LY.fc_b[2]);
    hb.dz1 = dz1; hb.dz2 = dz2; hb.dz3 = dz3; hb.dfeat = dfeat;
    hipLaunchKernelGGL(mc_head_bwd_kernel, dim3(1), dim3(256), 0, st, hb);
    VAD_LAUNCH_CHECK();
    return 0;
  }

  int backward_convs(hipStream_t st) {
    VAD_TRY(adaptive_avgpool3d_bwd(dfeat, pooled_vol[2], 1, 1, 1, dpool, st));
    for (int s = 2; s >= 0; --s) {
      const int Co = MC_CO[s];
      const int64_t V = conv_out[s].voxels();
      VAD_TRY(maxpool3d_bwd(y[s], stats[s], 1, conv_out[s], MC_POOL[s][0], MC_POOL[s][1], MC_POOL[s][2], dpool, dA,
                            st));
      int np = 0, nb = 0;
      VAD_TRY(bn_bwd_reduce(dA, y[s], stats[s], (int)V, Co, parts, &np, st));
      VAD_TRY(bn_bwd_finalize(parts, np, Co, (double)V, P(LY.bn_w[s]), stats[s], G(LY.bn_w[s]), G(LY.bn_b[s]),
                              training, st));
      VAD_TRY(bn_bwd_apply(dA, y[s], stats[s], (int)V, Co, dY, bparts, &nb, st));
      if (direct_fwd) {
        const float* src = s == 0 ? xin : pooled[s - 1];
        const Strides5 str = s == 0 ? ncdhw_strides(g[0].in) : ndhwc_strides(g[s].in);
        VAD_TRY(conv3d_direct_wgrad(dY, Co, src, str, g[s].in, G(LY.conv_w[s]), G(LY.conv_b[s]), scratch,
                                    scratch_floats, st));
        if (s > 0) {  // dX = conv(dY, flipped W^T): NDHWC over the layer's input grid
          const Vol5 vy{g[s].in.N, Co, g[s].in.D, g[s].in.H, g[s].in.W};
          VAD_TRY(conv3d_direct_fwd(dY, ndhwc_strides(vy), vy, wd[s], g[s].in.C, nullptr, dpool, st));
        }
      } else {
        VAD_TRY(dense_wgrad(dY, (int)V, Co, cols[s], g[s].K(), G(LY.conv_w[s]), G(LY.conv_b[s]), scratch,
                            scratch_floats, nullptr, st));
        if (s > 0) {
          VAD_TRY(dense_dgrad(dY, (int)V, Co, P(LY.conv_w[s]), g[s].K(), dcols, nullptr, 1.f, nullptr, st));
          VAD_TRY(col2im3d(dcols, g[s], dpool, st));
        }
      }
    }
    return 0;
  }

  int optimizer(float lr, float b1, float b2, float eps, float wd, float clip_above, float max_norm, hipStream_t st) {
    // coupled decay; the clip only above clip_above (mc:304-306); losses[1] norm, [2] clipped, [3] the status word
    const AdamStep a{lr, b1, b2, eps, wd, false, clip_above, max_norm, 1.f, losses + 3, losses + 1, nullptr,
                     losses + 2, losses + 3};
    return adam_clip_step(LY.adam_slots(), params, grads, m, v, LY.param_floats, steps, aws, a, st);
  }
};

}  // namespace vad

using namespace vad;

struct vad_mc_plan {
  explicit vad_mc_plan(int B, int C, int T, int H, int W) : impl(B, C, T, H, W) {}
  McPlanImpl impl;
  float* user_losses = nullptr;
};

extern "C" {

int vad_mc_create(int B, int C, int T, int H, int W, vad_mc_plan** out) {
  VAD_CHECK(out != nullptr, "vad_mc_create: out is null");
  VAD_CHECK(B >= 1 && B <= MC_MAXB && C >= 1 && C <= 64 && T >= 4 && H >= 8 && W >= 8,
            "vad_mc_create: unsupported shape (B<=1024, T>=4, H,W>=8 so every MaxPool3d window fits)");
  auto* p = new vad_mc_plan(B, C, T, H, W);
  for (int s = 0; s < 3; ++s)
    if (p->impl.pooled_vol[s].D < 1 || p->impl.pooled_vol[s].H < 1 || p->impl.pooled_vol[s].W < 1) {
      delete p;
      set_error("vad_mc_create: input too small for the three MaxPool3d stages");
      return 1;
    }
  Ws ws;
  p->impl.carve(ws);
  p->impl.ws_bytes = ws.off + 256;
  *out = p;
  return 0;
}

void vad_mc_destroy(vad_mc_plan* plan) { delete plan; }

VAD_FLAT_SLOT_ABI(mc, (const vad_mc_plan* p), (const vad_mc_plan* p, int i), p ? &p->impl.LY : nullptr)
VAD_FLAT_BUF_ABI(mc, (const vad_mc_plan* p), (const vad_mc_plan* p, int i), p ? &p->impl.LY : nullptr)
int64_t vad_mc_workspace_bytes(const vad_mc_plan* p) { return p ? p->impl.ws_bytes : -1; }

int vad_mc_bind(vad_mc_plan* plan, void* workspace, float* params, float* grads, float* bufs, int64_t* nbt,
                float* exp_avg, float* exp_avg_sq, int32_t* steps) {
  VAD_CHECK(plan && workspace && params && grads && bufs && exp_avg && exp_avg_sq && steps,
            "vad_mc_bind: null argument");
  VAD_CHECK((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "vad_mc_bind: workspace must be 256-B aligned");
  McPlanImpl& c = plan->impl;
  Ws ws;
  ws.base = reinterpret_cast<char*>(workspace);
  ws.dry = false;
  c.carve(ws);
  c.params = params; c.grads = grads; c.bufs = bufs; c.nbt = nbt;
  c.m = exp_avg; c.v = exp_avg_sq; c.steps = steps;
  return 0;
}

int vad_mc_forward(vad_mc_plan* plan, const float* x, int training, uint64_t seed, uint64_t step, int64_t clip0,
                   const float* labels, float* scores, float* losses, int32_t* flags, void* stream) {
  VAD_CHECK(plan && x && scores, "vad_mc_forward: null argument");
  McPlanImpl& c = plan->impl;
  VAD_CHECK(c.params != nullptr, "vad_mc_forward: plan not bound");
  hipStream_t st = (hipStream_t)stream;
  c.training = training;
  c.seed = seed;
  c.step = step;
  c.clip0 = clip0;
  c.have_labels = labels != nullptr;
  c.flags = flags;
  if (labels) VAD_HIP(hipMemcpyAsync(c.labels_copy, labels, sizeof(float) * c.B, hipMemcpyDeviceToDevice, st));
  VAD_TRY(c.forward(x, scores, st));
  plan->user_losses = losses;
  if (losses) VAD_HIP(hipMemcpyAsync(losses, c.losses, 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
  return 0;
}

int vad_mc_windows_forward(vad_mc_plan* plan, const float* frames, int64_t n_frames, int64_t first, int64_t stride,
                           int64_t ring, int nw, float* scores, void* stream) {
  VAD_CHECK(plan && frames && scores, "vad_mc_windows_forward: null argument");
  McPlanImpl& c = plan->impl;
  VAD_TRY(win_check("vad_mc_windows_forward", n_frames, first, stride, ring, nw, c.B, c.T));
  VAD_CHECK(c.params != nullptr, "vad_mc_windows_forward: plan not bound");
  const WinSrc ws{frames, (int64_t)c.C * c.H * c.W, first, stride, ring};
  return c.forward_windows(ws, nw, scores, (hipStream_t)stream);
}

int vad_mc_windows_forward_group(vad_mc_plan* plan, const float* ring, int64_t total_slots, int cap,
                                 const int64_t* host_windows, int nw, void* dev_table, float* scores, void* stream) {
  const char* fn = "vad_mc_windows_forward_group";
  VAD_CHECK(plan && scores, std::string(fn) + ": null plan or scores");
  McPlanImpl& c = plan->impl;
  VAD_TRY(win_group_check(fn, ring, total_slots, cap, host_windows, nw, dev_table, c.B, c.T));
  VAD_CHECK(c.params != nullptr, std::string(fn) + ": plan not bound");
  VAD_TRY(c.check_windows());
  WinSrc ws;
  VAD_TRY(win_group_src(fn, ring, (int64_t)c.C * c.H * c.W, total_slots, cap, host_windows, nw, dev_table,
                        (hipStream_t)stream, ws));
  return c.forward_windows(ws, nw, scores, (hipStream_t)stream);
}

int vad_mc_backward(vad_mc_plan* plan, const float* d_scores, void* stream) {
  VAD_CHECK(plan != nullptr, "vad_mc_backward: null plan");
  return plan->impl.backward(d_scores, (hipStream_t)stream);
}

int vad_mc_head_forward(vad_mc_plan* plan, const float* feats, int training, uint64_t seed, uint64_t step,
                        int64_t clip0, const float* labels, float* scores, float* losses, int32_t* flags,
                        float* const* saved, void* stream) {
  VAD_CHECK(plan != nullptr, "vad_mc_head_forward: null plan");
  McPlanImpl& c = plan->impl;
  VAD_CHECK(c.params != nullptr, "vad_mc_head_forward: plan not bound");
  VAD_CHECK(training == 0 || training == 1, "vad_mc_head_forward: training is 0 or 1");
  VAD_CHECK(scores != nullptr, "vad_mc_head_forward: null scores");
  hipStream_t st = (hipStream_t)stream;
  const int64_t B = c.B;
  if (feats) VAD_HIP(hipMemcpyAsync(c.feats, feats, sizeof(float) * B * 32, hipMemcpyDeviceToDevice, st));
  c.training = training;
  c.seed = seed;
  c.step = step;
  c.clip0 = clip0;
  c.have_labels = labels != nullptr;
  c.flags = flags;
  if (labels) VAD_HIP(hipMemcpyAsync(c.labels_copy, labels, sizeof(float) * B, hipMemcpyDeviceToDevice, st));
  VAD_TRY(c.head(scores, st));
  plan->user_losses = losses;
  const float* src[6] = {c.losses, c.fd, c.h1, c.h1d, c.h2, c.o};
  float* dst[6] = {losses};
  const int64_t n[6] = {4, B * 32, B * 16, B * 16, B * 8, B};
  for (int k = 0; k < 5; ++k) dst[1 + k] = saved ? saved[k] : nullptr;
  for (int k = 0; k < 6; ++k)
    if (dst[k]) VAD_HIP(hipMemcpyAsync(dst[k], src[k], sizeof(float) * n[k], hipMemcpyDeviceToDevice, st));
  return 0;
}

int vad_mc_head_backward(vad_mc_plan* plan, const float* d_scores, float* dfeat, float* const* dz, void* stream) {
  VAD_CHECK(plan != nullptr, "vad_mc_head_backward: null plan");
  McPlanImpl& c = plan->impl;
  VAD_CHECK(c.params != nullptr, "vad_mc_head_backward: plan not bound");
  VAD_CHECK(d_scores || c.have_labels, "vad_mc_head_backward: no labels in the last head forward and no d_scores");
  hipStream_t st = (hipStream_t)stream;
  VAD_TRY(c.backward_head(d_scores, st));
  const int64_t B = c.B;
  const float* src[4] = {c.dfeat, c.dz1, c.dz2, c.dz3};
  float* dst[4] = {dfeat};
  const int64_t n[4] = {B * 32, B * 16, B * 8, B};
  for (int k = 0; k < 3; ++k) dst[1 + k] = dz ? dz[k] : nullptr;
  for (int k = 0; k < 4; ++k)
    if (dst[k]) VAD_HIP(hipMemcpyAsync(dst[k], src[k], sizeof(float) * n[k], hipMemcpyDeviceToDevice, st));
  return 0;
}

int vad_mc_optimizer_step(vad_mc_plan* plan, float lr, float beta1, float beta2, float eps, float weight_decay,
                          float clip_above, float max_norm, void* stream) {
  VAD_CHECK(plan != nullptr, "vad_mc_optimizer_step: null plan");
  McPlanImpl& c = plan->impl;
  hipStream_t st = (hipStream_t)stream;
  VAD_TRY(c.optimizer(lr, beta1, beta2, eps, weight_decay, clip_above, max_norm, st));
  if (plan->user_losses)
    VAD_HIP(hipMemcpyAsync(plan->user_losses, c.losses, 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
  return 0;
}

}  // extern "C"
