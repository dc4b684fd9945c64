// Stand-alone entry points for single building blocks (dense layers, the fused MLP chain, 3x3 conv, the 3-D clip
// blocks, the causal head) used by the kernel unit tests.
#include <string>

#include "../../include/vad.h"
#include "backbone.h"
#include "conv3d.h"
#include "head.h"
#include "mlp.h"

using namespace vad;

extern "C" {

int vad_dense_forward(const float* X, int M, int K, const float* W, const float* b, int N, float* Y, int relu,
                      float* scratch, int64_t scratch_floats, void* stream) {
  DenseAct a;
  a.relu = relu;
  return dense_fwd(X, M, K, W, b, N, Y, a, scratch, scratch_floats, (hipStream_t)stream);
}

int vad_conv3x3_forward(const float* x_nhwc, int NF, int Ci, int IH, int IW, const float* w, const float* bias,
                        int Co, int stride, float* y_nhwc, float* wf_scratch, float* wd_scratch, float* partials,
                        void* stream) {
  Conv3Layer L{NF, Ci, Co, IH, IW, (IH - 1) / stride + 1, (IW - 1) / stride + 1, stride};
  if (w) VAD_TRY(conv3_prep_weights(w, L, wf_scratch, wd_scratch, (hipStream_t)stream));  // w == NULL: prepared
  int np = 0;
  return conv3_fwd(L, x_nhwc, nullptr, wf_scratch, bias, y_nhwc, partials, &np, (hipStream_t)stream);
}

int vad_conv3x3_dgrad(const float* dy_nhwc, int NF, int Ci, int IH, int IW, const float* w, int Co, int stride,
                      float* dx_nhwc, float* wf_scratch, float* wd_scratch, void* stream) {
  Conv3Layer L{NF, Ci, Co, IH, IW, (IH - 1) / stride + 1, (IW - 1) / stride + 1, stride};
  if (w) VAD_TRY(conv3_prep_weights(w, L, wf_scratch, wd_scratch, (hipStream_t)stream));  // w == NULL: prepared
  return conv3_dgrad(L, dy_nhwc, wd_scratch, dx_nhwc, (hipStream_t)stream);
}

int vad_conv3x3_forward_bn(const float* x_nhwc, const float* src_stats, int NF, int Ci, int IH, int IW, const float* w,
                           const float* bias, int Co, int stride, float* y_nhwc, float* wf_scratch, float* wd_scratch,
                           float* partials, int* nparts, int* parts_cm, void* stream) {
  Conv3Layer L{NF, Ci, Co, IH, IW, (IH - 1) / stride + 1, (IW - 1) / stride + 1, stride};
  if (w) VAD_TRY(conv3_prep_weights(w, L, wf_scratch, wd_scratch, (hipStream_t)stream));  // w == NULL: prepared
  return conv3_fwd(L, x_nhwc, src_stats, wf_scratch, bias, y_nhwc, partials, nparts, (hipStream_t)stream, parts_cm);
}

int vad_conv3x3_dgrad_bnfuse(const float* dy_nhwc, int NF, int Ci, int IH, int IW, const float* w, int Co, int stride,
                             float* dx_nhwc, float* wf_scratch, float* wd_scratch, const float* y_nhwc,
                             const float* stats, float* parts, int64_t parts_floats, int* nparts, void* stream) {
  Conv3Layer L{NF, Ci, Co, IH, IW, (IH - 1) / stride + 1, (IW - 1) / stride + 1, stride};
  if (w) VAD_TRY(conv3_prep_weights(w, L, wf_scratch, wd_scratch, (hipStream_t)stream));  // w == NULL: prepared
  const BnBwdFuse f{y_nhwc, stats, parts, parts_floats, nparts};
  return conv3_dgrad(L, dy_nhwc, wd_scratch, dx_nhwc, (hipStream_t)stream, &f);
}

}  // extern "C"

extern "C" int vad_conv3x3_wgrad(const float* x_nhwc, const float* dy_nhwc, int NF, int Ci, int IH, int IW, int Co,
                                 int stride, float* dW, float* partial, int64_t partial_floats, void* stream) {
  Conv3Layer L{NF, Ci, Co, IH, IW, (IH - 1) / stride + 1, (IW - 1) / stride + 1, stride};
  int ns = 0;
  VAD_TRY(conv3_wgrad(L, dy_nhwc, x_nhwc, nullptr, partial, &ns, partial_floats, (hipStream_t)stream));
  return conv3_wgrad_reduce(L, partial, ns, nullptr, 0, dW, nullptr, (hipStream_t)stream);
}

extern "C" int vad_set_tuning(const char* key, int value) { return vad::set_tuning(key, value); }
extern "C" int vad_get_tuning(const char* key, int* value) { return vad::get_tuning(key, value); }
extern "C" const char* vad_tuning_name(int i) { return vad::tuning_name(i); }

// The BN backward apply pass alone (measurement / tests): dY = k (dZ - mean dZ - xhat mean(dZ xhat)), dZ = dA masked by
// the ReLU of s y + t; stats = the layer's [7 C] BN state; bf16: dA / y / dY stored as bf16 (config 4).
extern "C" int vad_bn_bwd_apply(const void* dA, const void* y, const float* stats, int M, int C, void* dY, int bf16,
                                void* stream) {
  ActStorage abf(bf16);
  int nb = 0;
  return bn_bwd_apply(reinterpret_cast<const float*>(dA), reinterpret_cast<const float*>(y), stats, M, C,
                      reinterpret_cast<float*>(dY), nullptr, &nb, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------------------
// The 3-D building blocks of the clip-level CNNs, one kernel family per call (the plans pick a family by shape and
// knobs; the unit tests pin each at the shapes the plans accept).  Thin wrappers: weight images, columns and split-K
// slabs are carved from the caller's scratch in the order the plans keep them.
// ------------------------------------------------------------------------------------------------------------
namespace {

constexpr int64_t kAlign = 64;  // floats: every carved region starts 256-byte aligned
int64_t up(int64_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

struct Conv3dCall {
  Vol5 in;
  Conv3dGeom g;
  int Co, path;
};

// kind 0 forward / 1 input gradient / 2 weight gradient; sets the error text and returns non-zero when `path` does not
// run this combination
int conv3d_call(int kind, int path, int layout, int N, int Ci, int D, int H, int W, int Co, int sd, int sh, int sw,
                bool gate, Conv3dCall* c) {
  VAD_CHECK(kind >= 0 && kind <= 2 && N >= 1 && Ci >= 1 && Co >= 1 && D >= 1 && H >= 1 && W >= 1 && sd >= 1 &&
                sh >= 1 && sw >= 1 && (layout == 0 || layout == 1),
            "vad_conv3d: unsupported shape");
  const bool s1 = sd == 1 && sh == 1 && sw == 1, s2 = sd == 2 && sh == 2 && sw == 2;
  switch (path) {
    case 0:
      VAD_CHECK(!gate, "vad_conv3d: path 0 (im2col) has no fused gate");
      break;
    case 1:
      VAD_CHECK(s1, "vad_conv3d: path 1 (direct) is stride 1");
      VAD_CHECK(Ci <= 16 && (Co == 8 || Co == 16 || Co == 32), "vad_conv3d: path 1 (direct) needs Ci <= 16 and Co in {8, 16, 32}");
      VAD_CHECK(kind != 1 || Ci == 8 || Ci == 16, "vad_conv3d: path 1 (direct) input gradient needs Ci in {8, 16}");
      VAD_CHECK(!gate, "vad_conv3d: path 1 (direct) has no fused gate");
      break;
    case 2:
      VAD_CHECK(s2, "vad_conv3d: path 2 (conv3s2) is stride 2 on all three axes");
      VAD_CHECK(Ci % 4 == 0 && Co % 4 == 0, "vad_conv3d: path 2 (conv3s2) needs Ci % 4 == 0 and Co % 4 == 0");
      VAD_CHECK(layout == 1, "vad_conv3d: path 2 (conv3s2) reads NDHWC");
      break;
    case 3:
      VAD_CHECK(kind == 0, "vad_conv3d: path 3 (x3) is forward only");
      VAD_CHECK(s1, "vad_conv3d: path 3 (x3) is stride 1");
      VAD_CHECK(Ci % 16 == 0 && Co % 32 == 0, "vad_conv3d: path 3 (x3) needs Ci % 16 == 0 and Co % 32 == 0");
      VAD_CHECK(layout == 1, "vad_conv3d: path 3 (x3) reads NDHWC");
      break;
    default:
      VAD_CHECK(false, "vad_conv3d: unknown path");
  }
  c->in = Vol5{N, Ci, D, H, W};
  c->g = conv3d_geom(c->in, Co, 3, sd, sh, sw, 1);
  c->Co = Co;
  c->path = path;
  VAD_CHECK(c->g.rows() * c->g.K() < (1ll << 31) && c->in.numel() < (1ll << 31) && c->g.rows() * Co < (1ll << 31),
            "vad_conv3d: volume too large for a unit call");
  return 0;
}

int64_t conv3d_min_scratch(int kind, const Conv3dCall& c) {
  const int64_t wimg = 27ll * c.in.C * c.Co, cols = c.g.rows() * c.g.K();
  switch (c.path) {
    case 0: return up(cols) + (kind == 2 ? (int64_t)c.Co * (c.g.K() + 1) : 0);
    case 1: return kind == 2 ? conv3d_direct_wgrad_slab_floats(c.in, c.Co) : 2 * up(wimg);
    case 2: return kind == 2 ? (int64_t)c.Co * (27 * c.in.C + 1) : 2 * up(wimg);
    default: return up(wimg);
  }
}

}  // namespace

extern "C" int64_t vad_conv3d_scratch_floats(int kind, int path, int N, int Ci, int D, int H, int W, int Co, int sd,
                                             int sh, int sw) {
  Conv3dCall c;
  if (conv3d_call(kind, path, 1, N, Ci, D, H, W, Co, sd, sh, sw, false, &c) != 0) return -1;
  return conv3d_min_scratch(kind, c);
}

extern "C" int vad_conv3d_forward(const float* x, int layout, int N, int Ci, int D, int H, int W, const float* w,
                                  const float* bias, int Co, int sd, int sh, int sw, int path, float* y, float* scratch,
                                  int64_t scratch_floats, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  Conv3dCall c;
  VAD_TRY(conv3d_call(0, path, layout, N, Ci, D, H, W, Co, sd, sh, sw, false, &c));
  VAD_CHECK(scratch && scratch_floats >= conv3d_min_scratch(0, c), "vad_conv3d_forward: scratch too small");
  const Strides5 str = layout == 0 ? ncdhw_strides(c.in) : ndhwc_strides(c.in);
  const int64_t wimg = up(27ll * Ci * Co);
  if (path == 0) {
    const int64_t cols = up(c.g.rows() * c.g.K());
    VAD_TRY(im2col3d(x, str, c.g, nullptr, nullptr, 0, scratch, st));
    return dense_fwd(scratch, (int)c.g.rows(), c.g.K(), w, bias, Co, y, DenseAct{}, scratch + cols,
                     scratch_floats - cols, st);
  }
  if (path == 1) {
    VAD_TRY(conv3d_direct_prep(w, Co, Ci, scratch, scratch + wimg, st));
    return conv3d_direct_fwd(x, str, c.in, scratch, Co, bias, y, st);
  }
  if (path == 2) {
    VAD_TRY(conv3s2_prep(w, Co, Ci, scratch, scratch + wimg, st));
    return conv3s2_fwd(x, N, D, H, W, Ci, scratch, bias, Co, 0, y, st, scratch + 2 * wimg, scratch_floats - 2 * wimg);
  }
  VAD_TRY(conv3d_prep_w3(w, Co, Ci, scratch, st));
  return conv3d_x3_fwd(N, D, H, W, Ci, Co, x, scratch, bias, y, st);
}

extern "C" int vad_conv3d_dgrad(const float* dy, int N, int Ci, int D, int H, int W, const float* w, int Co, int sd,
                                int sh, int sw, int path, const float* gate, float* dx, float* scratch,
                                int64_t scratch_floats, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  Conv3dCall c;
  VAD_TRY(conv3d_call(1, path, 1, N, Ci, D, H, W, Co, sd, sh, sw, gate != nullptr, &c));
  VAD_CHECK(scratch && scratch_floats >= conv3d_min_scratch(1, c), "vad_conv3d_dgrad: scratch too small");
  const int64_t wimg = up(27ll * Ci * Co);
  if (path == 0) {
    VAD_TRY(dense_dgrad(dy, (int)c.g.rows(), Co, w, c.g.K(), scratch, nullptr, 1.f, nullptr, st));
    return col2im3d(scratch, c.g, dx, st);
  }
  if (path == 1) {  // dX = conv(dY, flipped W^T) over the layer's input grid (stride 1: the output grid)
    VAD_TRY(conv3d_direct_prep(w, Co, Ci, scratch, scratch + wimg, st));
    const Vol5 vy{N, Co, D, H, W};
    return conv3d_direct_fwd(dy, ndhwc_strides(vy), vy, scratch + wimg, Ci, nullptr, dx, st);
  }
  VAD_TRY(conv3s2_prep(w, Co, Ci, scratch, scratch + wimg, st));
  return conv3s2_dgrad(dy, N, Co, scratch + wimg, Ci, dx, D, H, W, st, gate);
}

extern "C" int vad_conv3d_wgrad(const float* x, int layout, const float* dy, int N, int Ci, int D, int H, int W,
                                int Co, int sd, int sh, int sw, int path, float* dW, float* db, float* scratch,
                                int64_t scratch_floats, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  Conv3dCall c;
  VAD_TRY(conv3d_call(2, path, layout, N, Ci, D, H, W, Co, sd, sh, sw, false, &c));
  VAD_CHECK(scratch && scratch_floats >= conv3d_min_scratch(2, c), "vad_conv3d_wgrad: scratch too small");
  const Strides5 str = layout == 0 ? ncdhw_strides(c.in) : ndhwc_strides(c.in);
  if (path == 0) {
    VAD_CHECK(db, "vad_conv3d_wgrad: path 0 (im2col) writes db");
    const int64_t cols = up(c.g.rows() * c.g.K());
    VAD_TRY(im2col3d(x, str, c.g, nullptr, nullptr, 0, scratch, st));
    return dense_wgrad(dy, (int)c.g.rows(), Co, scratch, c.g.K(), dW, db, scratch + cols, scratch_floats - cols,
                       nullptr, st, 1024);
  }
  if (path == 1) return conv3d_direct_wgrad(dy, Co, x, str, c.in, dW, db, scratch, scratch_floats, st);
  return conv3s2_wgrad(dy, Co, x, Ci, N, D, H, W, dW, scratch, scratch_floats, 1024, st, db);
}

extern "C" int vad_maxpool3d_forward(const float* y, const float* stats, int relu, int N, int C, int D, int H, int W,
                                     int kd, int kh, int kw, float* out, void* stream) {
  VAD_CHECK(N >= 1 && C >= 1 && D >= 1 && H >= 1 && W >= 1 && kd >= 1 && kh >= 1 && kw >= 1,
            "vad_maxpool3d_forward: unsupported shape");
  return maxpool3d_fwd(y, stats, relu, Vol5{N, C, D, H, W}, kd, kh, kw, out, (hipStream_t)stream);
}

extern "C" int vad_maxpool3d_backward(const float* y, const float* stats, int relu, int N, int C, int D, int H, int W,
                                      int kd, int kh, int kw, const float* dout, float* dA, void* stream) {
  VAD_CHECK(N >= 1 && C >= 1 && D >= 1 && H >= 1 && W >= 1 && kd >= 1 && kh >= 1 && kw >= 1,
            "vad_maxpool3d_backward: unsupported shape");
  return maxpool3d_bwd(y, stats, relu, Vol5{N, C, D, H, W}, kd, kh, kw, dout, dA, (hipStream_t)stream);
}

extern "C" int vad_adaptive_avgpool3d_forward(const float* x, const float* stats, int relu, int N, int C, int D, int H,
                                              int W, int OD, int OH, int OW, float* out, void* stream) {
  VAD_CHECK(N >= 1 && C >= 1 && D >= 1 && H >= 1 && W >= 1 && OD >= 1 && OH >= 1 && OW >= 1,
            "vad_adaptive_avgpool3d_forward: unsupported shape");
  return adaptive_avgpool3d_fwd(x, stats, relu, Vol5{N, C, D, H, W}, OD, OH, OW, out, (hipStream_t)stream);
}

extern "C" int vad_adaptive_avgpool3d_backward(const float* dout, int N, int C, int D, int H, int W, int OD, int OH,
                                               int OW, const float* gate, float* dx, void* stream) {
  VAD_CHECK(N >= 1 && C >= 1 && D >= 1 && H >= 1 && W >= 1 && OD >= 1 && OH >= 1 && OW >= 1,
            "vad_adaptive_avgpool3d_backward: unsupported shape");
  return adaptive_avgpool3d_bwd(dout, Vol5{N, C, D, H, W}, OD, OH, OW, dx, (hipStream_t)stream, gate);
}

// ------------------------------------------------------------------------------------------------------------
// The dense-layer launchers and the fused MLP chain alone (backbone.h, mlp.h), with every argument the plans give
// them.  Thin wrappers: they fill the argument structs as the cad plan does and launch nothing of their own.
// ------------------------------------------------------------------------------------------------------------
namespace {

// the cad plan's act(): dropout after the activation, keyed by (seed, stream_id, step) and the global row
DenseAct dense_act(int relu, double p, uint64_t seed, uint32_t stream_id, uint64_t step, int64_t row0) {
  DenseAct a;
  a.relu = relu ? 1 : 0;
  if (p > 0) {
    a.drop = 1;
    a.h1 = rng_h1(seed, stream_id, step);
    a.thr = drop_threshold(p);
    a.dscale = 1.0f / (float)(1.0 - p);
    a.row0 = row0;
  }
  return a;
}

}  // namespace

extern "C" int vad_dense_forward_ex(const float* X, int M, int K, const float* W, const float* b, int N, float* Y,
                                    int relu, double drop_p, uint64_t seed, uint32_t stream_id, uint64_t step,
                                    int64_t row0, int max_splits, float* scratch, int64_t scratch_floats,
                                    void* stream) {
  VAD_CHECK(M >= 1 && K >= 1 && N >= 1 && drop_p >= 0 && drop_p < 1 && scratch_floats >= 0,
            "vad_dense_forward_ex: unsupported shape");
  return dense_fwd(X, M, K, W, b, N, Y, dense_act(relu, drop_p, seed, stream_id, step, row0), scratch, scratch_floats,
                   (hipStream_t)stream, max_splits);
}

extern "C" int vad_dense_dgrad(const float* dY, int M, int N, const float* W, int K, float* dX, const float* gate,
                               float gscale, int gate_rows, const int* skip, float* scratch, int64_t scratch_floats,
                               void* stream) {
  VAD_CHECK(M >= 1 && K >= 1 && N >= 1 && gate_rows >= 0 && scratch_floats >= 0, "vad_dense_dgrad: unsupported shape");
  return dense_dgrad(dY, M, N, W, K, dX, gate, gscale, skip, (hipStream_t)stream, gate_rows, scratch, scratch_floats);
}

extern "C" int vad_dense_wgrad(const float* dY, int M, int N, const float* X, int K, float* dW, float* db,
                               const int* skip, float* scratch, int64_t scratch_floats, int target_blocks,
                               void* stream) {
  VAD_CHECK(M >= 1 && K >= 1 && N >= 1 && target_blocks >= 1 && scratch_floats >= 0,
            "vad_dense_wgrad: unsupported shape");
  return dense_wgrad(dY, M, N, X, K, dW, db, scratch, scratch_floats, skip, (hipStream_t)stream, target_blocks);
}

extern "C" int vad_mlp_tail_forward(const float* X, int M, int K0, const int* N, const float* const* W,
                                    const float* const* b, const int* relu, const double* drop_p,
                                    const uint32_t* stream_id, uint64_t seed, uint64_t step, int64_t row0, int mode,
                                    float* const* out, float* scratch, int64_t scratch_floats, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  VAD_CHECK(M >= 1 && K0 >= 1 && (mode == 0 || mode == 1) && scratch_floats >= 0,
            "vad_mlp_tail_forward: unsupported shape");
  MlpTailArgs m{};
  m.M = M;
  m.row0 = row0;
  DenseAct a0;
  for (int i = 0; i < 5; ++i) {
    VAD_CHECK(N[i] >= 1 && drop_p[i] >= 0 && drop_p[i] < 1, "vad_mlp_tail_forward: unsupported shape");
    const DenseAct a = dense_act(relu[i], drop_p[i], seed, stream_id[i], step, row0);
    if (i == 0) a0 = a;
    MlpLayer& L = m.L[i];
    L.W = W[i];
    L.b = b[i];
    L.out = out[i];
    L.K = i == 0 ? K0 : N[i - 1];
    L.N = N[i];
    L.relu = a.relu;
    L.drop = a.drop;
    L.h1 = a.h1;
    L.thr = a.thr;
    L.dscale = a.dscale;
  }
  VAD_TRY(mlp_tail_fwd_check(m));  // before anything is queued: a refused chain launches nothing
  // the transposed weights of layers 1-4 first, the split-K slabs in what is left
  MlpTransposeArgs t{};
  int64_t off = 0;
  for (int i = 1; i < 5; ++i, ++t.n) {
    m.WT[i] = scratch + off;
    t.W[t.n] = W[i];
    t.WT[t.n] = scratch + off;
    t.K[t.n] = m.L[i].K;
    t.N[t.n] = m.L[i].N;
    off += up((int64_t)m.L[i].K * m.L[i].N);
  }
  VAD_CHECK(scratch && off <= scratch_floats, "vad_mlp_tail_forward: scratch too small");
  VAD_TRY(mlp_transpose(t, st));
  if (mode == 0) {
    VAD_TRY(dense_fwd(X, M, K0, W[0], b[0], N[0], out[0], a0, scratch + off, scratch_floats - off, st));
  } else {
    int ns = 0;
    VAD_TRY(dense_fwd_splitk(X, M, K0, W[0], N[0], scratch + off, scratch_floats - off, &ns, st));
    m.parts = scratch + off;
    m.nsplit = ns;
  }
  return mlp_tail_fwd(m, st);
}

extern "C" int vad_mlp_tail_backward(int M, const float* dout, const float* const* W, const int* K, const int* N,
                                     const float* const* h, const float* gscale, float* const* d, const int* skip,
                                     void* stream) {
  VAD_CHECK(M >= 1, "vad_mlp_tail_backward: unsupported shape");
  MlpTailBwdArgs a{};
  a.M = M;
  a.dout = dout;
  for (int i = 0; i < 5; ++i) {
    a.W[i] = W[i];
    a.K[i] = K[i];
    a.N[i] = N[i];
    VAD_CHECK(K[i] >= 1 && N[i] >= 1 && (i == 0 || K[i] == N[i - 1]), "vad_mlp_tail_backward: unsupported shape");
  }
  for (int i = 0; i < 4; ++i) {
    a.h[i] = h[i];
    a.gscale[i] = gscale[i];
    a.d[i] = d[i];
  }
  a.skip = skip;
  return mlp_tail_bwd(a, (hipStream_t)stream);
}

extern "C" int vad_rows_wgrad(int R, int nseg, float* const* dW, float* const* db, const float* const* A,
                              const float* const* X, const int* O, const int* I, const int* skip, void* stream) {
  RowsWgradArgs a{};
  a.R = R;
  a.nseg = nseg;  // (a count outside 1 .. ROWS_WGRAD_MAXSEG is the launcher's to refuse)
  for (int s = 0; s < nseg && s < ROWS_WGRAD_MAXSEG; ++s) {
    VAD_CHECK(R >= 1 && O[s] >= 1 && I[s] >= 1, "vad_rows_wgrad: unsupported shape");
    a.seg[s] = RowsWgradSeg{dW[s], db ? db[s] : nullptr, A[s], X[s], O[s], I[s]};
  }
  a.skip = skip;
  return rows_wgrad(a, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------------------
// The causal head alone (head.h): head_fwd, and head_bwd + head_slab_reduce + head_rows_wgrad in the plan's order, on
// logits the caller chose.  Thin wrappers: HeadArgs comes from cad_head_args, the function the plan fills its own
// with; rows, per-clip workspaces and gradient slabs are carved from the caller's scratch; they launch nothing of
// their own.
// ------------------------------------------------------------------------------------------------------------
namespace {

struct HeadScratch {
  int64_t rows, ws, iws, slabs, total;
  HeadScratch(int B, int T) {
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t r = o; o += up(n); return r; };
    rows = take(head_rows_floats(B, T));
    ws = take((int64_t)B * head_ws_floats(T));
    iws = take((int64_t)B * head_iws_ints(T));  // ints, one float's size each
    slabs = take((int64_t)B * cad_head_slab_len());
    total = o;
  }
};

int head_call(const char* who, int B, int T, int training, const void* logits, const void* params, const float* scratch,
              int64_t scratch_floats) {
  const std::string w(who);
  VAD_CHECK(B >= 1 && T >= 1 && T <= 4096 && (int64_t)B * T * NMAX < (1ll << 24) && (training == 0 || training == 1),
            w + ": unsupported shape");
  VAD_CHECK(logits && params, w + ": null argument");
  VAD_CHECK(scratch && scratch_floats >= HeadScratch(B, T).total, w + ": scratch too small");
  VAD_CHECK(reinterpret_cast<uintptr_t>(scratch) % 16 == 0 && reinterpret_cast<uintptr_t>(params) % 16 == 0,
            w + ": params and scratch must be 16-byte aligned");
  return 0;
}

HeadArgs head_call_args(int B, int T, int training, uint64_t seed, uint64_t step, int64_t clip0, const float* params,
                        float* grads, float* scratch) {
  const HeadScratch s(B, T);
  return cad_head_args(B, T, clip0, training, seed, step, params, grads, scratch + s.ws,
                       reinterpret_cast<int*>(scratch + s.iws), scratch + s.rows);
}

}  // namespace

extern "C" int64_t vad_head_scratch_floats(int B, int T) {
  if (B < 1 || T < 1 || T > 4096 || (int64_t)B * T * NMAX >= (1ll << 24)) {
    set_error("vad_head_scratch_floats: unsupported shape");
    return -1;
  }
  return HeadScratch(B, T).total;
}

extern "C" int vad_head_forward(const float* det_logits, int B, int T, const float* params, int training, uint64_t seed,
                                uint64_t step, int64_t clip0, float* causal, float* kl, float* z, float* adj,
                                float* boxes, int* counts, int* nmax, int* clip_flags, float* scratch,
                                int64_t scratch_floats, void* stream) {
  VAD_TRY(head_call("vad_head_forward", B, T, training, det_logits, params, scratch, scratch_floats));
  VAD_CHECK(causal && kl && z && adj && boxes && counts && nmax && clip_flags, "vad_head_forward: null argument");
  const HeadArgs a = head_call_args(B, T, training, seed, step, clip0, params, nullptr, scratch);
  return head_fwd(a, det_logits, HeadOut{causal, kl, z, adj, boxes, counts, nmax, clip_flags}, (hipStream_t)stream);
}

extern "C" int vad_head_backward(const float* det_logits, int B, int T, const float* params, int training,
                                 uint64_t seed, uint64_t step, int64_t clip0, float* causal, float* kl, float* z,
                                 float* adj, float* boxes, int* counts, int* nmax, int* clip_flags,
                                 const float* d_causal, const float* d_kl, const float* d_z, const float* d_adj,
                                 const float* d_boxes, float* grads, float* d_det_logits, float* scratch,
                                 int64_t scratch_floats, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  VAD_TRY(head_call("vad_head_backward", B, T, training, det_logits, params, scratch, scratch_floats));
  VAD_CHECK(causal && kl && z && adj && boxes && counts && nmax && clip_flags && d_causal && d_kl && grads &&
                d_det_logits,
            "vad_head_backward: null argument");
  const HeadArgs a = head_call_args(B, T, training, seed, step, clip0, params, grads, scratch);
  float* slabs = scratch + HeadScratch(B, T).slabs;
  const int64_t slab_len = cad_head_slab_len();
  VAD_TRY(head_bwd(a, det_logits, HeadOut{causal, kl, z, adj, boxes, counts, nmax, clip_flags},
                   HeadUp{d_causal, d_kl, d_z, d_adj, d_boxes}, slabs, slab_len, d_det_logits, st));
  VAD_TRY(head_slab_reduce(slabs, B, slab_len, grads + cad_head_grad_begin(), st));
  return head_rows_wgrad(a, st);
}
