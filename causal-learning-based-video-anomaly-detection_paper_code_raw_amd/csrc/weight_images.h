// The derived weight images of the cad plan and the one store routine that writes them: the 3x3 convs' forward
// image Wf, input-gradient image Wd (plain or the four concatenated stride-2 parity-class images), the pre-split
// bf16 planes of Wd, the bf16 copies behind Wf / Wd, and the detector's transposed layers.  Both writers -- the
// relayout kernels (conv3_prep_all_kernel, mlp_transpose_kernel) and the fused optimizer (adamw_kernel) -- go through
// these functions, so an image is bit-identical whichever kernel wrote it.
#pragma once
#include "common.h"

namespace vad {

struct PrepTab {
  const float* w[8];
  float* wf[8];
  float* wd[8];
  __bf16* w3[8];  // nullable: pre-split bf16 planes of Wd, [ci][tap][co / 16][3][16]
  int Ci[8], Co[8], classes[8];
  int64_t end[8];  // inclusive prefix sums of Co*Ci*9
  int n;
  int bf16;  // also the bf16 copies of the plain images (conv3_bf16_image: behind the fp32 image)
};

// element i (torch layout [Co][Ci][3][3]) of layer l's weight, value v, into every image of that layer
__device__ inline void conv3_image_store(const PrepTab& t, int l, int64_t i, float v) {
  const int Ci = t.Ci[l], Co = t.Co[l];
  const uint32_t e = (uint32_t)i;  // (a layer has < 2^20 weights: 32-bit divisions)
  const int tap = (int)(e % 9u);
  const int ci = (int)((e / 9u) % (uint32_t)Ci);
  const int co = (int)(e / (9u * (uint32_t)Ci));
  t.wf[l][((int64_t)co * 9 + tap) * Ci + ci] = v;
  if (t.bf16) {
    const int64_t tot = (int64_t)Co * Ci * 9;
    reinterpret_cast<__bf16*>(t.wf[l] + tot)[((int64_t)co * 9 + tap) * Ci + ci] = (__bf16)v;
    reinterpret_cast<__bf16*>(t.wd[l] + tot)[((int64_t)ci * 9 + tap) * Co + co] = (__bf16)v;
  }
  if (t.w3[l]) {  // (the split of put_planes / split3: hi, mid, lo)
    const __bf16 h = (__bf16)v;
    const float r = v - (float)h;
    const __bf16 m = (__bf16)r;
    __bf16* d = t.w3[l] + ((((int64_t)ci * 9 + tap) * (Co / 16) + co / 16) * 3) * 16 + co % 16;
    d[0] = h;
    d[16] = m;
    d[32] = (__bf16)(r - (float)m);
  }
  if (!t.classes[l]) {
    t.wd[l][((int64_t)ci * 9 + tap) * Co + co] = v;
  } else {
    // class (ph,pw): kh valid iff (ph+1-kh) even -> ph = (kh+1)&1; its index among the class's row taps
    const int kh = tap / 3, kw = tap % 3;
    const int ph = (kh + 1) & 1, pw = (kw + 1) & 1;
    const int ri = (ph == 0) ? 0 : (kh == 0 ? 0 : 1);
    const int cj = (pw == 0) ? 0 : (kw == 0 ? 0 : 1);
    const int nrt = ph == 0 ? 1 : 2, nct = pw == 0 ? 1 : 2;
    int64_t off = 0;  // classes in order (0,0),(0,1),(1,0),(1,1)
    for (int c = 0; c < ph * 2 + pw; ++c) {
      const int r = (c >> 1) == 0 ? 1 : 2, q = (c & 1) == 0 ? 1 : 2;
      off += (int64_t)r * q * Ci * Co;
    }
    t.wd[l][off + ((int64_t)ci * (nrt * nct) + ri * nct + cj) * Co + co] = v;
  }
}

// WT[k][n] = W[n][k] for up to 8 matrices (the detector's layer-1..4 weights)
struct MlpTransposeArgs {
  int n;
  const float* W[8];
  float* WT[8];
  int K[8], N[8];
};

__device__ inline void mlp_wt_store(const MlpTransposeArgs& a, int m, int n, int k, float v) {
  a.WT[m][(int64_t)k * a.N[m] + n] = v;
}
// the same by element index i of W (torch layout [N][K])
__device__ inline void mlp_wt_store(const MlpTransposeArgs& a, int m, int64_t i, float v) {
  const uint32_t K = (uint32_t)a.K[m], e = (uint32_t)i;
  mlp_wt_store(a, m, (int)(e / K), (int)(e % K), v);
}

// what the fused optimizer needs to keep the images current: the two tables above and, per parameter slot, the image
// it feeds (0..7: conv layer; 8 + j: entry j of the transpose table; -1: none)
struct WeightImages {
  PrepTab conv;
  MlpTransposeArgs det;
  int64_t off[16], numel[16];  // per image: its slot's offset in the flat parameter buffer and element count
  int8_t slot_img[160];
};

__device__ inline void weight_image_store(const WeightImages& w, int slot, int64_t i /* index in the flat buffer */,
                                          float v) {
  const int im = w.slot_img[slot];
  if (im < 0) return;
  const int64_t e = i - w.off[im];
  if (e >= w.numel[im]) return;  // (the padding of the slot's last 256-float chunk)
  if (im < 8) conv3_image_store(w.conv, im, e, v);
  else mlp_wt_store(w.det, im - 8, e, v);
}

}  // namespace vad
