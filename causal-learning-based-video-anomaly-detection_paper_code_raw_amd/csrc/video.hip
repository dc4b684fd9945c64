// Sliding-window scoring of a video with CausalAnomalyDetector in eval mode (include/vad.h: vad_cad_frames_forward /
// vad_cad_windows_forward).  With running BatchNorm statistics everything up to the GRU input projection depends on the
// frame alone, so the per-frame stage of the forward runs once per frame and leaves its results in a frame cache; a
// window then reads T frames of the cache.  This file: the cache's store kernel and the per-window mean of the pooled
// features; the windowed sequence kernel shares its body with the clip kernel (head.hip).  The cache is a video's
// (linear), one live stream's ring or a group of rings; both kernels take the form as a WinForm and find their frames
// through win_rows.h.
#include "../../include/vad.h"
#include "head.h"

namespace vad {

constexpr int FEAT = 6144;  // 256 channels x (4, 6) bins (cad:560-566)
constexpr int G3V = 3 * GH;
static_assert(FEAT % 4 == 0 && (NMAX * G3V) % 4 == 0 && (NMAX * 4) % 4 == 0, "float4 copies");

// One block per frame f = b*T + t of the chunk: its features, its five projection rows and its boxes as float4s, its
// count and slots as words, to slot frame_slot<F>(f) of the cache (win_rows.h); a padding frame of a group returns
// before any load.
template <WinForm F>
__global__ __launch_bounds__(256) void frame_cache_store_kernel(const float* __restrict__ feats,
                                                                const float* __restrict__ gi,
                                                                const float* __restrict__ boxes,
                                                                const int* __restrict__ counts,
                                                                const int* __restrict__ iws, int64_t iws_stride, int T,
                                                                float* __restrict__ cache, int64_t nframes,
                                                                int frame0, const int* __restrict__ dst) {
  const int f = blockIdx.x, tid = threadIdx.x;
  const int b = f / T, t = f - b * T;
  const FrameCache C(nframes);
  const int64_t g = frame_slot<F>(f, frame0, (int)nframes, dst);
  if (F == WinForm::Group && g < 0) return;
  const f32x4* sf = reinterpret_cast<const f32x4*>(feats + (int64_t)f * FEAT);
  f32x4* df = reinterpret_cast<f32x4*>(cache + C.feats + g * FEAT);
  // (6 loads in flight per thread before the first store)
  f32x4 v[FEAT / 4 / 256];
#pragma unroll
  for (int k = 0; k < FEAT / 4 / 256; ++k) v[k] = sf[k * 256 + tid];
#pragma unroll
  for (int k = 0; k < FEAT / 4 / 256; ++k) df[k * 256 + tid] = v[k];
  if (tid < NMAX * G3V / 4)
    reinterpret_cast<f32x4*>(cache + C.gi + g * NMAX * G3V)[tid] =
        reinterpret_cast<const f32x4*>(gi + (int64_t)f * NMAX * G3V)[tid];
  if (tid < NMAX)
    reinterpret_cast<f32x4*>(cache + C.boxes + g * NMAX * 4)[tid] =
        reinterpret_cast<const f32x4*>(boxes + (int64_t)f * NMAX * 4)[tid];
  int* ci = reinterpret_cast<int*>(cache);
  if (tid == 64) ci[C.counts + g] = counts[f];
  if (tid >= 128 && tid < 128 + NMAX) {
    const int j = tid - 128;
    ci[C.slot + g * NMAX + j] = iws[(int64_t)b * iws_stride + T + t * NMAX + j];
  }
}
static_assert(FEAT / 4 % 256 == 0 && NMAX * G3V / 4 <= 256, "frame_cache_store_kernel: thread roles");

int frame_cache_store(const HeadArgs& a, const HeadOut& o, const float* feats, float* cache, int64_t nframes,
                      WinForm form, int64_t frame0, const int* dst, hipStream_t st) {
  const int64_t nf = (int64_t)a.B * a.T;
  if (form == WinForm::Group) {
    VAD_CHECK(nframes >= 1 && nframes < (1ll << 31) && dst != nullptr, "frame cache: no destination table");
    frame0 = 0;
  } else {
    VAD_CHECK(nframes >= 1 && nframes < (1ll << 31) && frame0 >= 0 &&
                  (form == WinForm::Ring ? nf <= nframes : frame0 + nf <= nframes),
              "frame cache: frames outside the cache");
    if (form == WinForm::Ring) frame0 %= nframes;  // (the kernel wraps once)
  }
  VAD_CHECK((reinterpret_cast<uintptr_t>(cache) & 15) == 0, "frame cache: the cache must be 16-B aligned");
  const float* gi = a.rows + head_rows_gi_offset(a.B, a.T);
  win_dispatch(form, [&](auto F) {
    VAD_KLAUNCH(frame_cache_store_kernel<F()>, dim3((unsigned)nf), dim3(256), 0, st, feats, gi, o.boxes, o.counts,
                a.iws, a.iws_stride, a.T, cache, nframes, (int)frame0, dst);
  });
  VAD_LAUNCH_CHECK();
  return 0;
}

// pooled[i][k] of window i: thread = one float4 of columns, the window's T frames (rows WinCursor<F>(win, i) of the
// cache's features) summed in ascending t from 0.f and divided by T -- the sum avgpool_fwd_kernel forms for a clip
// (pool += f; pool / T), so the direct classifier reads the number the clip path gives it.  A warp's loads are 1 KB
// contiguous; the loop is unrolled so several frames' loads are in flight per thread (the adds stay in order).
template <WinForm F>
__global__ __launch_bounds__(256) void window_mean_kernel(const float* __restrict__ cache, int64_t nframes, int T,
                                                          const WinRows win, float* __restrict__ pooled) {
  const int i = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;  // c < FEAT / 4 (the grid covers it exactly)
  const FrameCache C(nframes);
  const WinCursor<F> cur(win, i);
  const f32x4* src = reinterpret_cast<const f32x4*>(cache + C.feats + cur.base * FEAT) + c;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int t = 0; t < T; ++t) s += src[(int64_t)cur.row(t) * (FEAT / 4)];
  const float fT = (float)T;
  reinterpret_cast<f32x4*>(pooled + (int64_t)i * FEAT)[c] = f32x4{s[0] / fT, s[1] / fT, s[2] / fT, s[3] / fT};
}

int window_mean(const float* cache, int64_t nframes, int T, WinForm form, const WinRows& win, int nw, float* pooled,
                hipStream_t st) {
  if (form == WinForm::Group) {
    VAD_CHECK(win.tab != nullptr && win.words >= 2 && nw >= 1 && win.cap >= 1 && T >= 1 && T <= win.cap &&
                  win.cap <= nframes && nframes < (1ll << 31),
              "window_mean: windows outside the cache");
  } else {  // (ring: the batch's span fits the ring, so no slot is read as two different frames)
    VAD_CHECK(T >= 1 && win.stride >= 1 && win.first >= 0 && nw >= 1 &&
                  (form == WinForm::Ring ? 0 : win.first) + (int64_t)(nw - 1) * win.stride + T <= nframes &&
                  nframes < (1ll << 31) && (form == WinForm::Linear || win.cap == nframes),
              "window_mean: windows outside the cache");
  }
  win_dispatch(form, [&](auto F) {
    VAD_KLAUNCH(window_mean_kernel<F()>, dim3(FEAT / 4 / 256, (unsigned)nw), dim3(256), 0, st, cache, nframes, T, win,
                pooled);
  });
  VAD_LAUNCH_CHECK();
  return 0;
}

}  // namespace vad

extern "C" {

int64_t vad_cad_frame_cache_floats(int64_t nframes) {
  if (nframes < 1 || nframes > (1ll << 40)) {
    vad::set_error("vad_cad_frame_cache_floats: nframes must be >= 1");
    return -1;
  }
  return vad::FrameCache(nframes).total;
}

int64_t vad_cad_frame_cache_offset(int64_t nframes, int field) {
  if (nframes < 1 || nframes > (1ll << 40) || field < 0 || field > 4) {
    vad::set_error("vad_cad_frame_cache_offset: nframes must be >= 1 and field in 0..4");
    return -1;
  }
  const vad::FrameCache C(nframes);
  const int64_t off[5] = {C.feats, C.gi, C.boxes, C.counts, C.slot};
  return off[field];
}

}  // extern "C"
