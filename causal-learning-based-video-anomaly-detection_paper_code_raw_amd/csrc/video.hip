// Sliding-window scoring of a video with CausalAnomalyDetector in eval mode (include/vad.h: vad_cad_frames_forward /
// vad_cad_windows_forward).  With running BatchNorm statistics everything up to the GRU input projection depends on the
// frame alone, so the per-frame stage of the forward runs once per frame and leaves its results in a frame cache; a
// window then reads frames start + t of the cache.  This file: the cache's store kernel and the per-window mean of
// the pooled features; the windowed sequence kernel shares its body with the clip kernel (head.hip).  For a live
// stream (vad_cad_frames_forward_ring / vad_cad_windows_forward_ring) the same cache is a ring: frame g, counted from
// the start of the stream, lives in slot g mod nframes, and both kernels here have a RING form beside the linear one.
// For a group of streams (vad_cad_frames_forward_group / vad_cad_windows_forward_group) one cache holds many rings of
// cap slots each, and both kernels have a TABLE form: a block reads where it stores, or which ring it sums, from a
// device table the host validated (cad_plan.hip) -- the kernels themselves check nothing.
#include "../../include/vad.h"
#include "head.h"

namespace vad {

constexpr int FEAT = 6144;  // 256 channels x (4, 6) bins (cad:560-566)
constexpr int G3V = 3 * GH;
static_assert(FEAT % 4 == 0 && (NMAX * G3V) % 4 == 0 && (NMAX * 4) % 4 == 0, "float4 copies");

// One block per frame f = b*T + t of the chunk: its features, its five projection rows and its boxes as float4s, its
// count and slots as words, to frame frame0 + f of the cache.  RING: to slot (frame0 + f) mod nframes, with
// frame0 < nframes already reduced on the host and at most nframes frames in the chunk, so one conditional subtract.
// TABLE: block f stores to slot dst[f] of the cache, or, where dst[f] < 0, returns before any load (a padding frame);
// dst[f] is block-uniform, so it is one scalar load.
template <bool RING, bool TABLE = false>
__global__ __launch_bounds__(256) void frame_cache_store_kernel(const float* __restrict__ feats,
                                                                const float* __restrict__ gi,
                                                                const float* __restrict__ boxes,
                                                                const int* __restrict__ counts,
                                                                const int* __restrict__ iws, int64_t iws_stride, int T,
                                                                float* __restrict__ cache, int64_t nframes,
                                                                int64_t frame0, const int* __restrict__ dst) {
  static_assert(!(RING && TABLE), "a table names absolute slots");
  const int f = blockIdx.x, tid = threadIdx.x;
  const int b = f / T, t = f - b * T;
  const FrameCache C(nframes);
  int64_t g = frame0 + f;
  if constexpr (RING) {
    if (g >= nframes) g -= nframes;
  }
  if constexpr (TABLE) {
    g = dst[f];
    if (g < 0) return;
  }
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
                      int64_t frame0, hipStream_t st, bool ring) {
  const int64_t nf = (int64_t)a.B * a.T;
  VAD_CHECK(nframes >= 1 && frame0 >= 0 && (ring ? nf <= nframes : frame0 + nf <= nframes),
            "frame cache: frames outside the cache");
  VAD_CHECK((reinterpret_cast<uintptr_t>(cache) & 15) == 0, "frame cache: the cache must be 16-B aligned");
  const float* gi = a.rows + head_rows_gi_offset(a.B, a.T);
  if (ring)
    VAD_KLAUNCH(frame_cache_store_kernel<true>, dim3((unsigned)nf), dim3(256), 0, st, feats, gi, o.boxes, o.counts,
                a.iws, a.iws_stride, a.T, cache, nframes, frame0 % nframes, (const int*)nullptr);
  else
    VAD_KLAUNCH(frame_cache_store_kernel<false>, dim3((unsigned)nf), dim3(256), 0, st, feats, gi, o.boxes, o.counts,
                a.iws, a.iws_stride, a.T, cache, nframes, frame0, (const int*)nullptr);
  VAD_LAUNCH_CHECK();
  return 0;
}

int frame_cache_store_group(const HeadArgs& a, const HeadOut& o, const float* feats, float* cache, int64_t total_slots,
                            const int* dst, hipStream_t st) {
  const int64_t nf = (int64_t)a.B * a.T;
  VAD_CHECK(total_slots >= 1 && dst != nullptr, "frame cache: no destination table");
  VAD_CHECK((reinterpret_cast<uintptr_t>(cache) & 15) == 0, "frame cache: the cache must be 16-B aligned");
  const float* gi = a.rows + head_rows_gi_offset(a.B, a.T);
  VAD_KLAUNCH((frame_cache_store_kernel<false, true>), dim3((unsigned)nf), dim3(256), 0, st, feats, gi, o.boxes,
              o.counts, a.iws, a.iws_stride, a.T, cache, total_slots, (int64_t)0, dst);
  VAD_LAUNCH_CHECK();
  return 0;
}

// pooled[i][k] of window i (frames first + i * stride + t): thread = one float4 of columns, the window's T frames
// summed in ascending t from 0.f and divided by T -- the sum avgpool_fwd_kernel forms for a clip (pool += f;
// pool / T), so the direct classifier reads the number the clip path gives it.  A warp's loads are 1 KB contiguous;
// the loop is unrolled so several frames' loads are in flight per thread (the adds stay in order).  RING: row t is
// slot (first + i * stride + t) mod nframes -- one modulo per thread, then increment and wrap -- and the sum is
// the same one.  TABLE (with RING): the cache holds nframes / cap rings of cap slots; block row i reads its entry
// (base_i, s0_i, key_i) of the window table (block-uniform: scalar loads) and sums slots base_i + (s0_i + t, wrapped
// once at cap) -- the ring form's loop on a ring that starts at slot base_i.
template <bool RING, bool TABLE = false>
__global__ __launch_bounds__(256) void window_mean_kernel(const float* __restrict__ cache, int64_t nframes, int T,
                                                          int stride, int64_t first, float* __restrict__ pooled,
                                                          const int64_t* __restrict__ tab, int tab_cap) {
  static_assert(RING || !TABLE, "the table form addresses rings");
  const int i = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;  // c < FEAT / 4 (the grid covers it exactly)
  const FrameCache C(nframes);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if constexpr (RING) {
    const f32x4* src = reinterpret_cast<const f32x4*>(cache + C.feats) + c;
    int cap, sl;
    if constexpr (TABLE) {
      src += tab[3 * i] * (FEAT / 4);
      cap = tab_cap;
      sl = (int)tab[3 * i + 1];
    } else {
      cap = (int)nframes;
      sl = (int)((first + (int64_t)i * stride) % nframes);
    }
#pragma unroll 8
    for (int t = 0; t < T; ++t) {
      s += src[(int64_t)sl * (FEAT / 4)];
      if (++sl == cap) sl = 0;
    }
  } else {
    const f32x4* src = reinterpret_cast<const f32x4*>(cache + C.feats + (first + (int64_t)i * stride) * FEAT) + c;
#pragma unroll 8
    for (int t = 0; t < T; ++t) s += src[(int64_t)t * (FEAT / 4)];
  }
  const float fT = (float)T;
  reinterpret_cast<f32x4*>(pooled + (int64_t)i * FEAT)[c] = f32x4{s[0] / fT, s[1] / fT, s[2] / fT, s[3] / fT};
}

int window_mean(const float* cache, int64_t nframes, int T, int stride, int64_t first, int nw, float* pooled,
                hipStream_t st, bool ring) {
  // (ring: the batch's span fits the ring, so no slot is read as two different frames)
  VAD_CHECK(T >= 1 && stride >= 1 && first >= 0 && nw >= 1 &&
                (ring ? 0 : first) + (int64_t)(nw - 1) * stride + T <= nframes && nframes < (1ll << 31),
            "window_mean: windows outside the cache");
  const dim3 grid(FEAT / 4 / 256, (unsigned)nw);
  const int64_t* no_tab = nullptr;
  if (ring)
    VAD_KLAUNCH(window_mean_kernel<true>, grid, dim3(256), 0, st, cache, nframes, T, stride, first, pooled, no_tab, 0);
  else
    VAD_KLAUNCH(window_mean_kernel<false>, grid, dim3(256), 0, st, cache, nframes, T, stride, first, pooled, no_tab, 0);
  VAD_LAUNCH_CHECK();
  return 0;
}

int window_mean_group(const float* cache, int64_t total_slots, int cap, int T, const int64_t* tab, int nw,
                      float* pooled, hipStream_t st) {
  VAD_CHECK(tab != nullptr && nw >= 1 && cap >= 1 && T >= 1 && T <= cap && cap <= total_slots &&
                total_slots < (1ll << 31),
            "window_mean: windows outside the cache");
  const dim3 grid(FEAT / 4 / 256, (unsigned)nw);
  VAD_KLAUNCH((window_mean_kernel<true, true>), grid, dim3(256), 0, st, cache, total_slots, T, 1, (int64_t)0, pooled,
              tab, cap);
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
