// Host data path: u8 frames staged in pinned host memory are copied to HBM as u8 (a quarter of
// the fp32 bytes over PCIe) and turned into the model's fp32 clip tensor on the device; frame resizing on the host.
//   vad_u8_to_clip  : dst = (u8 - 0.5) / 0.5   (mode 0: cad's Normalize([0.5],[0.5]) over raw 0..255 pixels,
//                                                causal_anomaly_detection.py:92-96, 1177-1179)
//                     dst = u8 / 255           (mode 1: ToTensor range, minicausal:120, bbox:409-411)
//                     -- the same float expressions as the synthetic-clip generator (bit-identical results)
//   vad_host_device_ptr: the device address of pinned (page-locked, mapped) host memory, so vad_u8_to_clip can read a
//                     staged batch straight over PCIe (ClipStager's direct mode: no copy engine, no u8 device slot)
//   vad_resize_u8   : bilinear resize with half-pixel centres, border clamping and 11-bit fixed-point weights
//                     (the scheme of cv2.resize INTER_LINEAR on u8 images that UCSDped2Dataset.__getitem__ calls,
//                     cad:88-89; restated from its published algorithm, cv2 itself is absent here: parity unpinned
//                     except for the identity case, which UCSD Ped2's native 360x240 frames hit)
//   vad_ingest_u8 / vad_ingest_u8_table: the scoring side's ingest: u8 frames at the source's own size
//                     and row pitch, in HBM or mapped host memory -> vad_resize_u8's pixel -> the normalisation ->
//                     fp32 (nf, 1, dh, dw), in one launch; bit for bit the host routine followed by u8_pixel
//   vad_ingest_u8_color / _table: the same launch on packed colour pixels: PIL's luma of every source
//                     tap (grey out), or the three channels as planes R, G, B (the bbox scorer's input)
//   vad_luma_u8     : that luma on the host, the other side of the equality
#include <math.h>

#include <algorithm>
#include <vector>

#include "../../include/vad.h"
#include "common.h"

namespace vad {

typedef unsigned u32x4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float u8_pixel(uint32_t u, int mode) {
  const float f = (float)u;
  return mode == 0 ? (f - 0.5f) / 0.5f : f / 255.f;
}

// 16 pixels per lane and iteration (one 16-B load, four 16-B stores): the source may be pinned host memory read over
// PCIe (vad_host_device_ptr), where wide requests matter; n16 = n / 16 full groups, the tail pixel by pixel
__global__ __launch_bounds__(256) void u8_to_clip_kernel(const uint8_t* __restrict__ src, int64_t n, int mode,
                                                         float* __restrict__ dst) {
  const int64_t n16 = n / 16;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) {
    const u32x4d w = reinterpret_cast<const u32x4d*>(src)[i];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = u8_pixel((w[q] >> (8 * e)) & 0xffu, mode);
      reinterpret_cast<f32x4*>(dst)[4 * i + q] = o;
    }
  }
  for (int64_t i = n16 * 16 + blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    dst[i] = u8_pixel(src[i], mode);
}


// ---------------------------------------------------------------- ingest: resize + normalise in one launch
// mode 2: the autoencoder dataset's /255 then clamp(0.001, 0.999) (cad1:110-114); modes 0 and 1 are u8_pixel's
__device__ __forceinline__ float ingest_pixel(uint32_t u, int mode) {
  return mode == 2 ? fminf(fmaxf((float)u / 255.f, 0.001f), 0.999f) : u8_pixel(u, mode);
}

// packed colour formats: 0 rgb, 1 bgr (3 bytes a pixel), 2 rgbx, 3 bgrx (4 bytes, X never read); G is byte 1 in all
__host__ __device__ __forceinline__ int ingest_step(int fmt) { return fmt >= 2 ? 4 : 3; }
__host__ __device__ __forceinline__ int ingest_r(int fmt) { return (fmt & 1) ? 2 : 0; }
__host__ __device__ __forceinline__ int ingest_b(int fmt) { return (fmt & 1) ? 0 : 2; }
// PIL's convert("L") (ITU-R 601-2 in 16-bit fixed point; the coefficients sum to 65536)
__host__ __device__ __forceinline__ int luma_u8(int r, int g, int b) {
  return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16;
}

constexpr int INGEST_ONE = 2048;      // vad_resize_u8's ONE
constexpr int INGEST_MAX_DW = 4096;   // columns of the LDS column table (32 KB): the bound on dw
constexpr int INGEST_MAX_ROWS = 32;   // output rows of one block
constexpr int INGEST_ITEMS = 512;     // four-pixel groups a block aims at (two per thread)

// One entry of vad_resize_u8's table(): the source index of destination index d and its two 11-bit weights, packed
// c0 | c1 << 16 (both <= 2048).  The host rounds (d + 0.5) * scale and the subtraction separately; hipcc contracts
// device code by default and an fma would round once, moving f by an ulp and a weight by one: contraction is off for
// this block.  The double division is IEEE on gfx950, as on the host.
__device__ __forceinline__ void resize_tap(int d, int sn, int dn, int& ofs, uint32_t& w) {
#pragma clang fp contract(off)
  const double scale = (double)sn / dn;
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) {
    f = 0.f;
    s = 0;
  }
  if (s >= sn - 1) {
    f = 0.f;
    s = sn - 1;
  }
  ofs = s;
  w = (uint32_t)(int)lrintf((1.f - f) * INGEST_ONE) | (uint32_t)(int)lrintf(f * INGEST_ONE) << 16;
}

// A block writes `rows` output rows of one frame: blockIdx.x = frame * strips + strip.  It builds the 256-entry pixel
// table (the normalisation has 256 possible inputs: no division per pixel), the column table of all dw columns and
// the row table of its rows in LDS, then each lane takes groups of four neighbouring pixels of a row.
// TABLE: frame f reads (address, sh, sw, pitch) from row f of the device table, address 0 = a frame of zeros
// (block-uniform: scalar loads); otherwise all frames share one size and lie frame_stride bytes apart.
// Integer widths: the host's int64 is not needed -- a horizontal sum is at most 255 * 2049 (the two weights sum to
// 2048, 2049 where both round up), the vertical one at most 2049 * 255 * 2048 + 2^21 = 1,072,169,984 < 2^31.
// Stores: a row of dw floats starts 16-byte aligned only where dw (and for later frames dh * dw) allows, so a group
// is stored as one f32x4 where its address is aligned and all four pixels exist, pixel by pixel otherwise.
// PLANES 0: grey source bytes, the form above.  PLANES 1 and 3: packed colour pixels of fmt (ingest_step bytes each, R
// and B at ingest_r / ingest_b, G at 1; an X byte is never loaded), read byte by byte -- rows have no alignment and a
// pixel of 3 bytes none either.  1: each of the four taps becomes its luma first, then the grey blend runs on the four
// luma values (a blend of the channels followed by one luma is other integers).  3: the blend per channel, written to
// planes R, G, B of frame f (dst frame f holds PLANES planes; a frame of zeros is zero in all of them).  The luma is at
// most 255 * 65536 + 32768 < 2^24; the sums stay those of the grey form.
template <bool TABLE, int PLANES = 0>
__global__ __launch_bounds__(256) void ingest_u8_kernel(const uint8_t* __restrict__ src, int64_t frame_stride, int sh,
                                                        int sw, int64_t pitch, const int64_t* __restrict__ table,
                                                        int dh, int dw, int rows, int strips, int mode,
                                                        float* __restrict__ dst, int fmt) {
  constexpr int NP = PLANES == 3 ? 3 : 1;
  __shared__ float lut[256];
  __shared__ int xofs[INGEST_MAX_DW];
  __shared__ uint32_t xw[INGEST_MAX_DW];
  __shared__ int yofs[INGEST_MAX_ROWS];
  __shared__ uint32_t yw[INGEST_MAX_ROWS];
  const int tid = threadIdx.x;
  const int f = blockIdx.x / strips;
  const int y0 = (blockIdx.x - f * strips) * rows;
  const int nr = min(rows, dh - y0);
  float* out = dst + ((int64_t)f * NP * dh + y0) * dw;
  if constexpr (TABLE) {
    const int64_t* e = table + 4 * (int64_t)f;
    src = reinterpret_cast<const uint8_t*>(e[0]);
    sh = (int)e[1];
    sw = (int)e[2];
    pitch = e[3];
    if (src == nullptr) {
#pragma unroll
      for (int c = 0; c < NP; ++c)
        for (int i = tid; i < nr * dw; i += 256) out[(int64_t)c * dh * dw + i] = 0.f;
      return;
    }
  } else {
    src += (int64_t)f * frame_stride;
  }
  lut[tid] = ingest_pixel((uint32_t)tid, mode);
  for (int d = tid; d < dw; d += 256) resize_tap(d, sw, dw, xofs[d], xw[d]);
  if (tid < nr) resize_tap(y0 + tid, sh, dh, yofs[tid], yw[tid]);
  __syncthreads();
  const int gpr = (dw + 3) >> 2;
  for (int it = tid; it < nr * gpr; it += 256) {
    const int r = it / gpr, x4 = (it - r * gpr) * 4;
    const int sy = yofs[r], ya = (int)(yw[r] & 0xffffu), yb = (int)(yw[r] >> 16);
    const uint8_t* s0 = src + (int64_t)sy * pitch;
    const uint8_t* s1 = src + (int64_t)min(sy + 1, sh - 1) * pitch;
    f32x4 o[NP];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = min(x4 + e, dw - 1);  // (a group past the row's end repeats its last pixel and stores none of it)
      const int sx = xofs[x], xa = (int)(xw[x] & 0xffffu), xb = (int)(xw[x] >> 16);
      if constexpr (PLANES == 0) {
        const int h0 = sx + 1 < sw ? s0[sx] * xa + s0[sx + 1] * xb : s0[sx] * INGEST_ONE;
        const int h1 = sx + 1 < sw ? s1[sx] * xa + s1[sx + 1] * xb : s1[sx] * INGEST_ONE;
        const int v = (ya * h0 + yb * h1 + (1 << 21)) >> 22;
        o[0][e] = lut[min(255, max(0, v))];
      } else {
        // the right-hand tap of the last column is the column itself (always in bounds) and its weight unused
        const bool two = sx + 1 < sw;
        const int step = ingest_step(fmt), ka = sx * step, kb = (two ? sx + 1 : sx) * step;
        const int cofs[3] = {ingest_r(fmt), 1, ingest_b(fmt)};
        int t[4][3];  // taps (row 0 left, row 0 right, row 1 left, row 1 right) x (R, G, B)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          t[0][c] = s0[ka + cofs[c]];
          t[1][c] = s0[kb + cofs[c]];
          t[2][c] = s1[ka + cofs[c]];
          t[3][c] = s1[kb + cofs[c]];
        }
        if constexpr (PLANES == 1) {
          int l[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) l[q] = luma_u8(t[q][0], t[q][1], t[q][2]);
          const int h0 = two ? l[0] * xa + l[1] * xb : l[0] * INGEST_ONE;
          const int h1 = two ? l[2] * xa + l[3] * xb : l[2] * INGEST_ONE;
          const int v = (ya * h0 + yb * h1 + (1 << 21)) >> 22;
          o[0][e] = lut[min(255, max(0, v))];
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int h0 = two ? t[0][c] * xa + t[1][c] * xb : t[0][c] * INGEST_ONE;
            const int h1 = two ? t[2][c] * xa + t[3][c] * xb : t[2][c] * INGEST_ONE;
            const int v = (ya * h0 + yb * h1 + (1 << 21)) >> 22;
            o[c][e] = lut[min(255, max(0, v))];
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < NP; ++c) {
      float* p = out + ((int64_t)c * dh + r) * dw + x4;
      if (x4 + 4 <= dw && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        *reinterpret_cast<f32x4*>(p) = o[c];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (x4 + e < dw) p[e] = o[c][e];
      }
    }
  }
}

// what both entry points ask of the output and the mode; returns the rows per block through `rows`
static int ingest_check_output(const char* fn, int64_t nf, int dh, int dw, int mode, const float* dst, int& rows) {
  const std::string name(fn);
  VAD_CHECK(dst != nullptr, name + ": null dst");
  VAD_CHECK(nf >= 1, name + ": nf must be >= 1");
  VAD_CHECK(dh >= 1 && dw >= 1, name + ": dh and dw must be >= 1");
  VAD_CHECK(dw <= INGEST_MAX_DW, name + ": dw must be at most " + std::to_string(INGEST_MAX_DW) +
                                     " (the columns of the kernel's LDS table)");
  VAD_CHECK(mode >= 0 && mode <= 2, name + ": mode 0 (Normalize 0.5/0.5), 1 (u8/255) or 2 (u8/255 clamped to "
                                               "0.001..0.999)");
  VAD_CHECK((reinterpret_cast<uintptr_t>(dst) & 15) == 0, name + ": dst must be 16-byte aligned");
  VAD_CHECK(nf <= ((1ll << 31) - 1) / ((int64_t)dh * dw * 4), name + ": dst (nf * dh * dw * 4 bytes) is 2 GB or more");
  rows = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(INGEST_MAX_ROWS, dh), INGEST_ITEMS / cdiv(dw, 4)));
  return 0;
}

// one source frame; `who` names it in the error text ("" for the uniform entry, "entry 3 " for a table row)
// (step: bytes per pixel, 1 for grey)
static int ingest_check_source(const char* fn, const std::string& who, int64_t sh, int64_t sw, int64_t pitch,
                               int step = 1) {
  const std::string name = std::string(fn) + ": " + who;
  VAD_CHECK(sh >= 1 && sw >= 1, name + "sh and sw must be >= 1 (got sh = " + std::to_string(sh) + ", sw = " +
                                    std::to_string(sw) + ")");
  if (step == 1) {
    VAD_CHECK(pitch >= sw, name + "pitch " + std::to_string(pitch) + " is less than sw = " + std::to_string(sw));
  } else {
    VAD_CHECK(sw < (1ll << 31) && pitch >= step * sw,
              name + "pitch " + std::to_string(pitch) + " is less than " + std::to_string(step) + " * sw = " +
                  std::to_string(step * sw) + " (sw = " + std::to_string(sw) + ")");
  }
  VAD_CHECK(sh < (1ll << 31) && pitch < (1ll << 31) && sh * pitch < (1ll << 31),
            name + "the frame (sh * pitch bytes) is 2 GB or more");
  return 0;
}

// what the colour entry points ask beyond the grey ones: the format, the planes and the larger output
static int ingest_check_color(const char* fn, int64_t nf, int fmt, int planes, int dh, int dw) {
  const std::string name(fn);
  VAD_CHECK(fmt >= 0 && fmt <= 3, name + ": fmt 0 (rgb), 1 (bgr), 2 (rgbx) or 3 (bgrx), got " + std::to_string(fmt));
  VAD_CHECK(planes == 1 || planes == 3, name + ": planes 1 (grey) or 3 (planar RGB), got " + std::to_string(planes));
  VAD_CHECK(nf <= ((1ll << 31) - 1) / ((int64_t)planes * dh * dw * 4),
            name + ": dst (nf * planes * dh * dw * 4 bytes) is 2 GB or more");
  return 0;
}

// The body of the four ingest entry points.  table: the nf rows (address, sh, sw, pitch) of host_table are validated
// and copied to dev_table; otherwise the uniform form, nf frames of sh x sw at src, frame_stride bytes apart.  color:
// packed colour pixels of fmt into `planes` planes; otherwise grey source bytes (fmt and planes are not read).
static int ingest_launch(const char* fn, bool table, const int64_t* host_table, void* dev_table, const uint8_t* src,
                         int sh, int sw, int64_t pitch, int64_t frame_stride, int64_t nf, bool color, int fmt,
                         int planes, int dh, int dw, int mode, float* dst, hipStream_t stream) {
  const std::string name(fn);
  VAD_CHECK(table || src != nullptr, name + ": null src");
  VAD_CHECK(!table || (host_table && dev_table), name + ": null table (host_table or dev_table)");
  VAD_CHECK((reinterpret_cast<uintptr_t>(dev_table) & 15) == 0, name + ": dev_table must be 16-B aligned");
  int rows = 0;
  VAD_TRY(ingest_check_output(fn, nf, dh, dw, mode, dst, rows));
  if (color) VAD_TRY(ingest_check_color(fn, nf, fmt, planes, dh, dw));
  const int step = color ? ingest_step(fmt) : 1;
  if (table) {
    for (int64_t f = 0; f < nf; ++f) {
      const int64_t* e = host_table + 4 * f;
      if (e[0] == 0) continue;  // a frame of zeros: its sizes are not read
      VAD_TRY(ingest_check_source(fn, "entry " + std::to_string(f) + ": ", e[1], e[2], e[3], step));
    }
    VAD_HIP(hipMemcpyAsync(dev_table, host_table, (size_t)nf * 32, hipMemcpyHostToDevice, stream));
  } else {
    VAD_TRY(ingest_check_source(fn, "", sh, sw, pitch, step));
    VAD_CHECK(frame_stride >= 0, name + ": frame_stride must be >= 0");
  }
  // [uniform, table form][grey, colour to 1 plane, colour to 3 planes]
  static constexpr decltype(&ingest_u8_kernel<false, 0>) kernels[2][3] = {
      {ingest_u8_kernel<false, 0>, ingest_u8_kernel<false, 1>, ingest_u8_kernel<false, 3>},
      {ingest_u8_kernel<true, 0>, ingest_u8_kernel<true, 1>, ingest_u8_kernel<true, 3>}};
  const auto kernel = kernels[table][!color ? 0 : planes == 1 ? 1 : 2];
  const int strips = (int)cdiv(dh, rows);
  hipLaunchKernelGGL(kernel, dim3((unsigned)(nf * strips)), dim3(256), 0, stream, src, frame_stride, sh, sw, pitch,
                     static_cast<const int64_t*>(dev_table), dh, dw, rows, strips, mode, dst, color ? fmt : 0);
  VAD_LAUNCH_CHECK();
  return 0;
}

}  // namespace vad

using namespace vad;

extern "C" {

int vad_u8_to_clip(const uint8_t* src, int64_t n, int mode, float* dst, void* stream) {
  VAD_CHECK(mode == 0 || mode == 1, "vad_u8_to_clip: mode 0 (Normalize 0.5/0.5) or 1 (u8/255)");
  VAD_CHECK((reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0,
            "vad_u8_to_clip: src and dst must be 16-byte aligned");
  if (n <= 0) return 0;
  // (1024 blocks keep ~4 MB of 16-B requests in flight: enough for HBM, and for PCIe when src is mapped host memory)
  hipLaunchKernelGGL(u8_to_clip_kernel, dim3((unsigned)std::min<int64_t>(cdiv(n / 16 + 1, 256), 1024)), dim3(256), 0,
                     (hipStream_t)stream, src, n, mode, dst);
  VAD_LAUNCH_CHECK();
  return 0;
}

int vad_ingest_u8(const uint8_t* src, int64_t nf, int sh, int sw, int64_t pitch, int64_t frame_stride, int dh, int dw,
                  int mode, float* dst, void* stream) {
  return ingest_launch("vad_ingest_u8", false, nullptr, nullptr, src, sh, sw, pitch, frame_stride, nf, false, 0, 0, dh,
                       dw, mode, dst, (hipStream_t)stream);
}

int vad_ingest_u8_color(const uint8_t* src, int64_t nf, int sh, int sw, int64_t pitch, int64_t frame_stride, int fmt,
                        int planes, int dh, int dw, int mode, float* dst, void* stream) {
  return ingest_launch("vad_ingest_u8_color", false, nullptr, nullptr, src, sh, sw, pitch, frame_stride, nf, true, fmt,
                       planes, dh, dw, mode, dst, (hipStream_t)stream);
}

int64_t vad_ingest_table_bytes(int64_t nf) {
  if (nf < 1 || nf > (1ll << 31)) {
    vad::set_error("vad_ingest_table_bytes: nf must be >= 1");
    return -1;
  }
  return nf * 32;
}

int vad_ingest_u8_table(const int64_t* host_table, int64_t nf, int dh, int dw, int mode, float* dst, void* dev_table,
                        void* stream) {
  return ingest_launch("vad_ingest_u8_table", true, host_table, dev_table, nullptr, 0, 0, 0, 0, nf, false, 0, 0, dh, dw,
                       mode, dst, (hipStream_t)stream);
}

int vad_ingest_u8_color_table(const int64_t* host_table, int64_t nf, int fmt, int planes, int dh, int dw, int mode,
                              float* dst, void* dev_table, void* stream) {
  return ingest_launch("vad_ingest_u8_color_table", true, host_table, dev_table, nullptr, 0, 0, 0, 0, nf, true, fmt,
                       planes, dh, dw, mode, dst, (hipStream_t)stream);
}

int vad_luma_u8(const uint8_t* src, int sh, int sw, int64_t pitch, int fmt, uint8_t* dst) {
  VAD_CHECK(src && dst && sh > 0 && sw > 0, "vad_luma_u8: bad arguments");
  VAD_CHECK(fmt >= 0 && fmt <= 3, "vad_luma_u8: fmt 0 (rgb), 1 (bgr), 2 (rgbx) or 3 (bgrx), got " + std::to_string(fmt));
  const int step = ingest_step(fmt), ro = ingest_r(fmt), bo = ingest_b(fmt);
  VAD_CHECK(pitch >= (int64_t)step * sw, "vad_luma_u8: pitch " + std::to_string(pitch) + " is less than " +
                                             std::to_string(step) + " * sw = " + std::to_string((int64_t)step * sw));
  for (int y = 0; y < sh; ++y) {
    const uint8_t* s = src + (int64_t)y * pitch;
    uint8_t* d = dst + (int64_t)y * sw;
    for (int x = 0; x < sw; ++x, s += step) d[x] = (uint8_t)luma_u8(s[ro], s[1], s[bo]);
  }
  return 0;
}

int vad_host_device_ptr(const void* host, void** dev) {
  VAD_CHECK(host != nullptr && dev != nullptr, "vad_host_device_ptr: null argument");
  VAD_HIP(hipHostGetDevicePointer(dev, const_cast<void*>(host), 0));
  return 0;
}

int vad_resize_u8(const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw) {
  VAD_CHECK(src && dst && sh > 0 && sw > 0 && dh > 0 && dw > 0, "vad_resize_u8: bad arguments");
  constexpr int ONE = 2048;  // INTER_RESIZE_COEF_SCALE
  // per destination column / row: source index and the two 11-bit weights (rounded like saturate_cast<short>)
  auto table = [&](int dn, int sn, std::vector<int>& ofs, std::vector<int>& c0, std::vector<int>& c1) {
    ofs.resize(dn);
    c0.resize(dn);
    c1.resize(dn);
    const double scale = (double)sn / dn;
    for (int d = 0; d < dn; ++d) {
      float f = (float)((d + 0.5) * scale - 0.5);
      int s = (int)floorf(f);
      f -= (float)s;
      if (s < 0) {
        f = 0.f;
        s = 0;
      }
      if (s >= sn - 1) {
        f = 0.f;
        s = sn - 1;
      }
      ofs[d] = s;
      c0[d] = (int)lrintf((1.f - f) * ONE);
      c1[d] = (int)lrintf(f * ONE);
    }
  };
  std::vector<int> xo, xa, xb, yo, ya, yb;
  table(dw, sw, xo, xa, xb);
  table(dh, sh, yo, ya, yb);
  std::vector<int> r0(dw), r1(dw);
  auto hrow = [&](int sy, std::vector<int>& r) {
    const uint8_t* s = src + (int64_t)sy * sw;
    for (int x = 0; x < dw; ++x) {
      const int sx = xo[x];
      r[x] = sx + 1 < sw ? s[sx] * xa[x] + s[sx + 1] * xb[x] : s[sx] * ONE;
    }
  };
  for (int y = 0; y < dh; ++y) {
    const int sy = yo[y];
    hrow(sy, r0);
    hrow(std::min(sy + 1, sh - 1), r1);
    uint8_t* d = dst + (int64_t)y * dw;
    for (int x = 0; x < dw; ++x) {
      const int64_t v = ((int64_t)ya[y] * r0[x] + (int64_t)yb[y] * r1[x] + (1 << 21)) >> 22;
      d[x] = (uint8_t)std::min<int64_t>(255, std::max<int64_t>(0, v));
    }
  }
  return 0;
}

}  // extern "C"
