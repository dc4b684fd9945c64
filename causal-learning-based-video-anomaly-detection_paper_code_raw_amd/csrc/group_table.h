// The device table of one stream-group push, shared by cad_plan.hip and ae_plan.hip (host code only): the plan's nf
// destination slots (int32) from byte 0, the window rows (row_words int64 each: base, first and for cad a key) from the
// next multiple of 16 bytes.  The kernels trust what they read, so both walks validate the host table entry by entry
// before anything is queued; fn, the calling entry point, prefixes every error text.
#pragma once
#include <algorithm>
#include <vector>

#include "common.h"

namespace vad {

static inline int64_t group_window_table_offset(int64_t nf) { return (nf * 4 + 15) & ~15ll; }
static inline int64_t* group_window_rows(void* dev_table, int64_t nf) {
  return reinterpret_cast<int64_t*>(static_cast<char*>(dev_table) + group_window_table_offset(nf));
}

static inline int64_t group_table_bytes(const char* fn, int64_t nf, int64_t nw, int row_bytes) {
  if (nf < 1 || nw < 0 || nf > (1ll << 31) || nw > (1ll << 31)) {
    set_error(std::string(fn) + ": nf must be >= 1 and nw >= 0");
    return -1;
  }
  return group_window_table_offset(nf) + nw * row_bytes;
}

// host_dst[0 .. nf): -1 (a padding frame, stored nowhere) or a slot in 0 .. total_slots - 1 that no other entry names
static inline int check_and_copy_dst_table(const char* fn, const int32_t* host_dst, int nf, int64_t total_slots,
                                           void* dev_table, hipStream_t stream) {
  const std::string name(fn);
  std::vector<int32_t> seen;
  for (int f = 0; f < nf; ++f) {
    const int32_t d = host_dst[f];
    VAD_CHECK(d >= -1 && d < total_slots, name + ": dst[" + std::to_string(f) + "] = " + std::to_string(d) +
                                              " is outside -1 .. total_slots - 1 = " + std::to_string(total_slots - 1));
    if (d >= 0) seen.push_back(d);
  }
  std::sort(seen.begin(), seen.end());
  for (size_t i = 1; i < seen.size(); ++i)
    VAD_CHECK(seen[i] != seen[i - 1], name + ": two entries of dst name slot " + std::to_string(seen[i]));
  VAD_HIP(hipMemcpyAsync(dev_table, host_dst, (size_t)nf * 4, hipMemcpyHostToDevice, stream));
  return 0;
}

// host_windows[0 .. nw) rows of row_words int64: base (the ring's first slot, a multiple of cap) and first (the slot of
// the window's first frame within the ring); further words are not read here.  Copies the rows to group_window_rows.
static inline int check_and_copy_window_rows(const char* fn, const int64_t* host_windows, int row_words, int nw, int cap,
                                             int64_t total_slots, void* dev_table, int nf, hipStream_t stream) {
  for (int i = 0; i < nw; ++i) {
    const int64_t base = host_windows[row_words * i], s0 = host_windows[row_words * i + 1];
    const char* what = nullptr;
    if (base < 0 || base % cap != 0) what = "base must be a non-negative multiple of cap";
    else if (base + cap > total_slots) what = "base + cap exceeds total_slots";
    else if (s0 < 0 || s0 >= cap) what = "first must be in 0..cap - 1";
    VAD_CHECK(!what, std::string(fn) + ": window " + std::to_string(i) + " (base " + std::to_string(base) + ", first " +
                         std::to_string(s0) + "): " + what);
  }
  VAD_HIP(hipMemcpyAsync(group_window_rows(dev_table, nf), host_windows, (size_t)nw * row_words * 8,
                         hipMemcpyHostToDevice, stream));
  return 0;
}

// The clip models' group windows calls (vad_a2 / vad_mc / vad_bbox _windows_forward_group): their device
// table has no destination part -- nw rows of (base, first) from byte 0.  win_group_check: the argument checks the
// three share, apart from the rows; the entry point then makes its plan's own checks and calls win_group_src, which
// validates the rows, queues their one copy and gives the window source the first conv reads (common.h WinSrc, group
// form).  frames holds total_slots frames of frame_floats floats: total_slots / cap rings of cap slots; nw windows of
// T frames on a plan of B clips.
static inline int win_group_check(const char* fn, const float* frames, int64_t total_slots, int cap,
                                  const int64_t* host_windows, int nw, void* dev_table, int64_t B, int64_t T) {
  const std::string name(fn);
  VAD_CHECK(frames != nullptr, name + ": null ring");
  VAD_CHECK(host_windows && dev_table, name + ": null table (host_windows or dev_table)");
  VAD_CHECK((reinterpret_cast<uintptr_t>(dev_table) & 15) == 0, name + ": dev_table must be 16-B aligned");
  VAD_CHECK(cap >= 1 && total_slots >= cap && total_slots % cap == 0,
            name + ": cap must be in 1..total_slots and divide it, got cap " + std::to_string(cap) + ", total_slots " +
                std::to_string(total_slots));
  VAD_CHECK(cap >= T, name + ": a ring of cap = " + std::to_string(cap) + " slots holds no window of " +
                          std::to_string(T) + " frames");
  VAD_CHECK(nw >= 1 && nw <= B, name + ": between 1 and the plan's " + std::to_string(B) + " windows per call, got " +
                                    std::to_string(nw));
  return 0;
}

static inline int win_group_src(const char* fn, const float* frames, int64_t frame_floats, int64_t total_slots, int cap,
                                const int64_t* host_windows, int nw, void* dev_table, hipStream_t stream, WinSrc& ws) {
  VAD_TRY(check_and_copy_window_rows(fn, host_windows, 2, nw, cap, total_slots, dev_table, 0, stream));
  ws = WinSrc{frames, frame_floats, 0, 0, 0, static_cast<const int64_t*>(dev_table), cap};
  return 0;
}

}  // namespace vad
