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

}  // namespace vad
