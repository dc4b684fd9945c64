// Where "frame t of window b" lives, for every scorer that reads cached per-frame rows.  Three forms:
//   Linear  a video's frame cache: row first + b * stride + t.
//   Ring    one live stream's ring of cap slots, frame g in slot g mod cap: slot (first + b * stride + t) mod cap.
//   Group   many rings of cap slots in one allocation: row b of a device table of int64 words (base, s0[, key]) names
//           the ring's first slot and the window's first slot within it; frame t is slot base + (s0 + t, wrapped once
//           at cap).  The host validated the rows (group_table.h); nothing here checks them.
// In the ring forms T <= cap and s0 < cap, so s0 + t < 2 cap and the modulo is wrap_once: an add, a compare and a
// select on block-uniform values, no division in a loop.  The store kernels use the destination side, frame_slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace vad {

enum class WinForm { Linear, Ring, Group };

// s in [0, 2 cap) -> s mod cap.  The slot rule of every ring form, here and in WinSrc (common.h).
template <class I>
__host__ __device__ inline I wrap_once(I s, I cap) {
  return s >= cap ? s - cap : s;
}

// The windows of one launch; filled on the host by one of the three makers, passed to the kernel by value.
struct WinRows {
  int64_t first;       // Linear: the first frame of window 0.  Ring: its slot (reduced mod cap by ring()).
  int stride;          // Linear, Ring: frames between the starts of windows b and b + 1
  int cap;             // Ring, Group: slots per ring
  const int64_t* tab;  // Group: the device table, words int64 per window
  int words;           // 2: (base, s0); 3: (base, s0, key)
  static WinRows linear(int64_t first, int stride) { return {first, stride, 0, nullptr, 0}; }
  static WinRows ring(int64_t first, int stride, int64_t cap) { return {first % cap, stride, (int)cap, nullptr, 0}; }
  static WinRows group(const int64_t* tab, int words, int cap) { return {0, 1, cap, tab, words}; }
};

// Window b of the launch, resolved once per block: the rows of its frames are base + row(t), t < T.  b must be
// block-uniform: the Group form's table words are then scalar loads (the table is read through the constant address
// space -- nothing writes it while a kernel reads it) and base, s0 and cap stay in scalar registers.
template <WinForm F>
struct WinCursor {
  int64_t base;  // Linear: the window's first row.  Ring: 0.  Group: the first slot of the window's ring.
  int s0, cap;   // Ring, Group: the slot of the window's first frame within its ring; slots per ring
  const __attribute__((address_space(4))) int64_t* e;  // Group: the window's table row
  __device__ WinCursor(const WinRows& w, int b) : base(0), s0(0), cap(w.cap), e(nullptr) {
    if constexpr (F == WinForm::Linear) {
      base = w.first + (int64_t)b * w.stride;
    } else if constexpr (F == WinForm::Ring) {
      // (first < cap and the launch's span fits the ring, so 32 bits hold the sum)
      s0 = (int)(((unsigned)w.first + (unsigned)b * (unsigned)w.stride) % (unsigned)cap);
    } else {
      e = (const __attribute__((address_space(4))) int64_t*)w.tab + (int64_t)w.words * b;
      base = e[0];
      s0 = (int)e[1];
    }
  }
  __device__ int row(int t) const {
    if constexpr (F == WinForm::Linear) return t;
    else return wrap_once(s0 + t, cap);
  }
  __device__ int64_t key() const { return e[2]; }  // Group with words = 3: the window's RNG clip key
};

// The destination side, for a kernel that stores frame f of a chunk: frame0 + f (Linear), that wrapped once at cap
// (Ring: frame0 < cap reduced on the host, and the chunk holds at most cap frames), or dst[f] (Group: block-uniform f
// makes it one scalar load).  A negative result (Group only: a padding frame) means the frame is stored nowhere.
template <WinForm F>
__device__ inline int frame_slot(int f, int frame0, int cap, const int* __restrict__ dst) {
  if constexpr (F == WinForm::Linear) return frame0 + f;
  else if constexpr (F == WinForm::Ring) return wrap_once(frame0 + f, cap);
  else return dst[f];
}

// f(std::integral_constant<WinForm, form>{}): the form as a compile-time constant, so a launch site is one call --
//   win_dispatch(form, [&](auto F) { VAD_KLAUNCH(kernel<F()>, ...); });
template <class Fn>
inline void win_dispatch(WinForm form, Fn&& f) {
  switch (form) {
    case WinForm::Linear: return f(std::integral_constant<WinForm, WinForm::Linear>{});
    case WinForm::Ring: return f(std::integral_constant<WinForm, WinForm::Ring>{});
    case WinForm::Group: return f(std::integral_constant<WinForm, WinForm::Group>{});
  }
}

}  // namespace vad
