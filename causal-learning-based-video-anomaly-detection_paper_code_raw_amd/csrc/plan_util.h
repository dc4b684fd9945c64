// Shared by the plans: the workspace carving (a dry pass sizes the workspace, a bound pass hands out aligned pointers)
// and the flat parameter layout (one table of named slots per model, offsets by one rule, one set of C accessors).
#pragma once
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "common.h"

namespace vad {

struct Ws {
  char* base = nullptr;
  int64_t off = 0;
  bool dry = true;
  template <class T>
  T* take(int64_t n) {
    off = (off + 255) / 256 * 256;
    T* p = dry ? nullptr : reinterpret_cast<T*>(base + off);
    off += n * (int64_t)sizeof(T);
    return p;
  }
};

constexpr int ADAM_MAX_SLOTS = 64;
// the slot table optim.h's Adam step takes: off, numel in floats (more slots than the cap: refused by adam_clip_step)
struct AdamSlots {
  int n;
  int64_t off[ADAM_MAX_SLOTS], numel[ADAM_MAX_SLOTS];
};

struct FlatSlot {
  std::string name;
  int64_t numel, offset;
  int group;  // cad's optimizer groups; 0 elsewhere
};

// Where every parameter (slots: named_parameters() order) and BatchNorm running statistic (bufs) of a model lives in
// its flat fp32 buffers: a running sum, each slot rounded up to 256 floats.
struct FlatLayout {
  std::vector<FlatSlot> slots, bufs;
  std::vector<int64_t> offsets;  // slots[i].offset, contiguous (a2 copies it to the device)
  int64_t param_floats = 0, buf_floats = 0;

  FlatLayout() = default;
  FlatLayout(std::initializer_list<std::pair<const char*, int64_t>> table) {
    for (const auto& s : table) add(s.first, s.second);
    finish();
  }
  int add(const std::string& name, int64_t numel, int group = 0) {
    slots.push_back({name, numel, 0, group});
    return (int)slots.size() - 1;
  }
  int add_buf(const std::string& name, int64_t numel) {
    bufs.push_back({name, numel, 0, 0});
    return (int)bufs.size() - 1;
  }
  void finish() {
    for (auto& s : slots) {
      s.offset = param_floats;
      offsets.push_back(s.offset);
      param_floats += (s.numel + 255) / 256 * 256;
    }
    for (auto& b : bufs) {
      b.offset = buf_floats;
      buf_floats += (b.numel + 255) / 256 * 256;
    }
  }
  AdamSlots adam_slots() const {
    AdamSlots t{};
    t.n = (int)slots.size();
    for (int i = 0; i < t.n && i < ADAM_MAX_SLOTS; ++i) {
      t.off[i] = slots[i].offset;
      t.numel[i] = slots[i].numel;
    }
    return t;
  }
};

// the one bounds-checked lookup behind the vad_*_slot_* / vad_*_buf_* accessors (null layout or index out of range:
// nullptr)
inline const FlatSlot* flat_at(const FlatLayout* l, std::vector<FlatSlot> FlatLayout::*table, int i) {
  return (l && i >= 0 && i < (int)(l->*table).size()) ? &(l->*table)[i] : nullptr;
}

}  // namespace vad

// The five table accessors of include/vad.h for one model prefix and one table (slot, slots, param_floats) or
// (buf, bufs, buf_floats).  P0 / P1: the parameter lists without / with the index i; LY: a const FlatLayout* (null:
// every accessor answers -1 / nullptr, as an index out of range does).
#define VAD_FLAT_ABI(pfx, kind, table, total, P0, P1, LY)                             \
  int vad_##pfx##_num_##kind##s P0 {                                                  \
    const vad::FlatLayout* l = (LY);                                                  \
    return l ? (int)l->table.size() : -1;                                             \
  }                                                                                   \
  const char* vad_##pfx##_##kind##_name P1 {                                          \
    const vad::FlatSlot* s = vad::flat_at((LY), &vad::FlatLayout::table, i);          \
    return s ? s->name.c_str() : nullptr;                                             \
  }                                                                                   \
  int64_t vad_##pfx##_##kind##_numel P1 {                                             \
    const vad::FlatSlot* s = vad::flat_at((LY), &vad::FlatLayout::table, i);          \
    return s ? s->numel : -1;                                                         \
  }                                                                                   \
  int64_t vad_##pfx##_##kind##_offset P1 {                                            \
    const vad::FlatSlot* s = vad::flat_at((LY), &vad::FlatLayout::table, i);          \
    return s ? s->offset : -1;                                                        \
  }                                                                                   \
  int64_t vad_##pfx##_##total P0 {                                                    \
    const vad::FlatLayout* l = (LY);                                                  \
    return l ? l->total : -1;                                                         \
  }
#define VAD_FLAT_SLOT_ABI(pfx, P0, P1, LY) VAD_FLAT_ABI(pfx, slot, slots, param_floats, P0, P1, LY)
#define VAD_FLAT_BUF_ABI(pfx, P0, P1, LY) VAD_FLAT_ABI(pfx, buf, bufs, buf_floats, P0, P1, LY)
