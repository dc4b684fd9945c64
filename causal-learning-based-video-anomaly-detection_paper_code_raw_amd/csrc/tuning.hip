// Definitions of the tuning knobs listed in tuning.h and the lookup behind vad_set_tuning / vad_get_tuning.
#include "tuning.h"

#include <cstring>

#include "common.h"

namespace vad {

#define VAD_KNOB_G(key, var, def, doc) int var = def;
#define VAD_KNOB_T(key, var, def, doc) thread_local int var = def;
VAD_TUNING_KNOBS(VAD_KNOB_G, VAD_KNOB_T)
#undef VAD_KNOB_G
#undef VAD_KNOB_T

namespace {
struct Knob {
  const char* key;
  int* (*var)();  // an accessor, not a data pointer: a thread_local's address is no constant
};
#define VAD_KNOB(key, var, def, doc) {#key, []() -> int* { return &var; }},
const Knob KNOBS[] = {VAD_TUNING_KNOBS(VAD_KNOB, VAD_KNOB)};
#undef VAD_KNOB
constexpr int NKNOBS = sizeof(KNOBS) / sizeof(KNOBS[0]);

int* find(const char* key) {
  for (const Knob& k : KNOBS)
    if (key && !std::strcmp(k.key, key)) return k.var();
  set_error(std::string("unknown tuning key ") + (key ? key : "(null)"));
  return nullptr;
}
}  // namespace

int set_tuning(const char* key, int value) {
  int* v = find(key);
  if (v) *v = value;
  return v ? 0 : 1;
}

int get_tuning(const char* key, int* value) {
  VAD_CHECK(value != nullptr, "get_tuning: null value pointer");
  const int* v = find(key);
  if (v) *value = *v;
  return v ? 0 : 1;
}

const char* tuning_name(int i) { return i >= 0 && i < NKNOBS ? KNOBS[i].key : nullptr; }

}  // namespace vad
