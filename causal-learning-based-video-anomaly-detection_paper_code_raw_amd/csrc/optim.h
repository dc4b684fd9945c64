// The slot-wise Adam step of the minicausal, a2 and cad1-autoencoder plans: clip_grad_norm_ (norm of the per-slot
// norms: each rounded to float, summed in double, as torch), then torch.optim.Adam (coupled L2 decay) or AdamW
// (decoupled) over one flat parameter / grad / moment buffer split into slots (= named_parameters()).  What differs
// between the plans is data (AdamStep), not code.  (cad's optimizer, with slot groups and weight images, is its own:
// cad_plan.hip.)
#pragma once
#include "common.h"
#include "plan_util.h"

namespace vad {

constexpr int ADAM_SQ_CHUNKS = 64;  // blocks per slot of the squared-norm pass (fixed-order partials)
// (AdamSlots, the slot table of a step, comes from the plan's FlatLayout::adam_slots(): plan_util.h)

struct AdamWs {
  double* sq;   // [ADAM_MAX_SLOTS][ADAM_SQ_CHUNKS]
  int* bad;     // [ADAM_MAX_SLOTS][ADAM_SQ_CHUNKS]
  float* ctrl;  // [8], five used
  void carve(Ws& w) {
    sq = w.take<double>(ADAM_MAX_SLOTS * ADAM_SQ_CHUNKS);
    bad = w.take<int>(ADAM_MAX_SLOTS * ADAM_SQ_CHUNKS);
    ctrl = w.take<float>(8);
  }
};

// One step's hyperparameters and the device words it reads and writes.
struct AdamStep {
  float lr, b1, b2, eps, wd;
  bool decoupled;    // AdamW: param *= 1 - lr * wd; otherwise wd * param joins the clipped grad
  float clip_above;  // clip only when the norm exceeds it; < 0: always (plain clip_grad_norm_)
  float max_norm;
  float grad_scale;  // multiplies the grads first (1/world after a data-parallel sum)
  const float* gate;  // < 1 on entry: the step was skipped before backward, nothing happens
  float* norm;        // <- grad norm sqrt(sum_p ||g_p||^2)
  float* norm_host;   // nullable: a second place for the norm (device-visible host memory)
  float* clipped;     // nullable: <- 1 when clipped, else 0
  float* status;      // nullable: non-finite grads skip the step (the reference's skip) and leave 1 here, a step 2;
                      // null: no finiteness gate
};

// steps: int32 per slot (torch's per-param counters)
int adam_clip_step(const AdamSlots& t, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                   int64_t nfloats, int32_t* steps, const AdamWs& w, const AdamStep& a, hipStream_t st);

}  // namespace vad
