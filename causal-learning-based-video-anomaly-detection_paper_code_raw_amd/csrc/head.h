// Fused per-clip causal head of CausalAnomalyDetector (causal_anomaly_detection.py:160-502) and the step tail
// (softmax of the direct classifier, score blend cad:573-576, losses cad:673-686).
#pragma once
#include "common.h"

namespace vad {

constexpr int NMAX = 5;      // detections per frame (cad:178)
constexpr int NF_ = 6;       // num_factors
constexpr int GH = 64;       // GRU hidden
constexpr int GIN = 68;      // 4 + reid_dim

// head parameter tensors, in state_dict order
enum HeadSlot {
  H_REID0_W, H_REID0_B, H_REID2_W, H_REID2_B, H_REID4_W, H_REID4_B,
  H_GRU_WIH, H_GRU_WHH, H_GRU_BIH, H_GRU_BHH, H_ENC_W, H_ENC_B,
  H_CE0_W, H_CE0_B, H_CE2_W, H_CE2_B, H_MU_W, H_MU_B, H_LV_W, H_LV_B,
  H_SP, H_NODE_W, H_NODE_B, H_EDGE0_W, H_EDGE0_B, H_EDGE2_W, H_EDGE2_B,
  H_DYN0_W, H_DYN0_B, H_DYN2_W, H_DYN2_B, H_DYN4_W, H_DYN4_B,
  H_CS0_W, H_CS0_B, H_CS3_W, H_CS3_B, H_CS5_W, H_CS5_B,
  H_MS0_W, H_MS0_B, H_MS2_W, H_MS2_B, H_MS4_W, H_MS4_B,
  H_TS0_W, H_TS0_B, H_TS2_W, H_TS2_B, H_TS4_W, H_TS4_B,
  H_NUM
};

struct HeadArgs {
  int B, T;
  int64_t clip0;          // global index of clip 0 (RNG keying under data parallelism)
  int training;
  uint64_t h1_eps, h1_drop;
  uint32_t thr_drop;      // scorer dropout p = 0.2
  const float* pbase;     // flat parameter buffer
  int64_t off[H_NUM];     // slot offsets into pbase / grad slabs (relative to head_begin for slabs)
  int64_t head_begin;
  int lw_len;             // floats of the parameter range [off[H_ENC_W], end of the last slot) staged in LDS
  float* ws;              // per-clip workspace (small per-clip tensors)
  int64_t ws_stride;
  int* iws;               // per-clip int workspace
  int64_t iws_stride;
  float* rows;            // per-trajectory-row arrays, R = B*T*NMAX rows (see RowLayout in head.hip)
  float* grad;            // flat grad buffer (GRU / ReID weight grads are written here directly)
};

constexpr int HW_LDS = 20480;  // capacity (floats) of the sequence kernels' LDS weight image
// sets lw_len from a.off and the last slot's size; nonzero if the image does not fit or a slot is not 16-B aligned
int head_pack_weights(HeadArgs& a, const int64_t* numel);

// HeadArgs of one head call on the cad parameter layout (cad_plan.hip): RNG keys of (seed, step), slot offsets and the
// LDS image length from the layout, the caller's parameter / gradient buffers and workspaces.  The plan and the
// stand-alone entry points (ops_api.hip) both fill their arguments here.
HeadArgs cad_head_args(int B, int T, int64_t clip0, int training, uint64_t seed, uint64_t step, const float* params,
                       float* grads, float* ws, int* iws, float* rows);
int64_t cad_head_grad_begin();  // offset of the first head slot in the flat parameter / gradient buffers
int64_t cad_head_slab_len();    // floats from there to the first slot after the head: one per-clip gradient slab

int64_t head_ws_floats(int T);
int64_t head_iws_ints(int T);
int64_t head_rows_floats(int B, int T);
int64_t head_rows_gi_offset(int B, int T);  // of the GRU input projections [B*T*5][192] in the row arrays

// forward: det logits [B*T][20] -> per-clip outputs
struct HeadOut {
  float* causal;   // [B]
  float* kl;       // [B]
  float* z;        // [B][5][6]
  float* adj;      // [B][6][6]
  float* boxes;    // [B][T][5][4]  valid boxes compacted per frame (fallback box when none)
  int* counts;     // [B][T]        boxes per frame (>=1)
  int* nmax;       // [B]
  int* clip_flags; // [B][2]       (any valid detection, nmax>=2)
};
int head_fwd(const HeadArgs& a, const float* det_logits, const HeadOut& o, hipStream_t st);
// the two launches of head_fwd (row-parallel part, then the per-clip sequence part)
int head_rows_fwd(const HeadArgs& a, const float* det_logits, const HeadOut& o, hipStream_t st);
int head_seq_fwd(const HeadArgs& a, const HeadOut& o, hipStream_t st);

// ------------------------------------------------------------------ sliding-window scoring (video.hip)
// Frame cache of a video of N frames: what the per-frame stage of the eval forward leaves for the windowed stage.
// Five arrays over the video's frames (float offsets, each 64-float aligned): feats [N][6144], gi [N][5][192] (the
// GRU input projections of the frame's five trajectory rows), boxes [N][5][4], counts [N] (int), slot [N][5] (int).
struct FrameCache {
  int64_t N, feats, gi, boxes, counts, slot, total;
  __host__ __device__ explicit FrameCache(int64_t N_) : N(N_) {
    int64_t o = 0;
    auto take = [&](int64_t w) { int64_t r_ = o; o += (N * w + 63) & ~63ll; return r_; };
    feats = take(6144); gi = take(NMAX * 3 * GH); boxes = take(NMAX * 4); counts = take(1); slot = take(NMAX);
    total = o;
  }
};
// The same layout serves a live stream as a ring of N slots, and a group of streams as total_slots = (number of
// rings) * cap slots, ring s in slots s * cap .. (s + 1) * cap - 1.  The three functions below take the form as a
// WinForm; how each form finds frame t of window b, and where it stores frame f of a chunk, is win_rows.h.  The group
// form's device tables were validated by the caller on the host (vad_cad_*_group in cad_plan.hip); nothing here looks
// at a table's contents.  Which frames are resident is the caller's bookkeeping.
// copies the B*T frames head_rows_fwd just processed (a.rows / a.iws, o.boxes / o.counts) and their pooled features to
// the cache: frame f to slot frame_slot(f) of its nframes slots (Linear, Ring: from frame0, and a ring's chunk may
// straddle the wrap; Group: to dst[f], a device table, or nowhere where dst[f] < 0)
int frame_cache_store(const HeadArgs& a, const HeadOut& o, const float* feats, float* cache, int64_t nframes,
                      WinForm form, int64_t frame0, const int* dst, hipStream_t st);
// pooled[i][k] = (sum_{t < T} feats[frame t of window i of win][k]) / T for i < nw, summed in ascending t from 0 as
// avgpool_fwd forms a clip's mean, in every form
int window_mean(const float* cache, int64_t nframes, int T, WinForm form, const WinRows& win, int nw, float* pooled,
                hipStream_t st);
// head_seq_fwd on windows of the cache, forward only: block i runs window i of win.rows with the RNG key of clip
// a.clip0 + i (Group: the key of its table row, three words per row; a.clip0 is not read) and writes row i of
// o.causal / kl / z / adj / nmax / clip_flags; a.T is the window length; a.rows / a.ws / a.iws are not used (no
// backward state is kept).
struct SeqWindows {
  const float* gi;    // FrameCache::gi
  const int* counts;  // FrameCache::counts
  const int* slot;    // FrameCache::slot
  WinRows rows;
};
int head_seq_windows_fwd(const HeadArgs& a, WinForm form, const SeqWindows& win, int nw, const HeadOut& o,
                         hipStream_t st);

// backward: upstream grads -> grad slabs [B][slab] and d(det logits) [B*T][20]
struct HeadUp {
  const float* d_causal;  // [B]
  const float* d_kl;      // [B]
  const float* d_z;       // [B][5][6] or null
  const float* d_adj;     // [B][6][6] or null
  const float* d_boxes;   // [B][T][5][4] or null: grads of the compacted per-frame detections (HeadOut::boxes)
};
int head_bwd(const HeadArgs& a, const float* det_logits, const HeadOut& o, const HeadUp& up, float* slabs,
             int64_t slab_len, float* d_det_logits, hipStream_t st);
int head_slab_reduce(const float* slabs, int B, int64_t slab_len, float* grad_head, hipStream_t st);
// GRU / ReID weight grads over all trajectory rows, written to a.grad (run after head_slab_reduce)
int head_rows_wgrad(const HeadArgs& a, hipStream_t st);

// tail: softmax(direct logits), final score, optional loss + upstream grads, flag OR-reduce
struct TailArgs {
  int B;
  const float* direct_logits;   // [B][2]
  const float* causal;          // [B]
  const float* kl;              // [B]
  const int* clip_flags;        // [B][2]
  float* probs;                 // [B][2]
  float* final_scores;          // [B]
  int* flags;                   // [2] (det_in_graph, struct_in_graph) -> also mirrored as floats
  float* flags_f;               // [2] or null
  uint64_t* det_gate;           // forward: 1 when no box is in range (no detector gradient), else 0; or null
  // loss mode
  const int64_t* labels;        // [B] or null
  float* losses;                // [5]: classification, anomaly, causal, kl, total
  // upstream grads (written when labels != null or ext grads given)
  const float* ext_d_final;     // [B]   (module API) or null
  const float* ext_d_probs;     // [B][2]
  const float* ext_d_causal;    // [B]
  const float* ext_d_kl;        // [B]
  float* d_causal;              // [B]
  float* d_kl;                  // [B]
  float* d_direct_logits;       // [B][2]
  int64_t* nbt;                 // forward: BN num_batches_tracked counters bumped (train mode) or null
  int nbt_n;
  int fwd_bwd;                  // forward with labels: also write the loss-mode upstream grads (the backward then
                                // skips its tail launch)
};
int cad_tail_fwd(const TailArgs& t, hipStream_t st);
int cad_tail_bwd(const TailArgs& t, hipStream_t st);

}  // namespace vad
