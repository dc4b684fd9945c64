/*
 * libvadhip — C ABI of the MI355X (gfx950) hot path of
 * pvvkishore/Causal-Learning-Based-Video-Anomaly-Detection_Paper_Code_Raw.
 *
 * The reference exposes no FFI: its boundary is the Python nn.Module surface
 * (SURVEY.md §8b).  Every entry point below replaces one piece of that surface;
 * the Python package binds them with ctypes.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless stated; fp32 unless stated;
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work;
 *   - return 0 on success, non-zero on error; vad_last_error() has the text
 *     (the Python layer raises RuntimeError, mirroring cad:702-709);
 *   - the caller (PyTorch) owns every buffer, including the workspace.
 */
#ifndef VAD_H_
#define VAD_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAD_ABI_VERSION 1

int vad_abi_version(void);
const char* vad_last_error(void);

/* ------------------------------------------------------------------------------------------
 * RNG (bit-exact twin of oracle/rng.py).  Replaces the torch CPU generator draws of
 * nn.Dropout and torch.randn_like in the reference (cad:170,173,330,438,528,531).
 * ------------------------------------------------------------------------------------------ */
/* uint32 u24 draws for rows row0.. and cols 0..ncols-1 (testing the contract) */
int vad_rng_u24(uint64_t seed, uint32_t stream_id, uint64_t step, int64_t row0, int64_t nrows, int64_t ncols,
                uint32_t* out, void* stream);
/* synthetic clips: x = (u8 - 0.5) / 0.5, u8 = hash >> 56 (UCSDped2Dataset + Normalize(0.5,0.5), cad:92-96) */
int vad_synth_frames(uint64_t seed, uint64_t step, int64_t frame0, int64_t nframes, int64_t npix, int mode,
                     float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * causal_anomaly_detection.py — CausalAnomalyDetector (cad:508-586) + train_model step (cad:609-690)
 * ------------------------------------------------------------------------------------------ */
typedef struct vad_cad_plan vad_cad_plan;

/* flat parameter layout: slot i = i-th entry of model.named_parameters() (state_dict order) */
int vad_cad_num_slots(void);
const char* vad_cad_slot_name(int i);
int64_t vad_cad_slot_numel(int i);
int64_t vad_cad_slot_offset(int i);
/* 0 frozen (cad:596-598), 1 always has grad, 2 detector (grad iff any in-range box), 3 structure learner
 * (grad iff some clip has >=2 trajectories), 4 never has grad (structure_params) */
int vad_cad_slot_group(int i);
int64_t vad_cad_param_floats(void);   /* flat params size; the grad buffer has 256 extra floats (flags) */
int vad_cad_num_bufs(void);           /* BatchNorm running_mean / running_var tensors, state_dict order */
const char* vad_cad_buf_name(int i);
int64_t vad_cad_buf_numel(int i);
int64_t vad_cad_buf_offset(int i);
int64_t vad_cad_buf_floats(void);
int vad_cad_num_bn(void);             /* num_batches_tracked counters (int64 array) */

int vad_cad_create(int B, int T, int H, int W, vad_cad_plan** out);
void vad_cad_destroy(vad_cad_plan* plan);
int64_t vad_cad_workspace_bytes(const vad_cad_plan* plan);
/* bind caller-owned buffers. exp_avg/exp_avg_sq/steps may be NULL when no optimizer step is used. */
int vad_cad_bind(vad_cad_plan* plan, void* workspace, float* params, float* grads, float* bufs, int64_t* nbt,
                 float* exp_avg, float* exp_avg_sq, int32_t* steps);

/* CausalAnomalyDetector.forward.  training=1: batch-stat BN + running-stat update + dropout.
 * labels (int64 [B], may be NULL) additionally computes the train_model loss terms.
 * outputs: final [B], probs [B,2], causal [B], kl [B], z [B,5,6], adj [B,6,6], nmax int32 [B],
 *          boxes [B,T,5,4], counts int32 [B,T], losses [5] (cls, anomaly, causal, kl, total), flags int32 [2] */
int vad_cad_forward(vad_cad_plan* plan, const float* x, int training, uint64_t seed, uint64_t step, int64_t clip0,
                    const int64_t* labels, float* final_scores, float* probs, float* causal, float* kl, float* z,
                    float* adj, int32_t* nmax, float* boxes, int32_t* counts, float* losses, int32_t* flags,
                    void* stream);
/* backward of the last forward.  use_loss=1: upstream grads of the train_model loss (needs labels in forward);
 * otherwise the given upstream grads (any may be NULL = zero).  Writes the flat grad buffer (all slots). */
int vad_cad_backward(vad_cad_plan* plan, int use_loss, const float* d_final, const float* d_probs,
                     const float* d_causal, const float* d_kl, const float* d_z, const float* d_adj, void* stream);
/* vad_cad_backward in two calls (same arguments; stage 0 then stage 1, both on the same stream): stage 0 runs the
 * loss tail, the causal head, the direct classifier and the detector and zeroes the grad buffer first, so every
 * grad outside the backbone slots is final when it returns; stage 1 runs the backbone (cad:141-158).  Replaces
 * the single `total_loss.backward()` (cad:688) when a data-parallel caller overlaps the head-grad all-reduce with
 * the backbone backward (DDP's bucketed reduce during backward). */
int vad_cad_backward_stage(vad_cad_plan* plan, int stage, int use_loss, const float* d_final, const float* d_probs,
                           const float* d_causal, const float* d_kl, const float* d_z, const float* d_adj,
                           void* stream);
/* stage 2 of vad_cad_backward_stage is stage 0 for a caller that orders its own consumer of the non-backbone grads
 * itself: it returns as soon as the caller's stream has its part queued, the causal head / detector backward keeps
 * running on the plan's side stream, and stage 1 (the backbone) then waits only for the detector's input gradient;
 * vad_cad_wait_side(plan, s) makes stream s wait for everything queued so far on that side stream (a data-parallel
 * caller's all-reduce stream, before it sums those grads).  Stage 1 after stage 2 re-joins the side stream. */
int vad_cad_wait_side(vad_cad_plan* plan, void* stream);
/* vad_cad_wait_layer_grads(plan, l, s): stream s waits until every grad of backbone layer l (0..7: the conv weight and
 * bias and the BatchNorm gamma / beta of causal_anomaly_detection.py:128-139's l-th conv; layer 0 also the stem's) of
 * the backbone backward queued last is final -- the per-layer buckets of a data-parallel gradient all-reduce, issued
 * while the layers below are still in their backward (DDP's reduce-during-backward, cad:688-690). */
int vad_cad_wait_layer_grads(vad_cad_plan* plan, int layer, void* stream);
/* vad_cad_input_ready(plan, s) arms the NEXT vad_cad_forward of this plan (one-shot): its input clips are complete
 * once the work queued on stream s at this call is.  With the frozen fused stem (and per-rank BatchNorm statistics)
 * that forward then runs conv1 + bn1 + the max pool on a plan stream ordered after that point only -- not after
 * what the caller's stream still has queued, e.g. the previous step's last weight gradient and optimizer step --
 * and layer1.0 waits for it.  Without the call a forward orders its stem after the caller's stream, as before.
 * (No reference counterpart: the reference's forward is synchronous, cad:669-690.) */
int vad_cad_input_ready(vad_cad_plan* plan, void* stream);
/* vad_cad_backward_stage with one more upstream grad: d_boxes [B,T,5,4] (may be NULL), the grad of a loss on the
 * forward's compacted per-frame detections (boxes output of vad_cad_forward; the reference's detections are slices
 * of the rescaled detector output and carry autograd, cad:201-222).  The constant fallback box takes no grad. */
int vad_cad_backward_ext(vad_cad_plan* plan, int stage, int use_loss, const float* d_final, const float* d_probs,
                         const float* d_causal, const float* d_kl, const float* d_z, const float* d_adj,
                         const float* d_boxes, void* stream);
/* clip_grad_norm_(max_norm) + AdamW over the flat buffers (torch.optim.AdamW semantics, per-slot steps,
 * slots without a grad this step are skipped).  grad_scale multiplies grads first (1/world for DP).
 * total_norm (device float [1], may be NULL) receives the pre-clip norm. */
int vad_cad_optimizer_step(vad_cad_plan* plan, float lr, float beta1, float beta2, float eps, float weight_decay,
                           float max_norm, float grad_scale, float* total_norm, void* stream);
/* SyncBatchNorm mode (BASELINE config 3 parity with the reference's single-process global batch: its BatchNorm2d
 * layers normalise over all B*T frames, cad:116,131,136).  In training mode each of the nine BN layers folds its
 * partial sums into a per-plan double buffer `sums` ([2*C]: forward sum(x) | sum(x^2); backward sum(dZ) |
 * sum(dZ*xhat)) and calls fn(user, bn_layer 0..8, phase 0 fwd / 1 bwd, n_doubles, stream); fn must replace the
 * buffer by its sum over the process group (an all-reduce ordered on `stream`) and return 0.  Statistics then use
 * world * local count.  The buffer's address: vad_cad_debug_buffer(plan, "bn_sync").  fn NULL = per-rank BN
 * (DDP default). */
typedef int (*vad_bn_sync_fn)(void* user, int bn_layer, int phase, int64_t n, void* stream);
int vad_cad_set_bn_sync(vad_cad_plan* plan, vad_bn_sync_fn fn, void* user, int world);

/* Sliding-window scoring of a video (eval mode, forward only).  Replaces test_model's loop over clips
 * (cad:1210-1232) on the clips UCSDped2Dataset enumerates at stride T/2 (cad:57), which runs every frame's backbone
 * once per clip that holds it: with running BatchNorm statistics everything up to the GRU input projection depends on
 * the frame alone, so it runs once per frame into a caller-owned frame cache, and windows then read frames
 * start + t of the cache.
 * The cache of a video of nframes frames holds five fields, each [nframes][...] and 64-float aligned:
 * 0 feats [6144] (cad:560-566), 1 gi [5][192] (W_ih x + b_ih of the frame's zero-padded trajectory rows, cad:248-274,
 * 298), 2 boxes [5][4] (compacted in-range boxes or the fallback box, cad:198-228), 3 counts (int32), 4 slot [5]
 * (int32: the detector output a compacted box came from, -1 fallback, -2 padding).
 * vad_cad_frame_cache_floats: its size in floats; vad_cad_frame_cache_offset: a field's offset in floats (both -1 on
 * a bad argument). */
int64_t vad_cad_frame_cache_floats(int64_t nframes);
int64_t vad_cad_frame_cache_offset(int64_t nframes, int field);
/* The per-frame stage of CausalAnomalyDetector.forward in eval mode (cad:548-566 backbone + pooled features,
 * cad:167-179 detector_net, cad:198-228 box decode, cad:248-274 ReID + trajectory rows, and the GRU's input
 * projection of cad:298) on the plan's B*T frames x [B*T,1,H,W], written to frames frame0 .. frame0 + B*T - 1 of
 * the cache.  It stops before the recurrence.  No parameter, BatchNorm buffer or counter changes; the plan's
 * activations of an earlier forward do. */
int vad_cad_frames_forward(vad_cad_plan* plan, const float* x, int64_t nframes, float* cache, int64_t frame0,
                           void* stream);
/* The per-window stage for windows w0 .. w0 + nw - 1 (window w = frames w*stride .. w*stride + T - 1 of the cache; nw
 * at most the plan's B): the mean over the window's features and the direct classifier on it (cad:568-570), the GRU
 * recurrence, VAE, structure learner, dynamics and scorers per window (cad:287-502; Nmax = the largest box count
 * among the window's own frames, cad:262-271) and the blend (cad:573-576).  Row i of every output is window w0 + i,
 * which equals vad_cad_forward(training = 0) on that clip at clip index clip0 + w0 + i -- the key of its VAE noise
 * (cad:328-331 draws it in eval mode too).  outputs: final [nw], probs [nw,2], causal [nw], kl [nw], z [nw,5,6],
 * adj [nw,6,6], nmax int32 [nw]; none may be NULL.  T > nframes, stride < 1 or a window range outside the video is an
 * error and launches nothing. */
int vad_cad_windows_forward(vad_cad_plan* plan, const float* cache, int64_t nframes, int T, int stride, int64_t w0,
                            int nw, uint64_t seed, uint64_t step, int64_t clip0, float* final_scores, float* probs,
                            float* causal, float* kl, float* z, float* adj, int32_t* nmax, void* stream);
/* The same two stages on a live stream of frames, with the cache used as a ring: a cache of cap slots (the layout
 * vad_cad_frame_cache_floats(cap) / vad_cad_frame_cache_offset(cap, field) describe) in which frame g, counted from
 * the start of the stream, lives in slot g mod cap.  The library keeps no record of which frames a ring holds: that
 * is the caller's bookkeeping -- a frame is resident from its vad_cad_frames_forward_ring until a later one stores
 * frame g + cap over it, and a window must be scored while all its frames are.
 * vad_cad_frames_forward_ring: vad_cad_frames_forward on the plan's B*T frames, stored as frames frame0 .. frame0 +
 * B*T - 1 of the ring (the chunk may straddle the wrap).  B*T > cap or frame0 < 0 is an error and launches nothing. */
int vad_cad_frames_forward_ring(vad_cad_plan* plan, const float* x, int64_t cap, float* cache, int64_t frame0,
                                void* stream);
/* vad_cad_windows_forward for nw windows of the ring: window i < nw covers frames first_frame + i*stride + t, t < T,
 * and row i of every output equals vad_cad_forward(training = 0) on that clip at clip index clip0 + widx0 + i (widx0:
 * the index of the batch's first window since the start of the stream).  The batch must fit the ring: T outside
 * 1..cap, stride < 1, nw outside 1..the plan's B, or a span (nw - 1)*stride + T > cap is an error, names the argument
 * in vad_last_error and launches nothing. */
int vad_cad_windows_forward_ring(vad_cad_plan* plan, const float* cache, int64_t cap, int T, int stride,
                                 int64_t first_frame, int64_t widx0, int nw, uint64_t seed, uint64_t step,
                                 int64_t clip0, float* final_scores, float* probs, float* causal, float* kl, float* z,
                                 float* adj, int32_t* nmax, void* stream);
/* The same two stages for a group of streams that share launches: one cache of total_slots slots (the layout of
 * vad_cad_frame_cache_floats(total_slots)) holding total_slots / cap rings of cap slots, ring s in slots s*cap ..
 * (s+1)*cap - 1.  Which slot a frame goes to and which slots a window reads come from tables the caller passes as
 * HOST pointers.  Each call validates its table entry by entry on the host -- a violation returns non-zero, names the
 * entry in vad_last_error and launches nothing, so a bad table cannot cause a store or a load outside the cache --
 * and then copies it with one hipMemcpyAsync on `stream` into dev_table, which the kernels read.  dev_table is
 * caller-owned device memory, 16-byte aligned, of at least vad_cad_group_table_bytes(B*T of the frames plan, nw)
 * bytes (the destinations from byte 0, the window rows after them; -1 on a bad argument); the library still owns no
 * device memory.  The caller must not reuse dev_table -- for another call or anything else -- while an earlier call
 * on ANOTHER stream may still read it; calls on one stream are ordered by the stream.  A pageable host table may be
 * changed as soon as the call returns; a pinned one only once `stream` has passed the copy. */
int64_t vad_cad_group_table_bytes(int64_t nf, int64_t nw);
/* vad_cad_frames_forward on the plan's B*T frames, frame f stored to slot host_dst[f] of the cache, or nowhere where
 * host_dst[f] is -1 (a padding frame: its per-frame stage runs, nothing of it is kept).  Every host_dst[f] must lie
 * in -1 .. total_slots - 1 and no two entries >= 0 may be equal. */
int vad_cad_frames_forward_group(vad_cad_plan* plan, const float* x, int64_t total_slots, float* cache,
                                 const int32_t* host_dst, void* dev_table, void* stream);
/* vad_cad_windows_forward_ring for nw windows that may lie in different rings: host_windows holds three int64 per
 * window, (base, first, key) -- the window's frame t is slot base + ((first + t) wrapped once at cap), and row i of
 * every output equals vad_cad_forward(training = 0) on that clip at clip index key (the key of its VAE noise).
 * base must be a multiple of cap with base + cap <= total_slots, 0 <= first < cap, 1 <= T <= cap, T <= 4096 and
 * 1 <= nw <= the plan's B.  dev_table is the one of the frames call on the same plan (the window rows lie after that
 * plan's B*T destinations).  Outputs as vad_cad_windows_forward_ring. */
int vad_cad_windows_forward_group(vad_cad_plan* plan, const float* cache, int64_t total_slots, int cap, int T,
                                  const int64_t* host_windows, int nw, void* dev_table, uint64_t seed, uint64_t step,
                                  float* final_scores, float* probs, float* causal, float* kl, float* z, float* adj,
                                  int32_t* nmax, void* stream);

/* ------------------------------------------------------------------------------------------
 * Single building blocks (kernel unit tests; same kernels as the fused step)
 * ------------------------------------------------------------------------------------------ */
/* Y[M,N] = act(X[M,K] W[N,K]^T + b)  (nn.Linear + optional ReLU) */
int vad_dense_forward(const float* X, int M, int K, const float* W, const float* b, int N, float* Y, int relu,
                      float* scratch, int64_t scratch_floats, void* stream);
/* nn.Conv2d(Ci, Co, 3, stride, padding=1) on NHWC activations; W in torch layout [Co][Ci][3][3].
 * scratch: wf/wd 9*Ci*Co floats each, partials >= ceil(M/64)*2*Co floats (M = NF*OH*OW). */
int vad_conv3x3_forward(const float* x_nhwc, int NF, int Ci, int IH, int IW, const float* w, const float* bias,
                        int Co, int stride, float* y_nhwc, float* wf_scratch, float* wd_scratch, float* partials,
                        void* stream);
/* input gradient of the same conv (transposed conv; stride-2 split into four parity classes) */
int vad_conv3x3_dgrad(const float* dy_nhwc, int NF, int Ci, int IH, int IW, const float* w, int Co, int stride,
                      float* dx_nhwc, float* wf_scratch, float* wd_scratch, void* stream);
/* vad_conv3x3_forward with the fused-step extras: src_stats (nullable) = the BatchNorm state of the layer that made x,
 * [mean | invstd | scale | shift] (4 Ci floats): the conv reads relu(scale x + shift), zero-padded; *nparts = rows of
 * BN partial sums written to partials ([nparts][2 Co], or [2 Co][nparts] when *parts_cm comes back 1) */
int vad_conv3x3_forward_bn(const float* x_nhwc, const float* src_stats, int NF, int Ci, int IH, int IW, const float* w,
                           const float* bias, int Co, int stride, float* y_nhwc, float* wf_scratch, float* wd_scratch,
                           float* partials, int* nparts, int* parts_cm, void* stream);
/* vad_conv3x3_dgrad with the BN-backward reduce of the layer that made the conv's input fused into its epilogue:
 * y = that layer's raw output (dx's dims), stats = its BN state (4 Ci floats); the per-block sums of dZ and dZ xhat land
 * column-major [2 Ci][*nparts] in parts (parts_floats floats); *nparts = 0 when the dispatched kernel does not fuse */
int vad_conv3x3_dgrad_bnfuse(const float* dy_nhwc, int NF, int Ci, int IH, int IW, const float* w, int Co, int stride,
                             float* dx_nhwc, float* wf_scratch, float* wd_scratch, const float* y_nhwc,
                             const float* stats, float* parts, int64_t parts_floats, int* nparts, void* stream);
/* kernel tuning knobs (sweeps, A/B of kernel variants): the keys, their defaults and meanings are the list in
 * csrc/tuning.h.  Process-global, except "conv_bf16" and "act_bf16" (the calling thread's).  An unknown key fails with
 * the error "unknown tuning key <key>". */
int vad_set_tuning(const char* key, int value);
int vad_get_tuning(const char* key, int* value);
/* the i-th key of the list, or null past its end */
const char* vad_tuning_name(int i);
/* weight gradient of the same conv: dW[Co][Ci][3][3] = sum over pixels dY x patches(x); split-K slabs in partial */
int vad_conv3x3_wgrad(const float* x_nhwc, const float* dy_nhwc, int NF, int Ci, int IH, int IW, int Co, int stride,
                      float* dW, float* partial, int64_t partial_floats, void* stream);
/* the backbone's BatchNorm backward apply pass (cad:116,131,136 -- the per-element half of BatchNorm2d + ReLU
 * backward): dY = k (dZ - mean dZ - xhat mean(dZ xhat)), dZ = dA [s y + t > 0]; rows M = NF*H*W, channels C;
 * stats = the layer's [7 C] state [mean | invstd | scale | shift | k | mean dZ | mean dZ xhat]; bf16 != 0: dA, y, dY
 * are bf16 (config 4), else fp32 */
int vad_bn_bwd_apply(const void* dA, const void* y, const float* stats, int M, int C, void* dY, int bf16,
                     void* stream);
/* nn.Conv3d(Ci, Co, 3, stride (sd, sh, sw), padding=1) of the clip-level 3-D CNNs (mc:25-102, a2:27-35, bbox:58-65) on
 * one named kernel family; w in torch layout [Co][Ci][3][3][3]; outputs, dy and dx are NDHWC.  path:
 *   0  im2col3d + dense_fwd / dense_dgrad + col2im3d / dense_wgrad (any stride, any channel counts);
 *   1  conv3d_direct_*: stride 1, Ci <= 16, Co in {8, 16, 32}; its input gradient (the forward over dy with the
 *      flipped weights) additionally needs Ci in {8, 16};
 *   2  conv3s2_*: stride 2 on all three axes, Ci % 4 == 0, Co % 4 == 0;
 *   3  conv3d_prep_w3 + conv3d_x3_fwd: forward only, stride 1, Ci % 16 == 0, Co % 32 == 0.
 * A combination the path does not support is an error (no fall-back to another path).  layout: 0 = x is NCDHW (torch),
 * 1 = NDHWC; paths 2 and 3 read NDHWC only.  scratch (caller-owned) holds the path's weight images / columns and, in
 * what is left, its split-K slabs: vad_conv3d_scratch_floats(kind 0 forward / 1 input gradient / 2 weight gradient)
 * is the least it needs (< 0: unsupported combination); more lets the GEMMs split K as they do inside the plans. */
int64_t vad_conv3d_scratch_floats(int kind, int path, int N, int Ci, int D, int H, int W, int Co, int sd, int sh,
                                  int sw);
int vad_conv3d_forward(const float* x, int layout, int N, int Ci, int D, int H, int W, const float* w,
                       const float* bias, int Co, int sd, int sh, int sw, int path, float* y, float* scratch,
                       int64_t scratch_floats, void* stream);
/* gate (nullable, path 2 only, dx's layout): dx = 0 where !(gate > 0), the fused backward of the ReLU that made gate */
int vad_conv3d_dgrad(const float* dy, int N, int Ci, int D, int H, int W, const float* w, int Co, int sd, int sh,
                     int sw, int path, const float* gate, float* dx, float* scratch, int64_t scratch_floats,
                     void* stream);
/* dW [Co][Ci][27] and db [Co] (nullable on paths 1 and 2), written, not accumulated */
int vad_conv3d_wgrad(const float* x, int layout, const float* dy, int N, int Ci, int D, int H, int W, int Co, int sd,
                     int sh, int sw, int path, float* dW, float* db, float* scratch, int64_t scratch_floats,
                     void* stream);
/* nn.MaxPool3d((kd, kh, kw)) (stride = kernel, floor mode) of act(y), y NDHWC (N, D, H, W, C) -> out NDHWC;
 * act = relu(stats[2C + c] * y + stats[3C + c]) when stats != NULL (a BatchNorm state [mean | invstd | scale | shift],
 * 4 C floats), else relu(y) when relu, else y.  The backward writes dA (y's dims): dout at the first maximum of each
 * window in torch's scan order, zero elsewhere; it obeys the "maxpool3d_bwd_win" knob. */
int vad_maxpool3d_forward(const float* y, const float* stats, int relu, int N, int C, int D, int H, int W, int kd,
                          int kh, int kw, float* out, void* stream);
int vad_maxpool3d_backward(const float* y, const float* stats, int relu, int N, int C, int D, int H, int W, int kd,
                           int kh, int kw, const float* dout, float* dA, void* stream);
/* nn.AdaptiveAvgPool3d((OD, OH, OW)) of act(x) (act as above), x NDHWC -> out [N][C][OD][OH][OW] (torch's flatten
 * order); the backward writes dx (NDHWC) from dout in that order, zero where !(gate > 0) when gate (nullable, dx's
 * layout) is given */
int vad_adaptive_avgpool3d_forward(const float* x, const float* stats, int relu, int N, int C, int D, int H, int W,
                                   int OD, int OH, int OW, float* out, void* stream);
int vad_adaptive_avgpool3d_backward(const float* dout, int N, int C, int D, int H, int W, int OD, int OH, int OW,
                                    const float* gate, float* dx, void* stream);
/* The dense-layer launchers and the fused MLP chain alone, with every argument the plans give them (kernel unit
 * tests).  Arrays named "host" are host arrays (of device pointers where they hold pointers); `skip` is a nullable
 * DEVICE flag: 0 -> every kernel of the call returns without writing.
 * vad_dense_forward with dropout after the activation when drop_p > 0: keep iff u24(seed, stream_id, step, row0 + row,
 * col) >= floor(drop_p 2^24), kept values times 1 / (1 - drop_p) (oracle/rng.py dropout_keep / dropout_scale);
 * max_splits > 0 caps the split-K count, scratch_floats bounds it (0: no split) */
int vad_dense_forward_ex(const float* X, int M, int K, const float* W, const float* b, int N, float* Y, int relu,
                         double drop_p, uint64_t seed, uint32_t stream_id, uint64_t step, int64_t row0, int max_splits,
                         float* scratch, int64_t scratch_floats, void* stream);
/* dX[M,K] = (dY[M,N] W[N,K]) * (gate > 0 ? gscale : 0) (gate nullable, dX's layout; gate_rows > 0: row m is gated by
 * gate row m % gate_rows); scratch (nullable): split-K slabs */
int vad_dense_dgrad(const float* dY, int M, int N, const float* W, int K, float* dX, const float* gate, float gscale,
                    int gate_rows, const int* skip, float* scratch, int64_t scratch_floats, void* stream);
/* dW[N,K] = dY[M,N]^T X[M,K], db[N] (nullable) = colsum(dY); written, not accumulated.  scratch >= N (K + 1) floats
 * unless M <= 16 and K % 4 == 0; target_blocks: split-K blocks to aim for (the plans give 256 or 1024) */
int vad_dense_wgrad(const float* dY, int M, int N, const float* X, int K, float* dW, float* db, const int* skip,
                    float* scratch, int64_t scratch_floats, int target_blocks, void* stream);
/* A 5-layer chain out[i] = drop_i(act_i(out[i-1] W[i]^T + b[i])), out[-1] = X[M,K0]; host N[5], W[5], b[5], relu[5],
 * drop_p[5] (0: none), stream_id[5], out[5]; layers 1-4 need N[i] % 4 == 0, N[i-1] % 8 == 0 and widths <= 512.
 * mode 0: layer 0 by the dense forward, layers 1-4 by the fused tail; mode 1: layer 0 as split-K partial sums that the
 * tail finishes.  scratch: the four transposed weights (256-byte aligned each), then the split-K slabs
 * (mode 1: at least M N[0] floats) */
int vad_mlp_tail_forward(const float* X, int M, int K0, const int* N, const float* const* W, const float* const* b,
                         const int* relu, const double* drop_p, const uint32_t* stream_id, uint64_t seed,
                         uint64_t step, int64_t row0, int mode, float* const* out, float* scratch,
                         int64_t scratch_floats, void* stream);
/* the chain's input gradients d[i-1] = (d[i] W[i]) * (h[i-1] > 0 ? gscale[i-1] : 0), i = 4..1, d[4] = dout[M,N[4]];
 * host W[5], K[5], N[5] (W[i] is [N[i]][K[i]], K[i] = N[i-1]; entry 0 is not read), h[4], gscale[4], d[4] */
int vad_mlp_tail_backward(int M, const float* dout, const float* const* W, const int* K, const int* N,
                          const float* const* h, const float* gscale, float* const* d, const int* skip, void* stream);
/* dW[s][O,I] = A[s][R,O]^T X[s][R,I], db[s][O] (nullable) = colsum(A[s]) for nseg <= 6 layers in one launch, written;
 * host dW, db, A, X, O, I [nseg] */
int vad_rows_wgrad(int R, int nseg, float* const* dW, float* const* db, const float* const* A, const float* const* X,
                   const int* O, const int* I, const int* skip, void* stream);
/* The causal head alone (cad:194-502: box decode and compaction, ReID, GRU, VAE + KL, structure learner, dynamics,
 * scorers) on detector logits [B*T][20] the caller chose, with the arguments the cad plan gives it (kernel unit tests).
 * params / grads: flat buffers in the cad slot layout (vad_cad_slot_offset; only the head's slots are read / written;
 * grads has vad_cad_param_floats() floats).  The VAE noise and the scorer dropout are those of vad_cad_forward at
 * (seed, step, clip0); training = 0: no scorer dropout.  Outputs: causal [B], kl [B], z [B][5][6] (rows >= nmax zero),
 * adj [B][6][6], boxes [B][T][5][4] (in-range boxes compacted per frame, the fallback box when none), counts [B][T],
 * nmax [B], clip_flags [B][2] (a detection in range, nmax >= 2).  scratch (16-byte aligned, at least
 * vad_head_scratch_floats(B, T) floats) carries the forward's state to the backward: same buffer, untouched between.
 * vad_head_backward: upstream gradients d_causal [B], d_kl [B] and the nullable d_z, d_adj, d_boxes (the outputs'
 * shapes) -> every head slot of grads (written, not accumulated; the rest of grads is left alone) and
 * d_det_logits [B*T][20] (zero at every slot that is out of range or in a fallback frame); the forward's outputs are
 * passed again.  A refused call returns non-zero before anything is queued. */
int64_t vad_head_scratch_floats(int B, int T);
int vad_head_forward(const float* det_logits, int B, int T, const float* params, int training, uint64_t seed,
                     uint64_t step, int64_t clip0, float* causal, float* kl, float* z, float* adj, float* boxes,
                     int* counts, int* nmax, int* clip_flags, float* scratch, int64_t scratch_floats, void* stream);
int vad_head_backward(const float* det_logits, int B, int T, const float* params, int training, uint64_t seed,
                      uint64_t step, int64_t clip0, float* causal, float* kl, float* z, float* adj, float* boxes,
                      int* counts, int* nmax, int* clip_flags, const float* d_causal, const float* d_kl,
                      const float* d_z, const float* d_adj, const float* d_boxes, float* grads, float* d_det_logits,
                      float* scratch, int64_t scratch_floats, void* stream);

/* ------------------------------------------------------------------------------------------
 * minicausal_vad_complete3.py — SimpleVideoAnomalyDetector (mc:25-102) + StableTrainer step (mc:249-330)
 * replaces: model(data) (mc:272), criterion(outputs, targets) (mc:284), loss.backward() (mc:292), the grad
 * NaN check / norm / conditional clip (mc:294-306) and optimizer.step() (mc:308, Adam lr 1e-3 wd 1e-5, mc:229-234)
 * ------------------------------------------------------------------------------------------ */
typedef struct vad_mc_plan vad_mc_plan;

/* x: (B, C, T, H, W) fp32 NCDHW (torch layout) */
int vad_mc_create(int B, int C, int T, int H, int W, vad_mc_plan** out);
void vad_mc_destroy(vad_mc_plan* plan);
/* slot i = i-th entry of model.named_parameters(); buffers = BatchNorm3d running stats (state_dict order) */
int vad_mc_num_slots(const vad_mc_plan* plan);
const char* vad_mc_slot_name(const vad_mc_plan* plan, int i);
int64_t vad_mc_slot_numel(const vad_mc_plan* plan, int i);
int64_t vad_mc_slot_offset(const vad_mc_plan* plan, int i);
int64_t vad_mc_param_floats(const vad_mc_plan* plan);
int vad_mc_num_bufs(const vad_mc_plan* plan);
const char* vad_mc_buf_name(const vad_mc_plan* plan, int i);
int64_t vad_mc_buf_numel(const vad_mc_plan* plan, int i);
int64_t vad_mc_buf_offset(const vad_mc_plan* plan, int i);
int64_t vad_mc_buf_floats(const vad_mc_plan* plan);
int64_t vad_mc_workspace_bytes(const vad_mc_plan* plan);
/* nbt: int64[3] num_batches_tracked; steps: int32[num_slots] Adam step counters */
int vad_mc_bind(vad_mc_plan* plan, void* workspace, float* params, float* grads, float* bufs, int64_t* nbt,
                float* exp_avg, float* exp_avg_sq, int32_t* steps);
/* scores: (B,) sigmoid outputs.  labels (B,) fp32 nullable -> BCE.  losses (nullable, float[4]): bce, grad norm,
 * clipped (0/1), status (0 skipped: non-finite outputs/loss; 1 counted, no step: non-finite grads; 2 stepped) —
 * the last three are filled by vad_mc_optimizer_step.  Dropout keys: (seed, step, clip0 + b). */
int vad_mc_forward(vad_mc_plan* plan, const float* x, int training, uint64_t seed, uint64_t step, int64_t clip0,
                   const float* labels, float* scores, float* losses, int32_t* flags, void* stream);
/* The first nw clips of the plan as windows of a video or of a ring of raw frames, eval semantics
 * (training = 0: BatchNorm3d on the running statistics, no dropout): frames (n_frames, C, H, W) fp32 frame-major planar;
 * window b, time t is frame first + b * stride + t, modulo ring when ring > 0 (a ring of ring <= n_frames slots); the
 * first conv reads it in place, its temporal zero padding per window as for a clip.  scores (nw,).  running_mean,
 * running_var, num_batches_tracked, labels, losses and status words are neither read nor written.  The plan's
 * activations are overwritten: vad_mc_backward is refused until the next vad_mc_forward.  Refused before any launch:
 * a null pointer, stride < 1, first < 0, nw outside 1..B, ring < 0; ring = 0: first + (nw - 1) * stride + T > n_frames;
 * ring > 0: ring > n_frames, ring < T, (nw - 1) * stride + T > ring (a window of the call would lap another); an
 * unbound plan; a plan whose convs run on the im2col path (knob conv3d_direct = 0 or C > 16), which has no windows
 * form. */
int vad_mc_windows_forward(vad_mc_plan* plan, const float* frames, int64_t n_frames, int64_t first, int64_t stride,
                           int64_t ring, int nw, float* scores, void* stream);
/* Windows of a group of streams, for the three clip models alike (vad_mc / vad_a2 / vad_bbox
 * _windows_forward_group): ring is one allocation of total_slots frames of C * H * W floats holding total_slots / cap
 * rings of cap slots, ring s in slots s*cap .. (s+1)*cap - 1.  host_windows, a HOST pointer, holds two int64 per
 * window, (base, first): the window's frame t is slot base + (first + t) mod cap, read in place by the first conv, and
 * row i of every output is window i.  The call validates its arguments and the table row by row on the host -- a
 * violation returns non-zero, names the entry point and the numbers in vad_last_error and queues nothing, so a bad
 * table cannot cause a load outside the allocation -- and then copies the rows with one hipMemcpyAsync on `stream`
 * into dev_table, which the first conv reads.  Required: non-null pointers, dev_table 16-byte aligned, cap in
 * 1..total_slots and dividing it, cap >= the plan's T, 1 <= nw <= the plan's B, every base a non-negative multiple of
 * cap with base + cap <= total_slots, 0 <= first < cap; a bound plan and the conv path of the model's windows call.
 * dev_table is caller-owned device memory of at least vad_win_group_table_bytes(nw) bytes (the rows from byte 0, two
 * rows at least; -1 on a bad argument); the caller must not reuse it while an earlier call on ANOTHER stream may still
 * read it.  A pageable host table may be changed as soon as the call returns; a pinned one only once `stream` has
 * passed the copy.  Semantics, outputs and plan state are those of the model's windows call. */
int64_t vad_win_group_table_bytes(int64_t nw);
int vad_mc_windows_forward_group(vad_mc_plan* plan, const float* ring, int64_t total_slots, int cap,
                                 const int64_t* host_windows, int nw, void* dev_table, float* scores, void* stream);
/* d_scores (B,) nullable: NULL = backward of the forward's BCE (requires labels) */
int vad_mc_backward(vad_mc_plan* plan, const float* d_scores, void* stream);
/* grad norm (float64 sum of per-param norm^2); clip_grad_norm_(max_norm) only when norm > clip_above; Adam */
int vad_mc_optimizer_step(vad_mc_plan* plan, float lr, float beta1, float beta2, float eps, float weight_decay,
                          float clip_above, float max_norm, void* stream);
/* The minicausal classifier and its BCE alone (kernel unit tests): the part of vad_mc_forward / vad_mc_backward
 * behind the average pool -- Dropout(.5), Linear(32, 16), ReLU, Dropout(.3), Linear(16, 8), ReLU, Linear(8, 1),
 * sigmoid, the BCE, the status words -- run by the plan's own code on feature rows the caller chose; the convs are
 * never run, so a plan of the smallest clip (T = 4, H = W = 8) serves, and neither the BatchNorm running statistics
 * nor num_batches_tracked are touched.  feats [B][32] is copied into the plan's buffer (NULL: the rows of the plan's
 * last forward stay).  labels, scores, losses, flags as vad_mc_forward's; saved (nullable): host array of 5 nullable
 * device pointers that receive the saved activations fd [B][32], h1 [B][16], h1d [B][16], h2 [B][8] and o [B].
 * vad_mc_head_backward: d_scores as vad_mc_backward's (NULL needs labels in the last head forward) -> the six
 * classifier slots of the bound grads (written; the conv and BatchNorm slots are left alone), dfeat [B][32]
 * (nullable) and dz (nullable): host array of 3 nullable device pointers that receive the pre-activation gradients
 * dz1 [B][16], dz2 [B][8] and dz3 [B].  A refused call returns non-zero before anything is queued. */
int vad_mc_head_forward(vad_mc_plan* plan, const float* feats, int training, uint64_t seed, uint64_t step,
                        int64_t clip0, const float* labels, float* scores, float* losses, int32_t* flags,
                        float* const* saved, void* stream);
int vad_mc_head_backward(vad_mc_plan* plan, const float* d_scores, float* dfeat, float* const* dz, void* stream);

/* ------------------------------------------------------------------------------------------
 * avenue_training_script2.py — a2 CausalAnomalyDetector (a2:15-101), compute_improved_loss (a2:135-205) and the
 * ImprovedMiniCausalVAD step (a2:218-245).  replaces: self.model(videos) (a2:224), compute_improved_loss (a2:227),
 * loss.backward() (a2:235), clip_grad_norm_(0.5) (a2:236), AdamW(lr 5e-4, wd 1e-3).step() (a2:115-119, 238)
 * ------------------------------------------------------------------------------------------ */
typedef struct vad_a2_plan vad_a2_plan;

int vad_a2_num_slots(void);            /* 20 = model.named_parameters() order (188,849 parameters) */
const char* vad_a2_slot_name(int i);
int64_t vad_a2_slot_numel(int i);
int64_t vad_a2_slot_offset(int i);
int64_t vad_a2_param_floats(void);
/* x: (B, 3, T, H, W) fp32 NCDHW, 2 <= B <= 256 */
int vad_a2_create(int B, int T, int H, int W, vad_a2_plan** out);
void vad_a2_destroy(vad_a2_plan* plan);
int64_t vad_a2_workspace_bytes(const vad_a2_plan* plan);
int vad_a2_bind(vad_a2_plan* plan, void* workspace, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                int32_t* steps);
/* outputs (nullable): scores (B,), adj (B,16,16), features (B,16).  with_loss: compute_improved_loss with
 * pseudo-labels keyed (seed, step, clip0 + b); losses float[10]: total, anomaly, acyclicity, sparsity,
 * consistency, structure, edge_count, sparsity_ratio, grad norm (optimizer), status (0 NaN skip, 2 stepped) */
int vad_a2_forward(vad_a2_plan* plan, const float* x, int training, uint64_t seed, uint64_t step, int64_t clip0,
                   int with_loss, float* scores, float* adj, float* features, float* losses, void* stream);
/* "borrow_input" 1: the next forwards read x in place and the backward reads it again (the caller keeps it unchanged
 * until then, as the fused train step does); 0 (default): the forward copies x for conv3d_1's weight gradient */
int vad_a2_set_option(vad_a2_plan* plan, const char* key, int64_t value);
/* The first nw clips of the plan as windows of a video or of a ring of raw frames, forward only, eval
 * semantics (no dropout, no loss, nothing kept for a backward): frames (n_frames, 3, H, W) fp32 frame-major planar RGB;
 * window b, time t is frame first + b * stride + t, modulo ring when ring > 0; conv3d_1 reads it in place (nothing is
 * copied into the plan, borrow_input is ignored).  Outputs (nullable): scores (nw,), adj (nw,16,16), features (nw,16)
 * -- what vad_a2_forward(training = 0) gives for the nw gathered clips; nw = 1 runs as two copies of the window, as a
 * single clip must on the clip path, and returns the first.  The plan's activations are overwritten: vad_a2_backward
 * is refused until the next vad_a2_forward.  Refused before any launch: as vad_mc_windows_forward; a plan created with
 * knob a2_direct = 0. */
int vad_a2_windows_forward(vad_a2_plan* plan, const float* frames, int64_t n_frames, int64_t first, int64_t stride,
                           int64_t ring, int nw, float* scores, float* adj, float* features, void* stream);
/* vad_a2_windows_forward for the windows of a group of streams (vad_mc_windows_forward_group: the arguments, the
 * table and the refusals).  nw = 1 runs row 0 twice and returns the first, as vad_a2_windows_forward. */
int vad_a2_windows_forward_group(vad_a2_plan* plan, const float* ring, int64_t total_slots, int cap,
                                 const int64_t* host_windows, int nw, void* dev_table, float* scores, float* adj,
                                 float* features, void* stream);
/* compute_improved_loss alone, on the last forward's scores / adjacency (pseudo-labels keyed by seed/step/clip0);
 * vad_a2_loss_grads copies d total / d scores (B,) and d total / d adj (B,16,16) of that loss */
int vad_a2_loss(vad_a2_plan* plan, uint64_t seed, uint64_t step, int64_t clip0, float* losses, void* stream);
int vad_a2_loss_grads(vad_a2_plan* plan, float* d_scores, float* d_adj, void* stream);
/* all upstream grads NULL: backward of the forward's loss; else the given (nullable) output grads */
int vad_a2_backward(vad_a2_plan* plan, const float* d_scores, const float* d_adj, const float* d_features,
                    void* stream);
int vad_a2_optimizer_step(vad_a2_plan* plan, float lr, float beta1, float beta2, float eps, float weight_decay,
                          float max_norm, void* stream);
/* The a2 head and compute_improved_loss alone (kernel unit tests): the part of vad_a2_forward / vad_a2_backward behind
 * the average pool -- fc (+ Dropout), causal discovery, graph encoder, predictor, the loss -- run by the plan's own
 * code on pooled rows the caller chose; the convs are never run, so a plan of the smallest clip (T = 1, H = W = 4)
 * serves.  pooled [B][4096] is copied into the plan's buffer (NULL: the rows of the plan's last forward stay).
 * Outputs as vad_a2_forward's; saved (nullable): host array of 8 nullable device pointers that receive the saved
 * activations hc0 [B][32], sig [B][256], g1 [B][128], g1d [B][128], g2 [B][64], cat [B][80], hp0 [B][32] and the
 * pseudo-labels [B] (written with with_loss only).
 * vad_a2_head_backward: upstream gradients as vad_a2_backward's -> the fc and head slots of the bound grads (written;
 * the conv slots are left alone), dpooled [B][4096] (nullable) and dz (nullable): host array of 7 nullable device
 * pointers that receive the pre-activation gradients dz_ap2 [B], dz_ap0 [B][32], dg2 [B][64], dz_ge0 [B][128],
 * dz_cn2 [B][256], dz_cn0 [B][32] and dfeat [B][16] (fc's output gradient).  A refused call returns non-zero before
 * anything is queued. */
int vad_a2_head_forward(vad_a2_plan* plan, const float* pooled, int training, uint64_t seed, uint64_t step,
                        int64_t clip0, int with_loss, float* scores, float* adj, float* features, float* losses,
                        float* const* saved, void* stream);
int vad_a2_head_backward(vad_a2_plan* plan, const float* d_scores, const float* d_adj, const float* d_features,
                         float* dpooled, float* const* dz, void* stream);

/* ------------------------------------------------------------------------------------------
 * avenue_training_script_bbox.py — CausalAnomalyDetector forward (bbox:51-101), eval mode, as run by
 * AnomalyVisualizer.predict_anomaly_for_clip (bbox:339-368).  replaces: self.model(video_tensor) (bbox:357)
 * ------------------------------------------------------------------------------------------ */
typedef struct vad_bbox_plan vad_bbox_plan;

int vad_bbox_num_slots(void);          /* 12 = model.named_parameters() order */
const char* vad_bbox_slot_name(int i);
int64_t vad_bbox_slot_numel(int i);
int64_t vad_bbox_slot_offset(int i);
int64_t vad_bbox_param_floats(void);
/* x: (B, 3, T, H, W) fp32 NCDHW, one clip length per plan (mixed-T batches: one plan per T) */
int vad_bbox_create(int B, int T, int H, int W, vad_bbox_plan** out);
void vad_bbox_destroy(vad_bbox_plan* plan);
int64_t vad_bbox_workspace_bytes(const vad_bbox_plan* plan);
int vad_bbox_bind(vad_bbox_plan* plan, void* workspace, const float* params);
/* scores (B,), adj (B,16,16), features (B,1024, nullable) */
int vad_bbox_forward(vad_bbox_plan* plan, const float* x, float* scores, float* adj, float* features, void* stream);
/* The plan's B clips as windows of a video: frames (n_frames, 3, H, W) fp32 frame-major planar, window b
 * = frames first + b * stride .. + T - 1, read in place by the first layer (its temporal zero padding is per window, as
 * for a clip); the rest of the forward is vad_bbox_forward's.  Refused before any launch: a null pointer, stride < 1,
 * first < 0, first + (B - 1) * stride + T > n_frames, an unbound plan. */
int vad_bbox_windows_forward(vad_bbox_plan* plan, const float* frames, int64_t n_frames, int64_t first, int64_t stride,
                             float* scores, float* adj, float* features, void* stream);
/* vad_bbox_windows_forward on a ring of raw frames: frames holds n_frames >= ring frames, and window b,
 * time t is frame (first + b * stride + t) mod ring.  Refused before any launch: a null pointer, stride < 1, first < 0,
 * ring < T or > n_frames, (B - 1) * stride + T > ring (a window of the call would lap another), an unbound plan, and
 * -- at the launch of the first layer -- knob bbox_im2col = 1, whose strided view cannot express a ring.  ring = 0 is
 * vad_bbox_windows_forward. */
int vad_bbox_ring_forward(vad_bbox_plan* plan, const float* frames, int64_t n_frames, int64_t first, int64_t stride,
                          int64_t ring, float* scores, float* adj, float* features, void* stream);
/* vad_bbox_ring_forward for the windows of a group of streams (vad_mc_windows_forward_group: the arguments, the table
 * and the refusals).  The whole plan runs, so nw must be the plan's B; knob bbox_im2col = 1 is refused as for a ring. */
int vad_bbox_windows_forward_group(vad_bbox_plan* plan, const float* ring, int64_t total_slots, int cap,
                                   const int64_t* host_windows, int nw, void* dev_table, float* scores, float* adj,
                                   float* features, void* stream);
/* Test seams.  vad_bbox_forward is encoder (x -> features) then head (features -> scores, adj);
 * vad_bbox_head_forward runs the head alone -- the causal_net and classifier GEMMs and the sigmoid tail -- on feature
 * rows (B, 1024) the caller chose.  vad_bbox_debug_buffer hands out the workspace arrays of the last forward:
 * "pooled" (B, T/2, H/2, W/2, 32) NDHWC, "y2" (B, T/2, H/2, W/2, 64) NDHWC (conv2 + bias; before the ReLU, which the
 * average pool applies on load -- on the bbox_im2col path the GEMM epilogue has applied it), "hc" (B, 256),
 * "logits" (B, 256), "hcl" (B, 128).  Null arguments, an unbound plan or an unknown name return non-zero before
 * anything is queued. */
int vad_bbox_head_forward(vad_bbox_plan* plan, const float* features, float* scores, float* adj, void* stream);
int vad_bbox_debug_buffer(vad_bbox_plan* plan, const char* name, void** ptr, int64_t* nfloats);

/* ------------------------------------------------------------------------------------------
 * causal_anomaly_detection1.py — memory-bank VideoAutoEncoder (cad1:124-321) and the train_model iteration
 * (cad1:372-431).  replaces: model(videos) (cad1:392), reconstruction_loss (cad1:400), model.update_memory
 * (cad1:407), total_loss.backward() (cad1:411), the NaN-grad check + clip_grad_norm_(0.1) + Adam.step()
 * (cad1:413-425), and the eval forwards of the validation / calculate_anomaly_scores loops (cad1:460, 542-552)
 * ------------------------------------------------------------------------------------------ */
typedef struct vad_ae_plan vad_ae_plan;

int vad_ae_num_slots(void);            /* 38 = model.named_parameters() order */
const char* vad_ae_slot_name(int i);
int64_t vad_ae_slot_numel(int i);
int64_t vad_ae_slot_offset(int i);
int64_t vad_ae_param_floats(void);
int vad_ae_num_bufs(void);             /* 14 BatchNorm running_mean / running_var tensors, state_dict order */
const char* vad_ae_buf_name(int i);
int64_t vad_ae_buf_numel(int i);
int64_t vad_ae_buf_offset(int i);
int64_t vad_ae_buf_floats(void);
/* clips (B, T, 1, 64, 64) fp32 (the encoder's Linear(128*4*4) fixes 64x64 frames), 1 <= B <= 500 */
int vad_ae_create(int B, int T, vad_ae_plan** out);
void vad_ae_destroy(vad_ae_plan* plan);
int64_t vad_ae_workspace_bytes(const vad_ae_plan* plan);
/* nbt: int64[7] num_batches_tracked (encoder.1/4/7/10, decoder.4/7/10); memory: float[500*64] normal_memory;
 * memory_ptr: int64[1]; exp_avg / exp_avg_sq / steps (int32[num_slots]) may be NULL until an optimizer step */
int vad_ae_bind(vad_ae_plan* plan, void* workspace, float* params, float* grads, float* bufs, int64_t* nbt,
                float* memory, int64_t* memory_ptr, float* exp_avg, float* exp_avg_sq, int32_t* steps);
/* stages: 3 = forward() (encode_sequence + decode_sequence + compute_anomaly_score), 1 = encode_sequence only,
 * 2 = decode_sequence of seq_in (B, 64) over T frames.  loss_mode (stages 3): 0 none; 1 the reconstruction MSE
 * against x and per-clip errors (eval loops); 2 the train_model iteration: MSE and its gradient, a non-finite input
 * skips the batch without touching BN running stats / counters / the ring (cad1:385-387), a valid batch's sequence
 * features enter the ring after the scores (cad1:407).  Outputs (nullable): recon (B,T,1,64,64), seq (B,64),
 * frame_feats (B,T,64), scores (B,), recon_err (B,) (loss_mode > 0).  losses float[4]: mse, grad norm, clipped,
 * status (0 skipped, 1 non-finite grads, 2 stepped; the middle two and the final status from the optimizer) */
int vad_ae_forward(vad_ae_plan* plan, const float* x, const float* seq_in, int stages, int training, int loss_mode,
                   float* recon, float* seq, float* frame_feats, float* scores, float* recon_err, float* losses,
                   void* stream);
/* backward of the last full forward: use_loss = 1 -> of its train_model MSE, else the given output grads
 * (nullable = zero).  Writes every slot of the flat grad buffer. */
int vad_ae_backward(vad_ae_plan* plan, int use_loss, const float* d_recon, const float* d_seq,
                    const float* d_frame_feats, void* stream);
/* non-finite-grad skip, clip_grad_norm_(max_norm) and Adam with coupled L2 weight decay (cad1:350-351, 413-425);
 * grad_scale multiplies the grads first (1/world after a data-parallel sum) */
int vad_ae_optimizer_step(vad_ae_plan* plan, float lr, float beta1, float beta2, float eps, float weight_decay,
                          float max_norm, float grad_scale, void* stream);
/* Sliding-window scoring of a video (eval mode, forward only).  Replaces calculate_anomaly_scores' loop over clips
 * (cad1:542-552) on the clips the reference enumerates at stride T/4 (cad1:72), which encodes every frame once per
 * clip that holds it: with running BatchNorm statistics the encoder, Linear + tanh and the LSTM input projection
 * depend on the frame alone, so they run once per frame into a caller-owned frame cache, and windows then read frames
 * start + t of the cache.
 * The cache of a video of nframes frames holds two fields, each [nframes][...] and 64-float aligned: 0 lat [64] (the
 * frame's latent, tanh and NaN -> 0: frame_features), 1 gx [256] (W_ih lat + b_ih, gate order i, f, g, o).  The
 * frames themselves are not copied.  vad_ae_frame_cache_floats: its size in floats; vad_ae_frame_cache_offset: a
 * field's offset in floats (both -1 on a bad argument). */
int64_t vad_ae_frame_cache_floats(int64_t nframes);
int64_t vad_ae_frame_cache_offset(int64_t nframes, int field);
/* The per-frame stage on a plan created as (B = F, T = 1): the eval-mode encoder on the F frames frames_chunk
 * [F,1,64,64], lat and gx written to frames f0 .. f0 + F - 1 of the cache.  It stops after the gx GEMM: no recurrence,
 * decoder, loss, counter or ring update.  No parameter or buffer changes; the plan's activations of an earlier
 * forward do, so a vad_ae_backward of that forward fails ("needs a preceding full forward").  f0 + F > nframes is an
 * error and launches nothing. */
int vad_ae_frames_forward(vad_ae_plan* plan, const float* frames_chunk, int64_t nframes, float* cache, int64_t f0,
                          void* stream);
/* The per-window stage for windows w0 .. w0 + nw - 1 (window w = frames w*stride .. w*stride + T - 1; nw at most the
 * plan's B): the LSTM recurrence over the window's cached gx rows, the ring score of its last hidden state
 * (cad1:262-301), one decoder call (the reference stacks T copies of it, cad1:254-259), the mean over the window's
 * T*4096 pixels of (r - x)^2 against frames [nframes,1,64,64] (NaN -> 0 on both sides) and the blend 0.7 * error +
 * 0.3 * ring score (cad1:548-552).  Row i of every output is window w0 + i and equals vad_ae_forward(training = 0,
 * loss_mode = 1) on that clip.  Outputs: seq [nw,64] (16-byte aligned), recon_err [nw], mem_score [nw], score [nw],
 * recon [nw,4096] (nullable: one frame per window).  The plan's losses vector is not touched; a pending
 * vad_ae_backward of the plan fails as above.  T outside 1..nframes, stride < 1, nw outside 1..B or a window range
 * outside the video is an error and launches nothing. */
int vad_ae_windows_forward(vad_ae_plan* plan, const float* cache, const float* frames, int64_t nframes, int T,
                           int stride, int64_t w0, int nw, float* seq, float* recon_err, float* mem_score,
                           float* score, float* recon, void* stream);
/* The same two stages on a live stream of frames.  The window error re-reads the raw frames, so the ring holds them
 * beside the per-frame results: three arrays over cap slots, each 64-float aligned -- 0 lat [cap][64], 1 gx
 * [cap][256], 2 pix [cap][4096] (the frames with NaN -> 0), 17.25 KB per slot -- in which frame g, counted from the
 * start of the stream, lives in slot g mod cap.  vad_ae_ring_floats: its size in floats; vad_ae_ring_offset: a
 * field's offset in floats (both -1 on a bad argument: cap < 1, field outside 0..2).  The library keeps no record of
 * which frames a ring holds: that is the caller's bookkeeping -- a frame is resident from its
 * vad_ae_frames_forward_ring until a later one stores frame g + cap over it, and a window must be scored while all
 * its frames are. */
int64_t vad_ae_ring_floats(int64_t cap);
int64_t vad_ae_ring_offset(int64_t cap, int field);
/* vad_ae_frames_forward on a (B = k, T = 1) plan's k frames frames_chunk [k,1,64,64], stored as frames f0 .. f0 + k -
 * 1 of the ring (the chunk may straddle the wrap): the encoder writes the plan's own lat / gx rows, one store kernel
 * copies them and the plan's NaN -> 0 frames to their slots.  A null or unbound plan, a plan with T != 1, k > cap,
 * f0 < 0 or a null or misaligned pointer is an error, names the argument in vad_last_error and launches nothing. */
int vad_ae_frames_forward_ring(vad_ae_plan* plan, const float* frames_chunk, int64_t cap, float* ring, int64_t f0,
                               void* stream);
/* vad_ae_windows_forward for nw windows of the ring: window i < nw covers frames first_frame + i*stride + t, t < T,
 * and row i of every output equals vad_ae_forward(training = 0, loss_mode = 1) on that clip (outputs as
 * vad_ae_windows_forward; the frames come from the ring's pix array).  The batch must fit the ring: a null or unbound
 * plan, a plan with T != 1, T outside 1..cap, stride < 1, first_frame < 0, nw outside 1..the plan's B, a span
 * (nw - 1)*stride + T > cap or a null or misaligned pointer is an error, names the argument in vad_last_error and
 * launches nothing. */
int vad_ae_windows_forward_ring(vad_ae_plan* plan, const float* ring, int64_t cap, int T, int stride,
                                int64_t first_frame, int nw, float* seq, float* recon_err, float* mem_score,
                                float* score, float* recon, void* stream);
/* The same two stages for a group of streams that share launches: one ring allocation of total_slots slots (the
 * layout of vad_ae_ring_floats(total_slots) / vad_ae_ring_offset(total_slots, field)) holding total_slots / cap rings
 * of cap slots, ring s in slots s*cap .. (s+1)*cap - 1 of each of the three arrays.  Which slot a frame goes to and
 * which slots a window reads come from tables the caller passes as HOST pointers.  Each call validates its table entry
 * by entry on the host -- a violation returns non-zero, names the argument or the entry in vad_last_error and launches
 * nothing, so a bad table cannot cause a store or a load outside the ring -- and then copies it with one
 * hipMemcpyAsync on `stream` into dev_table, which the kernels read.  dev_table is caller-owned device memory, 16-byte
 * aligned, of at least vad_ae_group_table_bytes(B of the frames plan, nw) bytes (the destinations from byte 0, the
 * window rows after them; -1 on a bad argument); the library still owns no device memory.  The caller must not reuse
 * dev_table while an earlier call on ANOTHER stream may still read it; calls on one stream are ordered by the stream.
 * A pageable host table may be changed as soon as the call returns; a pinned one only once `stream` has passed the
 * copy. */
int64_t vad_ae_group_table_bytes(int64_t nf, int64_t nw);
/* vad_ae_frames_forward_ring on a (B, T = 1) plan's B frames, frame f stored to slot host_dst[f] of the three arrays,
 * or nowhere where host_dst[f] is -1 (a padding frame: it is encoded, nothing of it is kept).  A null or unbound plan,
 * a plan with T != 1, a null or misaligned pointer, total_slots outside 1..2^24, a host_dst[f] outside
 * -1 .. total_slots - 1 or two entries >= 0 that are equal is an error as above. */
int vad_ae_frames_forward_group(vad_ae_plan* plan, const float* frames_chunk, int64_t total_slots, float* ring,
                                const int32_t* host_dst, void* dev_table, void* stream);
/* vad_ae_windows_forward_ring for nw windows that may lie in different rings: host_windows holds two int64 per window,
 * (base, first) -- the window's frame t is slot base + ((first + t) wrapped once at cap) -- and row i of every output
 * equals vad_ae_forward(training = 0, loss_mode = 1) on that clip (outputs as vad_ae_windows_forward).  total_slots
 * must lie in 1..2^24 and be a multiple of cap, base must be a multiple of cap with base + cap <= total_slots,
 * 0 <= first < cap, 1 <= T <= cap, T <= 4096 and 1 <= nw <= the plan's B; the plan and the pointers as above.
 * dev_table is the one of the frames call on the same plan (the window rows lie after that plan's B destinations). */
int vad_ae_windows_forward_group(vad_ae_plan* plan, const float* ring, int64_t total_slots, int cap, int T,
                                 const int64_t* host_windows, int nw, void* dev_table, float* seq, float* recon_err,
                                 float* mem_score, float* score, float* recon, void* stream);
/* the memory ring of any VideoAutoEncoder: update_memory (cad1:201-219; n <= 500 features (n, 64)) and
 * compute_anomaly_score (cad1:262-301; n sequence features -> scores (n,)) */
/* test access to the last forward's pre-activations (the gradient tests pin their LeakyReLU decisions): "ey" idx l:
 * encoder conv l's raw output [T*B frames, t-major][H][W][Co]; "est" idx l: its per-frame-index BN state [T][8][Co]
 * (mean | invstd | scale | shift | ...); "dy" idx j < 3: decoder ConvTranspose2d j's raw output [B][H][W][Co]; "dst"
 * idx j: its BN state [8][Co]; "u": the decoder Linear's output [B][2048]; the LSTM's per-step state, rows t*B + b:
 * "lat" [T*B][64] frame latents, "gx" [T*B][256] input projection, "gates" [T*B][256] activated gates (i f g o), "cs"
 * [T*B][64] cell state, "dG" [T*B][256] the backward's d pre-activation gates; "seq" [B][64] the sequence feature.
 * Device pointers (vad_debug_d2h). */
int vad_ae_debug_buffer(vad_ae_plan* plan, const char* name, int idx, void** ptr, int64_t* nfloats);
int vad_ae_update_memory(float* memory, int64_t* memory_ptr, const float* features, int n, void* stream);
int vad_ae_memory_score(const float* memory, const int64_t* memory_ptr, const float* seq, int n, float* scores,
                        void* stream);

/* Host data path.
 * vad_u8_to_clip: n u8 pixels -> fp32; mode 0: (u8 - 0.5) / 0.5 (UCSDped2Dataset + Normalize, cad:85-104,
 *   1177-1179), mode 1: u8 / 255 (ToTensor, mc:120 / bbox:411).  src (in HBM, or pinned host memory at the address
 *   vad_host_device_ptr gives) and dst 16-byte aligned.
 * vad_host_device_ptr: the device address of pinned host memory (the ClipStager's direct mode reads batches there).
 * vad_resize_u8 (host): bilinear u8 resize, half-pixel centres, clamped borders, 11-bit fixed-point weights (the
 *   cv2.resize INTER_LINEAR scheme of cad:88-89). */
int vad_u8_to_clip(const uint8_t* src, int64_t n, int mode, float* dst, void* stream);
int vad_host_device_ptr(const void* host, void** dev);
int vad_resize_u8(const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw);

/* Ingest for scoring: u8 frames at the source's own size -> fp32 (nf, 1, dh, dw) contiguous at dst, in
 * one launch.  Every output pixel is vad_resize_u8's pixel pushed through the normalisation, bit for bit: mode 0 and 1
 * as vad_u8_to_clip, mode 2: fminf(fmaxf(u8 / 255, 0.001), 0.999) (the autoencoder's dataset, cad1:110-114).  Sources
 * lie in HBM or in pinned host memory at the address vad_host_device_ptr gives; rows are pitch >= sw bytes apart and
 * need no alignment.  Any sh, sw, dh >= 1; 1 <= dw <= 4096 (the kernel's LDS column table); a source frame (sh * pitch
 * bytes) and dst (nf * dh * dw * 4 bytes) stay below 2 GB; dst 16-byte aligned.
 * vad_ingest_u8: nf frames of one size, frame f at src + f * frame_stride bytes.
 * vad_ingest_u8_table: frame f is row f of host_table, four int64 (device address, sh, sw, pitch); address 0 writes a
 *   frame of zeros and its sizes are not read.  Every row is validated first (an error names the entry and nothing is
 *   queued), then the table is copied with one hipMemcpyAsync into dev_table -- caller-owned device memory, 16-byte
 *   aligned, of at least vad_ingest_table_bytes(nf) bytes -- and the kernel reads it there.  host_table must stay
 *   unchanged until that copy has run (pinned memory: the copy is asynchronous). */
int vad_ingest_u8(const uint8_t* src, int64_t nf, int sh, int sw, int64_t pitch, int64_t frame_stride, int dh, int dw,
                  int mode, float* dst, void* stream);
int64_t vad_ingest_table_bytes(int64_t nf);
int vad_ingest_u8_table(const int64_t* host_table, int64_t nf, int dh, int dw, int mode, float* dst, void* dev_table,
                        void* stream);

/* Colour ingest: packed colour pixels of step bytes with R, G, B at fixed byte offsets --
 * fmt 0 rgb, 1 bgr (step 3), 2 rgbx, 3 bgrx (step 4; the fourth byte is never read) -- rows pitch >= step * sw bytes
 * apart, no alignment; everything else as the grey pair above, whose checks these take over.
 * planes 1: fp32 (nf, 1, dh, dw), grey.  Luma L = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16 (PIL's
 *   convert("L")) of each of a pixel's four source taps, then vad_resize_u8's blend of the four luma values and the
 *   mode's pixel function: bit for bit vad_luma_u8 at the source size -> vad_resize_u8 -> the normalisation.
 * planes 3: fp32 (nf, 3, dh, dw), planes R, G, B whatever the source order; each plane is vad_resize_u8 of that channel
 *   and the mode's pixel function (mode 1: the bbox scorer's cv2.resize -> BGR2RGB -> / 255, bbox:399-411).
 * dst (nf * planes * dh * dw * 4 bytes) stays below 2 GB.  The table form reads the grey form's rows (address, sh, sw,
 * pitch; vad_ingest_table_bytes); address 0 writes zeros to all planes of the frame.  fmt and planes hold for the whole
 * launch.
 * vad_luma_u8 (host): the same luma of one (sh, sw) frame of packed pixels into dst (sh, sw), contiguous. */
int vad_luma_u8(const uint8_t* src, int sh, int sw, int64_t pitch, int fmt, uint8_t* dst);
int vad_ingest_u8_color(const uint8_t* src, int64_t nf, int sh, int sw, int64_t pitch, int64_t frame_stride, int fmt,
                        int planes, int dh, int dw, int mode, float* dst, void* stream);
int vad_ingest_u8_color_table(const int64_t* host_table, int64_t nf, int fmt, int planes, int dh, int dw, int mode,
                              float* dst, void* dev_table, void* stream);

/* Plan options.  "conv_bf16" (0/1): the 3x3 convs of the backbone run on bf16 operands with fp32 accumulation
 * (BASELINE config 4's bf16 compute; BN, pooling, heads, losses and the optimizer stay fp32).  Default 0: fp32
 * numerics (split-bf16 products).  "stem_grad" (0/1): backbone.conv1 / bn1 train (the module without
 * apply_memory_efficient_training, cad:592-598); set before the forward.  "wgrad_stream" (0/1, default 1): the
 * backbone's weight gradients run on a plan-owned stream beside the input gradients (results identical).
 * "opt_images" (0/1, default 1): vad_cad_optimizer_step also writes every new conv weight / detector layer-1..4
 * weight into the plan's derived images of it (relayouts, transposes), so the next forward runs no relayout; results
 * identical.  "images_fresh" (only 0): the caller changed the parameters itself (any write other than this plan's
 * vad_cad_optimizer_step -- another plan's step on the same buffer included): the next forward relayouts.  A plan
 * cannot see such writes; without this call it would compute with the images of the old parameters. */
int vad_cad_set_option(vad_cad_plan* plan, const char* key, int64_t value);
/* Kernel family of backbone 3x3 conv `layer` (0..7) for kind 0 forward / 1 input gradient / 2 weight gradient:
 * 6 = split-bf16 (fp32 numerics, six bf16 MFMA products per K step), 1 = bf16 operands, 0 = f32 MFMA; -1 on error.
 * (bench.py prices each launch against the peak of the instruction mix it runs.) */
int vad_cad_conv_path(vad_cad_plan* plan, int layer, int kind);

/* ------------------------------------------------------------------------------------------
 * Debug introspection (tests only): internal plan buffers, partial backward, device->host copy
 * names: y1, pool, y[0..7], stats[0..8], feats, pooled, dA, dY, d_pooled, d_feat_det, det_logits, the weight
 * images wf[0..7], wd[0..7] (whole buffers: fp32 image | bf16 copy or planes), wt[1..4]; images_fresh (value in nfloats)
 * ------------------------------------------------------------------------------------------ */
int vad_cad_debug_buffer(vad_cad_plan* plan, const char* name, int idx, void** ptr, int64_t* nfloats);
int vad_cad_set_debug(vad_cad_plan* plan, const char* key, int64_t value);  /* "stop_layer" */
int vad_debug_d2h(void* host, const void* dev, int64_t bytes);
/* HIP-event timing of labelled launches (conv_fwd/L<l>, conv_wgrad/L<l>, conv_dgrad/L<l>, bn_bwd_*, conv1,
 * det_fwd, head_fwd, optimizer, ...).  enable: 0 pauses (records kept), 1 clears the records and starts, 2 starts
 * appending.  only_prefix restricts the labels recorded; with a non-empty prefix the labelled conv kernels are
 * dispatched with their own start/stop events (hipExtLaunchKernel) instead of event records around the launch. */
int vad_cad_profile(vad_cad_plan* plan, int enable, const char* only_prefix);
int vad_cad_profile_read(vad_cad_plan* plan, char* labels, double* total_ms, int* counts, int cap);
/* per-record label / start / end (ms after the first record), record order (bench.py: the post-backbone chain) */
int vad_cad_profile_marks(vad_cad_plan* plan, char* labels, double* t0_ms, double* t1_ms, int cap);

#ifdef __cplusplus
}
#endif
#endif /* VAD_H_ */
