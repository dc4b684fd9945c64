// The library's tuning knobs: one line per knob -- key of vad_set_tuning / vad_get_tuning, variable, default, meaning.
// The list defines the variables (tuning.hip), declares them for the files that read them (below) and is the table
// set_tuning() looks a key up in.  A new knob is one line here plus its use.
// G: process-global.  T: thread_local (the ops API's modes of the calling thread; plans set them per call).
#pragma once

#define VAD_TUNING_KNOBS(G, T)                                                                                        \
  /* conv GEMMs and LDS-patch kernels (backbone.hip, conv_patch.hip) */                                               \
  G(conv_fwd_tile, g_conv_fwd_tile, -1, "forced tile id of the GEMM forwards (-1: heuristic; ids: with_tile)")        \
  G(conv_dgrad_tile, g_conv_dgrad_tile, -1, "forced tile id of the GEMM input gradients (-1: heuristic)")             \
  G(conv_wgrad_tile, g_conv_wgrad_tile, -1, "forced tile id of the GEMM weight gradients (-1: heuristic)")            \
  G(conv_wgrad_blocks, g_conv_wgrad_blocks, 1024, "target grid size of the split-K weight gradient")                  \
  G(conv_wgrad_min_ktiles, g_conv_wgrad_min_ktiles, 16, "minimum BK-slices per split")                                \
  G(conv_patch, g_conv_patch, 1, "stride-1 fwd/dgrad on the LDS-patch kernels")                                       \
  G(conv_patch_persist, g_patch_persist, 1,                                                                           \
    "single-chunk (C == 32) stride-1 layers on the persistent patch kernel")                                          \
  G(conv_wgrad_patch, g_conv_wgrad_patch, 1, "weight gradients on the LDS-patch kernel: 1 stride-1 layers, 2 all")    \
  G(conv_wgrad_patch_blocks, g_conv_wgrad_patch_blocks, 448,                                                          \
    "its target grid size (below 2 per CU: the weight gradients share the GPU with the input gradients, own stream)") \
  /* split-bf16 kernels (conv_x3.hip, conv_x3w.hip) */                                                                \
  G(conv_split, g_conv_split, 1, "1 = split-bf16 patch kernels where supported, 0 = f32 MFMA patch kernels")          \
  G(conv_dgrad_s2_x3, g_dgrad_s2_x3, 1, "stride-2 input gradients on the split-bf16 kernel")                          \
  G(conv_dgrad_s2_w3, g_dgrad_s2_w3, 1, "the plan pre-splits the stride-2 Wd images into bf16 planes")                \
  G(conv_wgrad_split, g_wgrad_split, 1, "stride-1 weight gradients on the split-bf16 kernel (2: 8x8 frames too)")     \
  G(conv_wgrad_split_s2, g_wgrad_split_s2, 1, "stride-2 weight gradients on the split-bf16 kernel")                   \
  G(conv_wgrad_tr, g_wgrad_tr, 1, "fp32 weight gradients on x3_wgrad_tr_kernel")                                      \
  G(conv_wgrad_tr_blocks, g_wgrad_tr_blocks, 384,                                                                     \
    "its target grid (1.5 blocks per CU: they share the CUs with the input gradients)")                               \
  G(conv_wgrad_tr_pft, g_wgrad_tr_pft, 0,                                                                             \
    "the next tap's input fragments read before this tap's MFMAs (off: config-2 step 1.696 ms off vs 1.72-1.74 on, "  \
    "profiles/r05_prefetch_ab.json)")                                                                                 \
  T(conv_bf16, g_conv_bf16, 0,                                                                                        \
    "bf16-operand convs (one plane, one product); ops API only (calling thread), plans use their own option")         \
  T(act_bf16, g_act_bf16, 0, "bf16 activation storage; ops API only (calling thread), plans use their own option")    \
  /* stem, BatchNorm, detector MLP */                                                                                 \
  G(stem_fused, g_stem_fused, 1, "the frozen stem's forward without the conv1 activation")                            \
  G(bn_apply_u, g_bn_apply_u, 4, "streaming BN-backward apply: rows in flight per thread (2, 4, 8)")                  \
  G(bn_apply_blocks, g_bn_apply_blocks, 2048, "streaming BN-backward apply: grid cap (grid-stride beyond it)")        \
  G(mlp_tail_rb, g_mlp_tail_rb, 0, "rows per block of the detector's layers 1-4 (0: auto)")                           \
  G(mlp_tail_wide, g_mlp_tail_wide, 1,                                                                                \
    "1024-thread blocks for the detector's layers 1-4 (4 x the K-slices and split-K loads in flight of 256 threads; " \
    "profiles/r03_mlp_tail_sweep.txt)")                                                                               \
  /* cad plan (cad_plan.hip) */                                                                                       \
  G(cad_prep_stream, g_cad_prep_stream, 1, "weight relayouts on the plan's side stream (A/B measurement)")            \
  G(cad_stem_early, g_cad_stem_early, 1, "an armed forward (vad_cad_input_ready) runs its stem early (0: off)")       \
  G(cad_det_gate, g_cad_det_gate, 1, "the backbone backward waits on the device detector gate")                       \
  G(cad_dir_affine, g_cad_dir_affine, 1, "direct classifier backward as A + c beta, precomputed in the forward")      \
  G(cad_opt_images, g_cad_opt_images, 1,                                                                              \
    "the fused optimizer writes the weight images it invalidates (0: the forward relayouts every time)")              \
  /* 3-D clip models: minicausal, bbox, cad1's autoencoder, a2 */                                                     \
  G(conv3d_direct, g_conv3d_direct, 1, "the minicausal convs on the direct kernels (0: im2col + GEMM)")               \
  G(maxpool3d_bwd_win, g_maxpool_bwd_win, 1, "one thread per window (0: one per input element)")                      \
  G(bbox_im2col, g_bbox_im2col, 0, "the bbox scorer's convs as im2col columns + f32 MFMA GEMMs")                      \
  G(ae_direct, g_ae_direct, 1, "cad1's convs as implicit GEMMs over NHWC frames (latched per plan)")                  \
  G(ae_wgrad_stream, g_ae_wgrad_stream, 1,                                                                            \
    "latched per plan, direct mode: the backward's weight gradients run on a low-priority stream of the plan beside " \
    "the input-gradient chain, on their own split-K scratch, with dY alternating between two buffers")                \
  G(conv4_split_tiles, g_conv4_split_tiles, 512,                                                                      \
    "implicit-GEMM convs with fewer 64 x 64 output tiles than this split K (slabs + a reduce)")                       \
  G(conv4_cls_batch_min, g_conv4_cls_batch_min, 0,                                                                    \
    "the four parity classes go to one batched launch (whole K per block, bias in the epilogue) from this many "      \
    "64 x 64 class tiles up; below it, per-class split-K launches with a reduce each (sweep at cad1: 512 "            \
    "1.845-1.850, 128 1.813-1.817, 0 1.785-1.795 ms)")                                                                \
  G(a2_direct, g_a2_direct, 1, "conv3d_1 direct on the VALU (latched per plan; 0: im2col + GEMM)")                    \
  G(a2_head_clip, g_a2_head_clip, 1, "the head forward / backward one block per clip (0: one launch per layer)")

namespace vad {

#define VAD_KNOB_G(key, var, def, doc) extern int var;
#define VAD_KNOB_T(key, var, def, doc) extern thread_local int var;
VAD_TUNING_KNOBS(VAD_KNOB_G, VAD_KNOB_T)
#undef VAD_KNOB_G
#undef VAD_KNOB_T

// set / get: 0, or 1 with the error "unknown tuning key <key>".  tuning_name: the i-th key, null past the end
int set_tuning(const char* key, int value);
int get_tuning(const char* key, int* value);
const char* tuning_name(int i);

}  // namespace vad
