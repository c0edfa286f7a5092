// Every host launcher that capi.hip calls, declared once with the parameter names of its definition.  capi.hip and each defining
// .hip include this header: a definition that drifts from its declaration becomes an overload nobody declared, and the call in
// capi.hip stops compiling or linking.  Default arguments live here only.  Grouped by defining file; "returns" is the group's
// convention (capi.hip maps both conventions to the C ABI's codes).
#pragma once
#include "common.h"

namespace univs {

// ---- msda_fwd.hip: returns UNIVS_OK or the launch's error
int msda_forward_generic_f32(const float* value, const LevelTable& lv, const float* loc,
                             const float* attn, int N, int S, int M, int D, int L, int Lq, int P,
                             float* out, hipStream_t st);
int msda_forward_generic_f64(const double* value, const LevelTable& lv, const double* loc,
                             const double* attn, int N, int S, int M, int D, int L, int Lq, int P,
                             double* out, hipStream_t st);

// ---- msda_tiled2.hip: returns 1 if launched, 0 if not covered, < 0 on error
int msda_forward_tiled2_f32(const float* value, const LevelTable& lv, const float* loc, const float* attn, int N,
                            int S, int M, int D, int L, int Lq, int P, float* out, hipStream_t st);

// ---- msda_strips.hip: returns 1 if launched, 0 if not covered, < 0 on error
int msda_forward_strips_f32(const float* vhm, const LevelTable& lv, const float* qhm, const float* ref,
                            long long ref_batch_stride, int N, int S, int M, int D, int L, int Lq, int P, float* out,
                            hipStream_t st);

// ---- msda_heads.hip: returns 1 if launched, 0 if not covered, < 0 on error
int msda_forward_heads_f32(const float* vhm, const LevelTable& lv, const float* qhm, const float* ref,
                           long long ref_batch_stride, int N, int S, int M, int D, int L, int Lq, int P, float* out,
                           hipStream_t st);

// ---- msda_bwd.hip: returns UNIVS_OK or the launch's error
int msda_backward_f32(const float* value, const LevelTable& lv, const float* loc, const float* attn,
                      const float* grad_out, int N, int S, int M, int D, int L, int Lq, int P, float* grad_value,
                      float* grad_loc, float* grad_attn, hipStream_t st);

// ---- msda_prepare.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int msda_prepare_f32(const float* qp, int row_stride, int n_off, const float* ref, long long ref_batch_stride,
                     const LevelTable& lv, int N, int Lq, int M, int L, int P, float* loc, float* attn, hipStream_t st);

// ---- mask_decode.hip: returns UNIVS_OK or the launch's error; mask_decode_last_impl: the kernel the last mask_decode_f32 of this thread ran
int mask_decode_f32(const float* mask_embed, const float* mask_features, int T, int Q, int C,
                    long long HW, float* out, hipStream_t st);
int mask_decode_last_impl();
int mask_decode_attn_f32(const float* mask_embed, const float* feat_lowres, int T, int Q, int C,
                         long long hw, uint8_t* attn_mask, unsigned* row_any_ws, unsigned generation, hipStream_t st);
int attn_mask_rows_reset(uint8_t* attn_mask, const unsigned* row_flags, unsigned generation, long long rows, long long hw, hipStream_t st);

// ---- linear_split.hip: returns 1 if launched, 0 if not covered, < 0 on error
int linear_split_f32(const float* x, const float* w, const float* bias, const float* residual, float* y, long long M, int N,
                     int K, int epi, hipStream_t st, int blk_rows = 0, int blk_cols = 0, const float* winv = nullptr);

// ---- linear_f16x3.hip: returns 1 if launched, 0 if not covered, < 0 on error
int linear_f16x3_f32(const float* x, const float* w, const float* bias, const float* residual, float* y, long long M, int N,
                     int K, int epi, hipStream_t st, int blk_rows, int blk_cols, const float* winv, int n_cu);

// ---- linear_pair_f16x3.hip: returns 1 if launched, 0 if not covered, < 0 on error
int linear_pair_f16x3_f32(const float* x, const float* add, long long add_rows, const void* wp_a, const float* winv_a, const float* bias_a,
                          int N_a, int blk_cols_a, float* y_a, const void* wp_b, const float* winv_b, const float* bias_b, int N_b,
                          int blk_cols_b, float* y_b, long long M, int K, long long blk_rows, hipStream_t st);

// ---- gemm_f16x3_stream.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int conv3x3_nhwc_f16x3_f32(const float* x, const void* wp, const float* winv, float* y, int T, int Cin, int Cout, int H, int W,
                           hipStream_t st);
int presplit_f16x3(const float* w, int N, int K, int conv_cin, int kperm, void* wp, float* winv, hipStream_t st);
int linear_f16x3_stream_f32(const float* x, const void* wp, const float* winv, const float* bias, const float* residual, float* y,
                            long long M, int N, int K, int epi, hipStream_t st);
int conv3x3_f16x3_f32(const float* x, const void* wp, const float* winv, float* y, int T, int Cin, int Cout, int H, int W,
                      hipStream_t st);
int conv1x1_f16x3_f32(const float* x, const void* wp, const float* winv, const float* bias, float* y, int T, int Cin, int Cout, int H,
                      int W, hipStream_t st);
int conv1x1_fused_f16x3_f32(const float* x, int channels_last, const float* affine, const void* wp, const float* winv, const float* bias,
                            float* y, int T, int Cin, int Cout, int H, int W, hipStream_t st);

// ---- conv3x3_wide.hip: returns 1 if launched, 0 if not covered (or switched off), < 0 on error.  xmode 1: x [T, Cin, H, W]; 2: x [T, H, W, Cin]
int conv3x3_wide_f32(int xmode, const float* x, const void* wp, const float* winv, float* y, int T, int Cin, int Cout, int H, int W,
                     hipStream_t st);

// ---- gemm_f16x3_tile.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int linear_f16x3_tile_f32(const float* x, const void* wp, const float* winv, const float* bias, const float* residual, float* y,
                          long long M, int N, int K, int epi, hipStream_t st);

// ---- mlp_f16x3.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int mlp_f16x3_f32(const float* x, const void* w1p, const float* w1inv, const float* b1, const void* w2p, const float* w2inv,
                  const float* b2, const float* residual, const float* ln_w, const float* ln_b, float ln_eps, const float* pln_w,
                  const float* pln_b, float pln_eps, const float* post_add, long long post_add_rows, float* y2, float* y, long long M,
                  int C, int Hd, int act, int flags, hipStream_t st);

// ---- small_linear.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int small_chain_f32(const float* x, int stages, const void* const* wp, const float* const* winv, const float* const* bias, const int* relu,
                    const float* in_g, const float* in_b, float in_eps, float* xn, float* y, long long M, int out_T, hipStream_t st);
int small_linear_f32(const float* x, const float* xadd, const void* wp, const float* winv, const float* bias, int n_w, int f_off,
                     const float* residual, const float* ln_g, const float* ln_b, float ln_eps, float* y, long long M, int N, int K,
                     int relu, int add_features, int out_T, hipStream_t st);
int small_linear_merged_f32(const float* ws, int plan, int L, int Nb, int Hh, const void* wp, const float* winv, const float* bias, int n_w,
                            int f_off, const float* residual, const float* ln_g, const float* ln_b, float ln_eps, float* y, int N,
                            hipStream_t st);
int small_seam_f32(const float* x, const void* wpa, const float* winv_a, const float* bias_a, const float* residual, const float* ln_g,
                   const float* ln_b, float ln_eps, float* t, const float* add, const void* wpb, const float* winv_b, const float* bias_b,
                   int n_wb, int f_off, float* y, long long M, int Ka, int Na, int Nb, int relu, int add_features, hipStream_t st);
int small_chain_seam_f32(const float* x, const float* pre_res, const float* pre_g, const float* pre_b, float pre_eps, float* xr,
                         const float* side_add, const void* side_wp, const float* side_winv, const float* side_bias, int side_nw,
                         int side_f_off, float* side_y, int stages, const void* const* wp, const float* const* winv,
                         const float* const* bias, const int* relu, const float* in_g, const float* in_b, float in_eps, float* xn, float* y,
                         long long M, int out_T, hipStream_t st);

// ---- cross_attn.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error; cross_attention_workspace_floats: a count
int cross_attention_f32(const float* q, const float* k, const float* v, const unsigned char* mask, const unsigned* row_flags,
                        unsigned generation, int L, int S, int N, int H, int hd, int ldq, int ldk, int ldv, float scale, float* ws,
                        float* out, hipStream_t st);
int cross_attention_partials_f32(const float* q, const float* k, const float* v, const unsigned char* mask, const unsigned* row_flags,
                                 unsigned generation, int L, int S, int N, int H, int hd, int ldq, int ldk, int ldv, float scale, float* ws,
                                 int* plan_out, hipStream_t st);
size_t cross_attention_workspace_floats(int L, int S, int N, int H);

// ---- window_attn.hip: returns UNIVS_OK or the launch's error
int window_attention_image_f32(const float* qkv, const float* qkv_bias, const float* bias, const float* shift_mask,
                               int B, int H, int W, int ws, int shift, int nH, int hd, float scale, float* out,
                               hipStream_t st);
int window_attention_f32(const float* qkv, const float* bias, const float* shift_mask, int B_, int nW,
                         int Ntok, int nH, int hd, float scale, float* out, hipStream_t st);

// ---- window_attn_f16.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int window_attention_image_f16mma(const float* qkv, const float* qkv_bias, const float* bias, const float* shift_mask, int B,
                                  int H, int W, int ws, int shift, int nH, int hd, float scale, int terms, float* out,
                                  hipStream_t st);

// ---- window_attn_qkv.hip: returns 1 if launched, 0 if not covered, < 0 on error
int window_attention_qkv_f16x3(const float* x, const void* wp, const float* winv, const float* qkv_bias, const float* bias,
                               const float* shift_mask, int B, int H, int W, int ws, int shift, int nH, int C, float scale, float* out,
                               hipStream_t st);

// ---- resample.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int bilinear_resample_f32(const float* in, const float* addend, float* out, long long planes, int Hin, int Win,
                          int Hout, int Wout, hipStream_t st);
int upsample2x_add_f32(const float* in, const float* addend, const float* affine, float* out, long long planes, int Hin, int Win,
                       hipStream_t st);
int normalize_pad_f32(const float* in, float* out, long long T, int C, int H, int W, int Hp, int Wp, const float* mean, const float* stdv,
                      hipStream_t st);
int bilinear_pyramid3_f32(const float* in, float* out2, float* out4, float* out8, long long planes, int H, int W, hipStream_t st);

// ---- semantic_extract.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int bilinear_crop_nearest_f32(const float* in, float* out, int C, int h, int w, int Hp, int Wp, int Hi, int Wi, int hc, int wc, int t_first,
                              int t_step, int K, hipStream_t st);

// ---- layer_norm.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int layer_norm_f32(const float* x, const float* res, const float* gamma, const float* beta, long long rows, int C,
                   float eps, float* sum_out, float* out, const float* addend, float* out2, long long addend_rows, hipStream_t st);
int patch_merge_norm_f32(const float* x, const float* gamma, const float* beta, int B, int H, int W, int C, float eps, float* out,
                         hipStream_t st);

// ---- group_norm.hip: returns UNIVS_OK or the launch's error
int group_norm_affine_f32(const float* x, const float* gamma, const float* beta, int N, int C, long long HW, int groups, float eps,
                          float* ws, long long ws_floats, float* affine, hipStream_t st);
int group_norm_f32(const float* x, const float* gamma, const float* beta, int N, int C, long long HW, int groups,
                   float eps, int relu, float* ws, long long ws_floats, float* out, hipStream_t st);

// ---- softmax.hip: returns UNIVS_OK or the launch's error
int masked_softmax_f32(float* scores, const unsigned char* mask, int N, int h, int L, int S, hipStream_t st);

// ---- proca_attn.hip: returns 1 if launched, 0 if not covered, < 0 on error
int proca_attention_f32(const float* qkv0, const float* kd, const float* vd, int Qp, int L, int T, int h, int hd, float scale,
                        float* out, hipStream_t st);

// ---- prompt_sampler.hip: returns UNIVS_OK or the launch's error; prompt_draw and token_mean_f32: 1 if launched, 0 if not covered, < 0 on error
int prompt_prefix_f32(const float* masks, const float* boxes, int Fk, int n, int h, int w, int scale, float feat_thresh,
                      float* feat_masks, unsigned* stats, uint8_t* sel, int* rowcnt, uint8_t* fmb, int* counts, uint8_t* valid,
                      uint8_t* visible, hipStream_t st);
int prompt_draw(const uint8_t* sel, const int* rowcnt, const uint8_t* fmb, const int* counts, const float* u, const float* keys,
                const long long* tab, int Fk, int n, int h, int w, int HW, int R, long long* point_idx, long long* dense_idx,
                uint8_t* empty, float* point_coords, hipStream_t st);
int prompt_point_pe_f32(const float* xy, const float* z, const float* dim_t, const float* dim_tz, float scale, int Fk, int n, int F,
                        float* out, hipStream_t st);
int token_mean_f32(const float* x, const float* add, int n, int L, int T, int C, float* out, hipStream_t st);
int prompt_tokens_f32(const float* feats, const long long* fs, const float* pos, const long long* ps, const float* qfeat,
                      const float* qpe, const long long* dense_idx, const uint8_t* empty, const uint8_t* valid, const float* boxes,
                      const long long* kf, int Fk, int n, int R, int T, int C, int h_img, int w_img, float* fd, float* pd, uint8_t* attn,
                      hipStream_t st);

// ---- transpose.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int transpose_f32(const float* in, float* out, long long B, int R, int C, long long in_bstride, long long out_bstride,
                  const float* row_affine, const float* addend, float* out2, hipStream_t st);
int decoder_memory_f32(const float* x, const float* level_embed, const float* yx, const float* pos_z, float* mem, float* key, int T, int C,
                       int HW, hipStream_t st);
int patch_embed4_f32(const float* x, const float* w, const float* bias, const float* ln_g, const float* ln_b, float eps, float* out, int T,
                     int H, int W, int E, hipStream_t st);

// ---- mask_stats.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int mask_stats_f32(const float* x, long long planes, int inner, long long stride_outer, long long stride_inner, int H, int W, int hv, int wv,
                   float t_hi, float t_lo, float t_box, int* out, hipStream_t st);

// ---- image_post.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int image_mask_stats_f32(const float* L, int Q, int h, int w, int Hp, int Wp, int hi, int wi, int* out, hipStream_t st);
int image_panoptic_ids_f32(const float* L, int Q, int h, int w, int Hp, int Wp, int hi, int wi, const int* planes, const float* scores, int K,
                           int* ids, int* counts, hipStream_t st);
int image_panoptic_paint_i32(const int* ids, int hi, int wi, const int* lut, int K, int H0, int W0, int* out, int* seen, hipStream_t st);
int image_semseg_f32(const float* L, int Q, int h, int w, int Hp, int Wp, int hi, int wi, const int* planes, const float* P, int Qs, int C,
                     float* R, hipStream_t st);
int image_instance_masks_u8(const float* L, int Q, int h, int w, int Hp, int Wp, int hi, int wi, const int* planes, int N, int H0, int W0,
                            unsigned char* masks, int* boxes, hipStream_t st);

// ---- video_post.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int minvis_accumulate_f32(float* S, int Q, int V, int h, int w, const float* M, int Qm, int T, const int* perm, int i, hipStream_t st);
int video_mask_stats_f32(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int* rows, int K, int step,
                         int* counts, hipStream_t st);
int video_instance_masks_u8(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int* rows, int N, int H0,
                            int W0, unsigned char* masks, hipStream_t st);
int video_panoptic_ids_i32(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int* rows, const float* scores,
                           int K, int* ids, hipStream_t st);
int video_panoptic_counts_i32(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int* rows, int K,
                              const int* ids, int H0, int W0, int* counts, hipStream_t st);
int video_panoptic_paint_i32(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int* rows, int K,
                             const int* ids, const int* lut, int H0, int W0, int* out, hipStream_t st);

// ---- pair_count.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int panoptic_pair_counts(const void* gt, int gt_rgb, const void* pred, int pred_rgb, int T, int H, int W, const int* gt_ids, int G,
                         const int* pred_ids, int P, int* counts, int* first_unknown, hipStream_t st);

// ---- vss_count.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int vss_video_counts(const unsigned char* gt, const unsigned char* pred, int T, int H, int W, int C, int* confusion, int* windows,
                     int* overflow, hipStream_t st);

// ---- davis_count.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape or alignment is not covered, or the launch's error
int davis_counts(const unsigned char* gt, const unsigned char* pred, int T, int H, int W, int G, int P, int radius, int use_void,
                 int* region, int* n_gt, int* n_fg, int* match, hipStream_t st);

// ---- vis_overlap.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the shape is not covered, or the launch's error
int vis_overlap_counts(const int* dt_bounds, const int* dt_starts, const int* gt_bounds, const int* gt_ones, const int* gt_starts, int D,
                       int G, int T, int H, int W, int gt_max_bounds, int* inter, hipStream_t st);

// ---- pvos_count.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the sizes are not covered, or the launch's error
int pvos_counts(const unsigned char* gt, const unsigned char* pred, int T, int H, int W, int d, int K, int* counts, hipStream_t st);

// ---- semantic_decode.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the sizes are not covered, or the launch's error
int semantic_quality_counts_f32(const float* mask_embed, const float* features, int T, int N, int C, int HW, int t_step, float t_hi,
                                float t_lo, int* counts, hipStream_t st);

// ---- frame_resize.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the sizes are not covered, or the launch's error
int resize_frames_u8(const unsigned char* src, int T, int Hi, int Wi, int Ho, int Wo, const int* first_x, const int* count_x,
                     const int* coef_x, int ksize_x, const int* first_y, const int* count_y, const int* coef_y, int ksize_y, int swap_rb,
                     unsigned char* out, hipStream_t st);

// ---- mask_prompt_resize.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the sizes are not covered, or the launch's error
int resize_rle_masks_u8(const int* bounds, const int* starts, long long n_bounds, int N, int H, int W, const int* ty, const int* tx, int Ho,
                        int Wo, unsigned char* masks, int* boxes, hipStream_t st);

// ---- idmap_prompts.hip: return UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the sizes are not covered, or the launch's error
int idmap_census_u8(const unsigned char* ids, int F, int H, int W, int* count, int* box, hipStream_t st);
int idmap_prompts_u8(const unsigned char* ids, int F, int H, int W, const int* frame, const int* value, int N, const int* ty, const int* tx,
                     int Ho, int Wo, unsigned char* masks, int* boxes, hipStream_t st);

// ---- semseg_labels.hip: return UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the sizes are not covered, or the launch's error
int semseg_labels_f32(const float* r, int C, int hi, int wi, int H, int W, unsigned char* labels, hipStream_t st);
int label_confusion_u8(const unsigned char* gt, const unsigned char* pred, long long n, int K, int ignore_label, long long* conf,
                       long long* stray, hipStream_t st);

// ---- text_attn.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the sizes are not covered, or the launch's error
int text_attention_f32(const float* qkv, const int* start, int S, long long Ntok, int E, int heads, int Lmax, float scale, float* out,
                       hipStream_t st);

// ---- polygon_runs.hip: returns UNIVS_OK or the launch's error (the entry answers what is not covered)
int polygons_to_runs(const double* xy, const int* poly_start, const int* obj_start, const int* size, const long long* slot, long long n_points,
                     int P, int N, long long cap_total, int* bounds, int* ones, int* count, int* status, hipStream_t st);

// ---- png_deflate.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the sizes are not covered, or the launch's error
int png_deflate_maps(const void* src, int src_is_i32, int N, int H, int W, const unsigned char* lut, int K, int C, int rows_per_stripe,
                     unsigned char* scratch, unsigned char* out, long long* offsets, hipStream_t st);

// ---- png_inflate.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the sizes are not covered, or the launch's error
int png_read(const unsigned char* streams, const long long* stream_offsets, const int* desc, const unsigned char* palettes, int P,
             const long long* filt_offsets, const long long* out_offsets, int N, long long streams_total, long long filt_total,
             long long out_total, int max_rowbytes, unsigned char* filtered, unsigned char* out, int* status, hipStream_t st);

// ---- jpeg_decode.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the sizes or the sampling are not covered, or the launch's error
int jpeg_decode(const unsigned char* src, const long long* src_off, const int* ri, const unsigned char* huff, const unsigned short* quant, int N,
                int W, int H, int ncomp, int h, int v, int subseq_bits, int max_intervals, long long src_total, int phases, unsigned char* comp,
                int* ivl, short* blocks, unsigned char* planes, unsigned char* out, int* status, int* rounds, hipStream_t st);

// ---- jpeg_encode.hip: returns UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the sizes, the sampling or the quality are not covered, or the
// launch's error
int jpeg_encode(const unsigned char* rgb, const void* ids, int ids_is_i32, const unsigned char* lut, int K, int edge, int N, int H, int W, int h,
                int v, int quality, int phases, short* blocks, unsigned* sizes, long long* bit_off, long long* totals, const long long* raw_off,
                long long raw_total, unsigned char* raw, unsigned char* out, long long* out_len, int* status, hipStream_t st);

// ---- hota_count.hip: return UNIVS_OK, UNIVS_ERR_NOT_IMPLEMENTED where the sizes are not covered, or the launch's error
int hota_counts(const int* inter, const int* gt_area, const int* tr_area, int D, int G, int T, const int* gt_ids, const int* gt_starts,
                const int* tr_ids, const int* tr_starts, int C, int max_g, int max_p, const double* thr, int A, int* tp_fn_fp, int* matches,
                double* loca_sum, int* gt_id_count, int* tracker_id_count, int* match_col, hipStream_t st);
int lsa_max_f64(const double* score, const int* rows, const int* cols, int B, int* col_of_row, hipStream_t st);

}  // namespace univs
