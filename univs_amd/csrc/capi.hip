// extern "C" entry points of libunivs_hip.so (declared in include/univs_hip.h).
// Argument validation + dispatch only; kernels live in the sibling .hip files (their launchers: launchers.h).
#include <stdarg.h>
#include <string.h>

#include <mutex>

#include "../../include/univs_encoder_hip.h"
#include "../../include/univs_eval_hip.h"
#include "../../include/univs_frames_hip.h"
#include "../../include/univs_fused_hip.h"
#include "../../include/univs_hota_hip.h"
#include "../../include/univs_idmap_hip.h"
#include "../../include/univs_imagelabels_hip.h"
#include "../../include/univs_jpeg_hip.h"
#include "../../include/univs_jpegenc_hip.h"
#include "../../include/univs_png_hip.h"
#include "../../include/univs_polygons_hip.h"
#include "../../include/univs_pngread_hip.h"
#include "../../include/univs_prompts_hip.h"
#include "../../include/univs_pvos_hip.h"
#include "../../include/univs_seam_hip.h"
#include "../../include/univs_semantic_hip.h"
#include "../../include/univs_swin_hip.h"
#include "../../include/univs_text_hip.h"
#include "common.h"
#include "config.h"
#include "launchers.h"
#include "pair_xres_plan.h"

namespace univs {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// "<name>: <text>"
static void report(const char* name, const char* fmt, va_list ap) {
  const int n = snprintf(g_err, sizeof(g_err), "%s: ", name);
  if (n >= 0 && (size_t)n < sizeof(g_err)) vsnprintf(g_err + n, sizeof(g_err) - (size_t)n, fmt, ap);
}

// ... with UNIVS_ERR_INVALID_ARGUMENT, for the settings entries (they launch nothing)
__attribute__((format(printf, 2, 3))) static int invalid_argument(const char* name, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  report(name, fmt, ap);
  va_end(ap);
  return UNIVS_ERR_INVALID_ARGUMENT;
}

// The skeleton of every launching entry.  Made first (it clears the sticky HIP error), it reports under `name` -- an entry that
// extends another reports under that one's name --, holds the stream, and maps the launcher's code to the ABI's: `covered` for the
// launchers that return UNIVS_* codes, `launched` for the 1 / 0 / < 0 ones (launchers.h states which is which).  The checks
// and their order stay with the entry: dimensions, empty shape, NULL pointers, whatever else it has, launch.
struct Entry {
  const char* name;
  hipStream_t st;
  Entry(const char* name_, void* stream) : name(name_), st(static_cast<hipStream_t>(stream)) { clear_sticky_error(); }

  __attribute__((format(printf, 2, 3))) int invalid(const char* fmt, ...) const {
    va_list ap;
    va_start(ap, fmt);
    report(name, fmt, ap);
    va_end(ap);
    return UNIVS_ERR_INVALID_ARGUMENT;
  }
  int null_pointer() const { return invalid("NULL data pointer"); }
  // a launcher's UNIVS_* code; where that is UNIVS_ERR_NOT_IMPLEMENTED, with the text of what is covered
  __attribute__((format(printf, 3, 4))) int covered(int rc, const char* fmt, ...) const {
    if (rc != UNIVS_ERR_NOT_IMPLEMENTED) return rc;
    va_list ap;
    va_start(ap, fmt);
    report(name, fmt, ap);
    va_end(ap);
    return rc;
  }
  // the code of a launcher that returns 1 if it launched, 0 if the shape is not covered (reported with the text), < 0 on error
  __attribute__((format(printf, 3, 4))) int launched(int rc, const char* fmt, ...) const {
    if (rc != 0) return rc > 0 ? UNIVS_OK : rc;
    va_list ap;
    va_start(ap, fmt);
    report(name, fmt, ap);
    va_end(ap);
    return UNIVS_ERR_NOT_IMPLEMENTED;
  }
};

// process-wide settings (include/univs_hip.h: UnivsConfig); a mutex-protected copy, handed out by value
static std::mutex g_cfg_mu;
static UnivsConfig g_cfg = {};
UnivsConfig config() {
  std::lock_guard<std::mutex> lock(g_cfg_mu);
  return g_cfg;
}
static thread_local int g_msda_last = 0;
static thread_local int g_msda_gen = 0;   // generation of the LDS-tiled kernel that ran last (0: none)

static int make_levels(const Entry& e, const int64_t* shapes, const int64_t* starts, int L, int S, LevelTable* lv) {
  if (L < 1 || L > UNIVS_MAX_LEVELS) return e.invalid("num_levels=%d outside [1,%d]", L, UNIVS_MAX_LEVELS);
  if (!shapes || !starts) return e.invalid("spatial_shapes / level_start_index must be host pointers, got NULL");
  // The table must describe the concatenation `value` holds (ms_deform_attn.py:95: the levels are flattened and
  // concatenated in order): start[l] is the running sum of H*W and the levels cover exactly S tokens.  A table that
  // merely fits inside S (e.g. the previous, smaller resolution's) would sample with the wrong geometry silently.
  int64_t run = 0;
  for (int l = 0; l < L; ++l) {
    const int64_t H = shapes[2 * l], W = shapes[2 * l + 1], st = starts[l];
    if (H <= 0 || W <= 0 || st != run || st + H * W > (int64_t)S)
      return e.invalid("level %d (H=%lld, W=%lld, start=%lld) is inconsistent: expected start=%lld, value length S=%d", l, (long long)H,
                       (long long)W, (long long)st, (long long)run, S);
    run += H * W;
    lv->H[l] = (int)H;
    lv->W[l] = (int)W;
    lv->start[l] = (int)st;
  }
  if (run != (int64_t)S) return e.invalid("the %d levels hold %lld tokens but value has S=%d", L, (long long)run, S);
  for (int l = L; l < UNIVS_MAX_LEVELS; ++l) lv->H[l] = lv->W[l] = lv->start[l] = 0;
  return UNIVS_OK;
}

// The Linear entries differ in their name, in their weight pointers (`ptrs_ok`), in what they launch and in the convention of its
// code (`resident`: the 1 / 0 / < 0 of the W-resident launcher): argument validation in one place.
template <class F>
static int linear_entry(const Entry& e, long long M, int N, int K, int act, const float* residual, bool ptrs_ok, bool resident, F&& launch) {
  if (M < 0 || N < 0 || K < 1 || act < 0 || act > 2 || (act != 0 && residual))
    return e.invalid("bad arguments M=%lld N=%d K=%d act=%d%s", M, N, K, act,
                     (act != 0 && residual) ? " (an activation and a residual exclude each other)" : "");
  if (M == 0 || N == 0) return UNIVS_OK;
  if (!ptrs_ok) return e.null_pointer();
  const int rc = launch(residual ? 3 : act);
  return resident ? e.launched(rc, "shape M=%lld N=%d K=%d (or alignment) is not covered", M, N, K)
                  : e.covered(rc, "shape M=%lld N=%d K=%d (or alignment) is not covered", M, N, K);
}
// ... and the two with the column-blocked output
template <class F>
static int linear_blocked_entry(const Entry& e, long long M, int N, int K, int rows_per_batch, int col_block, bool ptrs_ok, F&& launch) {
  if (M < 0 || N < 1 || K < 1 || rows_per_batch < 1 || col_block < 4 || col_block % 4 != 0 || N % col_block != 0 ||
      (M % rows_per_batch) != 0)
    return e.invalid("bad arguments M=%lld N=%d K=%d rows_per_batch=%d col_block=%d", M, N, K, rows_per_batch, col_block);
  if (M == 0) return UNIVS_OK;
  if (!ptrs_ok) return e.null_pointer();
  return e.launched(launch(), "shape M=%lld N=%d K=%d (or alignment) is not covered (K == 256, M >= 2048)", M, N, K);
}
// The convolution entries on the streamed kernel; `covers`: what the entry's kernel takes
template <class F>
static int conv_entry(const Entry& e, const char* covers, int T, int Cin, int Cout, int H, int W, bool ptrs_ok, F&& launch) {
  if (T < 0 || Cin < 1 || Cout < 0 || H < 0 || W < 0) return e.invalid("bad dimensions T=%d Cin=%d Cout=%d H=%d W=%d", T, Cin, Cout, H, W);
  if (T == 0 || Cout == 0 || H == 0 || W == 0) return UNIVS_OK;
  if (!ptrs_ok) return e.null_pointer();
  return e.covered(launch(), "T=%d Cin=%d Cout=%d H=%d W=%d not covered (%s)", T, Cin, Cout, H, W, covers);
}

}  // namespace univs

using namespace univs;

extern "C" {

const char* univs_version(void) { return "univs_hip 0.1.0 gfx950"; }
const char* univs_last_error(void) { return g_err; }

int univs_configure(const UnivsConfig* cfg) {
  UnivsConfig c = {};
  if (cfg) {
    if (cfg->size < (int)(2 * sizeof(int)) || cfg->size > (int)sizeof(UnivsConfig))
      return invalid_argument(__func__, "UnivsConfig.size=%d (this library: %d)", cfg->size, (int)sizeof(UnivsConfig));
    memcpy(&c, cfg, (size_t)cfg->size);   // fields the caller does not know keep their defaults (0)
    if (c.msda_impl < 0 || c.msda_impl > 2 || c.mask_decode_impl < 0 || c.mask_decode_impl > 2 || c.msda_halo > 64 ||
        (c.mask_decode_ct != 0 && c.mask_decode_ct != 2 && c.mask_decode_ct != 4) ||
        (c.linear_terms != 0 && c.linear_terms != 3 && c.linear_terms != 6) || c.mask_decode_wave_tiles > 64)
      return invalid_argument(__func__, "msda_impl=%d mask_decode_impl=%d msda_halo=%d mask_decode_ct=%d linear_terms=%d out of range", c.msda_impl,
                              c.mask_decode_impl, c.msda_halo, c.mask_decode_ct, c.linear_terms);
  }
  c.size = (int)sizeof(UnivsConfig);
  std::lock_guard<std::mutex> lock(g_cfg_mu);
  g_cfg = c;
  return UNIVS_OK;
}

int univs_get_config(UnivsConfig* out) {
  if (!out) return invalid_argument(__func__, "NULL");
  *out = config();
  out->size = (int)sizeof(UnivsConfig);
  return UNIVS_OK;
}

int univs_msda_set_impl(int impl) {
  if (impl < 0 || impl > 2) return invalid_argument(__func__, "impl=%d not in {0,1,2}", impl);
  std::lock_guard<std::mutex> lock(g_cfg_mu);
  g_cfg.msda_impl = impl;
  return UNIVS_OK;
}

int univs_msda_last_impl(void) { return g_msda_last; }
int univs_msda_last_tiled_generation(void) { return g_msda_gen; }

int univs_linear_fused_f32(const float* x, const float* weight, const float* bias, const float* residual, long long M, int N,
                           int K, int act, float* y, void* stream) {
  const Entry e("univs_linear_fused_f32", stream);
  return linear_entry(e, M, N, K, act, residual, x && weight && y, /*resident=*/true,
                      [&](int epi) { return linear_split_f32(x, weight, bias, residual, y, M, N, K, epi, e.st); });
}

int univs_presplit_weights_f32(const float* w, int N, int K, int conv, void* wp, float* winv, void* stream) {
  const Entry e("univs_presplit_weights_f32", stream);
  if (N < 0 || K < 32 || K % 32 != 0 || conv < 0 || conv > 2 || (conv == 1 && K % 9 != 0))
    return e.invalid("bad arguments N=%d K=%d mode=%d (K a multiple of 32; mode 1: K = 9 Cin)", N, K, conv);
  if (N == 0) return UNIVS_OK;
  if (!w || !wp || !winv || (reinterpret_cast<uintptr_t>(wp) & 15)) return e.invalid("NULL or unaligned pointer");
  return presplit_f16x3(w, N, K, conv == 1 ? K / 9 : 0, conv == 2 ? 1 : 0, wp, winv, e.st);
}

int univs_conv1x1_presplit_f32(const float* x, const void* wp, const float* winv, const float* bias, int T, int Cin, int Cout, int H,
                               int W, float* y, void* stream) {
  const Entry e("univs_conv1x1_presplit_f32", stream);
  return conv_entry(e, "Cin % 96 or % 128, Cout % 16, >= 4096 pixels", T, Cin, Cout, H, W, x && wp && winv && y,
                    [&] { return conv1x1_f16x3_f32(x, wp, winv, bias, y, T, Cin, Cout, H, W, e.st); });
}

long long univs_cross_attention_workspace(int L, int S, int N, int H) {
  if (L <= 0 || S <= 0 || N <= 0 || H <= 0) return 0;
  return (long long)cross_attention_workspace_floats(L, S, N, H);
}

int univs_cross_attention_f32(const float* q, const float* k, const float* v, const uint8_t* mask, int L, int S, int N, int H, int head_dim,
                              int ldq, int ldk, int ldv, float scale, float* workspace, float* out, void* stream) {
  return univs_cross_attention_flagged_f32(q, k, v, mask, nullptr, 0u, L, S, N, H, head_dim, ldq, ldk, ldv, scale, workspace, out, stream);
}

int univs_cross_attention_flagged_f32(const float* q, const float* k, const float* v, const uint8_t* mask, const uint32_t* mask_row_flags,
                                      uint32_t mask_generation, int L, int S, int N, int H, int head_dim, int ldq, int ldk, int ldv,
                                      float scale, float* workspace, float* out, void* stream) {
  const Entry e("univs_cross_attention_f32", stream);
  if (L < 0 || S < 1 || N < 0 || H < 1 || head_dim < 1) return e.invalid("bad dimensions L=%d S=%d N=%d H=%d head_dim=%d", L, S, N, H, head_dim);
  if (L == 0 || N == 0) return UNIVS_OK;
  if (!q || !k || !v || !workspace || !out || (mask_row_flags && !mask)) return e.invalid("NULL data pointer (row flags come with a mask)");
  return e.covered(cross_attention_f32(q, k, v, mask, mask_row_flags, mask_generation, L, S, N, H, head_dim, ldq, ldk, ldv, scale, workspace,
                                       out, e.st),
                   "L=%d S=%d N=%d H=%d head_dim=%d not covered (head_dim == 32, S >= 32, with a mask S %% 4 == 0, "
                   "N * H <= 65535, 16-byte aligned pointers)", L, S, N, H, head_dim);
}

int univs_mlp_presplit_f32(const float* x, const void* w1p, const float* w1inv, const float* b1, const void* w2p, const float* w2inv,
                           const float* b2, const float* residual, const float* ln_weight, const float* ln_bias, float ln_eps,
                           const float* post_ln_weight, const float* post_ln_bias, float post_ln_eps, const float* post_add,
                           long long post_add_rows, float* y2, long long M, int C, int Hd, int act, float* y, void* stream) {
  return univs_mlp_presplit_v2_f32(x, w1p, w1inv, b1, w2p, w2inv, b2, residual, 0, ln_weight, ln_bias, ln_eps, post_ln_weight, post_ln_bias,
                                   post_ln_eps, post_add, post_add_rows, y2, M, C, Hd, act, y, stream);
}

int univs_mlp_presplit_v2_f32(const float* x, const void* w1p, const float* w1inv, const float* b1, const void* w2p, const float* w2inv,
                              const float* b2, const float* residual, int flags, const float* ln_weight,
                              const float* ln_bias, float ln_eps, const float* post_ln_weight, const float* post_ln_bias, float post_ln_eps,
                              const float* post_add, long long post_add_rows, float* y2, long long M, int C, int Hd, int act, float* y,
                              void* stream) {
  const Entry e("univs_mlp_presplit_f32", stream);
  if (M < 0 || C < 1 || Hd < 1 || (act != 1 && act != 2)) return e.invalid("bad arguments M=%lld C=%d Hd=%d act=%d (1 ReLU, 2 GELU)", M, C, Hd, act);
  if (M == 0) return UNIVS_OK;
  if (!x || !w1p || !w1inv || !w2p || !w2inv || !y) return e.null_pointer();
  if ((flags & ~3) || ((flags & 1) && (residual || !ln_weight || x == y)) || ((flags & 2) && (!post_ln_weight || !y2 || post_add || (flags & 1))))
    return e.invalid("flags=%d: UNIVS_MLP_RESIDUAL_IS_NORMED_X needs ln_weight, no residual pointer and y distinct from x "
                     "(the normalised rows are parked in y); UNIVS_MLP_DUAL_OUTPUT needs post_ln_weight and y2, no post_add, and excludes the other",
                     flags);
  return e.covered(mlp_f16x3_f32(x, w1p, w1inv, b1, w2p, w2inv, b2, residual, ln_weight, ln_bias, ln_eps, post_ln_weight, post_ln_bias,
                                 post_ln_eps, post_add, post_add_rows, y2, y, M, C, Hd, act, flags, e.st),
                   "shape M=%lld C=%d Hd=%d (or alignment) is not covered (C in 96 / 128 / 192 / 256 / 384, Hd %% 32 == 0, M >= 2048)", M, C, Hd);
}

int univs_small_linear_presplit_f32(const float* x, const float* x_add, const void* wp, const float* winv, const float* bias, int n_w,
                                    int f_off, const float* residual, const float* ln_weight, const float* ln_bias, float ln_eps,
                                    long long M, int N, int K, int relu, int add_features, int out_T, float* y, void* stream) {
  const Entry e("univs_small_linear_presplit_f32", stream);
  if (M < 0 || N < 0 || K < 1 || n_w < 1 || f_off < 0 || f_off + N > n_w)
    return e.invalid("bad arguments M=%lld N=%d K=%d n_w=%d f_off=%d", M, N, K, n_w, f_off);
  if (M == 0 || N == 0) return UNIVS_OK;
  if (!x || !wp || !winv || !y || (ln_bias && !ln_weight)) return e.null_pointer();
  return e.covered(small_linear_f32(x, x_add, wp, winv, bias, n_w, f_off, residual, ln_weight, ln_bias, ln_eps, y, M, N, K, relu, add_features,
                                    out_T, e.st),
                   "M=%lld N=%d K=%d not covered (K %% 32 == 0, N %% 16 == 0, f_off %% 4 == 0, with a LayerNorm "
                   "N == 256, M <= 1 048 560, 16-byte aligned pointers)", M, N, K);
}

int univs_small_mlp_presplit_f32(const float* x, int stages, const void* const* wp, const float* const* winv, const float* const* bias,
                                 const int* relu, const float* in_ln_weight, const float* in_ln_bias, float in_ln_eps, float* x_normed,
                                 long long M, int out_T, float* y, void* stream) {
  const Entry e("univs_small_mlp_presplit_f32", stream);
  if (M < 0 || stages < 1 || stages > 3 || out_T < 0) return e.invalid("bad arguments M=%lld stages=%d out_T=%d", M, stages, out_T);
  if (M == 0) return UNIVS_OK;
  if (!x || !y || !wp || !winv || !bias || !relu) return e.invalid("NULL pointer");
  return e.covered(small_chain_f32(x, stages, wp, winv, bias, relu, in_ln_weight, in_ln_bias, in_ln_eps, x_normed, y, M, out_T, e.st),
                   "M=%lld not covered (M <= 1 048 560, out_T | M, 16-byte aligned pointers, x_normed / bias only with a LayerNorm)", M);
}

int univs_linear_presplit_f32(const float* x, const void* wp, const float* winv, const float* bias, const float* residual,
                              long long M, int N, int K, int act, float* y, void* stream) {
  // the two-dimensional tiling where it applies (gemm_f16x3_tile.hip; UnivsConfig.linear_ablate == LA_NO_TILE switches it off: A / B), else the
  // row-range x pass kernel -- bit-identical results
  const Entry e("univs_linear_presplit_f32", stream);
  return linear_entry(e, M, N, K, act, residual, x && wp && winv && y, /*resident=*/false, [&](int epi) {
    int rc = UNIVS_ERR_NOT_IMPLEMENTED;
    if (config().linear_ablate != LA_NO_TILE) rc = linear_f16x3_tile_f32(x, wp, winv, bias, residual, y, M, N, K, epi, e.st);
    if (rc == UNIVS_ERR_NOT_IMPLEMENTED) rc = linear_f16x3_stream_f32(x, wp, winv, bias, residual, y, M, N, K, epi, e.st);
    return rc;
  });
}

int univs_linear_resident_presplit_f32(const float* x, const void* wp, const float* winv, const float* bias, const float* residual,
                                       long long M, int N, int K, int act, float* y, void* stream) {
  const Entry e("univs_linear_resident_presplit_f32", stream);
  return linear_entry(e, M, N, K, act, residual, x && wp && winv && y, /*resident=*/true, [&](int epi) {
    return linear_split_f32(x, static_cast<const float*>(wp), bias, residual, y, M, N, K, epi, e.st, 0, 0, winv);
  });
}

int univs_linear_blocked_presplit_f32(const float* x, const void* wp, const float* winv, const float* bias, long long M, int N, int K,
                                      int rows_per_batch, int col_block, float* y, void* stream) {
  const Entry e("univs_linear_blocked_presplit_f32", stream);
  return linear_blocked_entry(e, M, N, K, rows_per_batch, col_block, x && wp && winv && y, [&] {
    return linear_split_f32(x, static_cast<const float*>(wp), bias, nullptr, y, M, N, K, /*LS_EPI_BLOCKED=*/4, e.st, rows_per_batch, col_block,
                            winv);
  });
}

int univs_encoder_linear_pair_presplit_f32(const float* x, const float* add, long long add_rows, const void* wp_a, const float* winv_a,
                                           const float* bias_a, int N_a, int col_block_a, float* y_a, const void* wp_b,
                                           const float* winv_b, const float* bias_b, int N_b, int col_block_b, float* y_b, long long M,
                                           int K, long long rows_per_batch, void* stream) {
  const Entry e("univs_encoder_linear_pair_presplit_f32", stream);
  if (M < 1 || N_a < 1 || N_b < 1 || K < 1 || add_rows < 1 || rows_per_batch < 1 || col_block_a < 1 || col_block_b < 1)
    return e.invalid("bad arguments M=%lld K=%d add_rows=%lld rows_per_batch=%lld N_a=%d col_block_a=%d N_b=%d col_block_b=%d", M, K, add_rows,
                     rows_per_batch, N_a, col_block_a, N_b, col_block_b);
  if (!x || !add || !wp_a || !winv_a || !y_a || !wp_b || !winv_b || !y_b) return e.null_pointer();
  // the x-resident kernel where it covers the call (linear_pair_xres.hip; UnivsConfig.linear_ablate == LA_NO_PAIR_XRES switches it off: A / B), else the
  // W-resident pass kernel -- bit-identical results, and the same coverage of the entry as before
  int rc = linear_pair_xres_f32(x, add, add_rows, wp_a, winv_a, bias_a, N_a, col_block_a, y_a, wp_b, winv_b, bias_b, N_b, col_block_b, y_b, M, K,
                                rows_per_batch, e.st);
  if (rc == 0)
    rc = linear_pair_f16x3_f32(x, add, add_rows, wp_a, winv_a, bias_a, N_a, col_block_a, y_a, wp_b, winv_b, bias_b, N_b, col_block_b, y_b, M, K,
                               rows_per_batch, e.st);
  return e.launched(rc,
                    "not covered (K == 256, add_rows == rows_per_batch dividing M, N_a in passes of 113 .. 128 features and N_b of 81 .. 96, "
                    "column blocks of a multiple of 4 dividing N, 16-byte aligned pointers, M max(K, N_a, N_b) 4 < 2^31)");
}

int univs_conv3x3_presplit_f32(const float* x, const void* wp, const float* winv, int T, int Cin, int Cout, int H, int W,
                               float* y, void* stream) {
  const Entry e("univs_conv3x3_presplit_f32", stream);
  return conv_entry(e, "Cin % 128, Cout % 16, >= 4096 pixels", T, Cin, Cout, H, W, x && wp && winv && y,
                    [&] { return conv3x3_f16x3_f32(x, wp, winv, y, T, Cin, Cout, H, W, e.st); });
}

int univs_conv3x3_nhwc_presplit_f32(const float* x, const void* wp, const float* winv, int T, int Cin, int Cout, int H, int W,
                                    float* y, void* stream) {
  const Entry e("univs_conv3x3_nhwc_presplit_f32", stream);
  return conv_entry(e, "Cin % 128, Cout % 16, >= 4096 pixels", T, Cin, Cout, H, W, x && wp && winv && y,
                    [&] { return conv3x3_nhwc_f16x3_f32(x, wp, winv, y, T, Cin, Cout, H, W, e.st); });
}

int univs_conv1x1_fused_presplit_f32(const float* x, int channels_last, const float* affine, const void* wp, const float* winv,
                                     const float* bias, int T, int Cin, int Cout, int H, int W, float* y, void* stream) {
  const Entry e("univs_conv1x1_fused_presplit_f32", stream);
  return conv_entry(e, "Cin % 96 or % 128, Cout % 16, >= 4096 pixels; with an affine H W >= 256 and Cin <= 1024", T, Cin, Cout, H, W,
                    x && wp && winv && y,
                    [&] { return conv1x1_fused_f16x3_f32(x, channels_last, affine, wp, winv, bias, y, T, Cin, Cout, H, W, e.st); });
}

int univs_cross_attention_partials_f32(const float* q, const float* k, const float* v, const uint8_t* mask, const uint32_t* mask_row_flags,
                                       uint32_t mask_generation, int L, int S, int N, int H, int head_dim, int ldq, int ldk, int ldv,
                                       float scale, float* workspace, int* plan, void* stream) {
  const Entry e("univs_cross_attention_partials_f32", stream);
  if (!plan) return e.invalid("NULL plan (a host int)");
  *plan = 0;
  if (L < 0 || S < 1 || N < 0 || H < 1 || head_dim < 1) return e.invalid("bad dimensions L=%d S=%d N=%d H=%d head_dim=%d", L, S, N, H, head_dim);
  if (L == 0 || N == 0) return UNIVS_OK;
  if (!q || !k || !v || !workspace || (mask_row_flags && !mask)) return e.invalid("NULL data pointer (row flags come with a mask)");
  return e.covered(cross_attention_partials_f32(q, k, v, mask, mask_row_flags, mask_generation, L, S, N, H, head_dim, ldq, ldk, ldv, scale,
                                                workspace, plan, e.st),
                   "L=%d S=%d N=%d H=%d head_dim=%d not covered (head_dim == 32, S >= 32, with a mask S %% 4 == 0, "
                   "N * H <= 65535, 16-byte aligned pointers)", L, S, N, H, head_dim);
}

int univs_small_linear_merged_presplit_f32(const float* workspace, long long workspace_floats, int plan, int L, int N, int H, const void* wp,
                                           const float* winv, const float* bias, int n_w, int f_off, const float* residual,
                                           const float* ln_weight, const float* ln_bias, float ln_eps, int n_out, float* y, void* stream) {
  const Entry e("univs_small_linear_merged_presplit_f32", stream);
  const int nseg = plan & 0xffff, nqb = plan >> 16;
  if (L < 0 || N < 0 || H < 1 || n_out < 0 || n_w < 1 || f_off < 0 || f_off + n_out > n_w)
    return e.invalid("bad arguments L=%d N=%d H=%d n_out=%d n_w=%d f_off=%d", L, N, H, n_out, n_w, f_off);
  if (L == 0 || N == 0 || n_out == 0) return UNIVS_OK;
  if (plan <= 0 || nseg < 1 || nqb < 1 || nqb > 7) return e.invalid("plan=%d is not segments + 65536 * query blocks per wave (1 .. 7)", plan);
  const long long chunks = ((long long)L + 16 * nqb - 1) / (16 * nqb);
  const long long need = chunks * N * H * nseg * (16 * nqb) * 34;
  if (workspace_floats < need)
    return e.invalid("workspace of %lld floats, the plan %d of L=%d N=%d H=%d takes %lld", workspace_floats, plan, L, N, H, need);
  if (!workspace || !wp || !winv || !y || (ln_bias && !ln_weight)) return e.null_pointer();
  return e.covered(small_linear_merged_f32(workspace, plan, L, N, H, wp, winv, bias, n_w, f_off, residual, ln_weight, ln_bias, ln_eps, y,
                                           n_out, e.st),
                   "L=%d N=%d H=%d n_out=%d not covered (H <= 8, n_out %% 16 == 0, f_off %% 4 == 0, with a LayerNorm n_out == 256, "
                   "L N <= 1 048 560, 16-byte aligned pointers)", L, N, H, n_out);
}

int univs_patch_embed4_f32(const float* x, const float* weight, const float* bias, const float* ln_weight, const float* ln_bias, float ln_eps,
                           int T, int H, int W, int E, float* out, void* stream) {
  const Entry e("univs_patch_embed4_f32", stream);
  if (T < 0 || H < 0 || W < 0 || E < 1) return e.invalid("bad dimensions T=%d H=%d W=%d E=%d", T, H, W, E);
  if (T == 0 || H == 0 || W == 0) return UNIVS_OK;
  if (!x || !weight || !out) return e.null_pointer();
  return e.covered(patch_embed4_f32(x, weight, bias, ln_weight, ln_bias, ln_eps, out, T, H, W, E, e.st),
                   "T=%d H=%d W=%d E=%d not covered (E in 96 / 128 / 192, H %% 4, W %% 4, 16-byte alignment)", T, H, W, E);
}

int univs_decoder_memory_f32(const float* x, const float* level_embed, const float* pos_yx, const float* pos_t, int T, int C, int HW,
                             float* memory, float* key, void* stream) {
  const Entry e("univs_decoder_memory_f32", stream);
  if (T < 0 || C < 0 || HW < 0) return e.invalid("bad dimensions T=%d C=%d HW=%d", T, C, HW);
  if (T == 0 || C == 0 || HW == 0) return UNIVS_OK;
  if (!x || !level_embed || !pos_yx || !pos_t || !memory || !key) return e.null_pointer();
  return e.covered(decoder_memory_f32(x, level_embed, pos_yx, pos_t, memory, key, T, C, HW, e.st),
                   "T=%d C=%d HW=%d not covered (C %% 4, HW %% 4, 16-byte alignment)", T, C, HW);
}

int univs_transpose_f32(const float* x, long long B, int R, int C, float* out, void* stream) {
  return univs_transpose_strided_f32(x, B, R, C, 0, out, stream);
}

int univs_transpose_strided_f32(const float* x, long long B, int R, int C, long long in_batch_stride, float* out, void* stream) {
  return univs_transpose_ex_f32(x, B, R, C, in_batch_stride, nullptr, out, 0, nullptr, nullptr, stream);
}

int univs_transpose_ex_f32(const float* x, long long B, int R, int C, long long in_batch_stride, const float* row_affine, float* out,
                           long long out_batch_stride, const float* addend, float* out2, void* stream) {
  const Entry e("univs_transpose_f32", stream);
  if (B < 0 || R < 0 || C < 0 || in_batch_stride < 0 || (in_batch_stride != 0 && in_batch_stride < (long long)R * C) ||
      out_batch_stride < 0 || (out_batch_stride != 0 && out_batch_stride < (long long)R * C))
    return e.invalid("bad dimensions B=%lld R=%d C=%d in_batch_stride=%lld out_batch_stride=%lld", B, R, C, in_batch_stride, out_batch_stride);
  if (B == 0 || R == 0 || C == 0) return UNIVS_OK;
  if (!x || !out || (addend != nullptr) != (out2 != nullptr)) return e.invalid("NULL data pointer (addend and out2 come together)");
  return e.covered(transpose_f32(x, out, B, R, C, in_batch_stride, out_batch_stride, row_affine, addend, out2, e.st),
                   "R=%d C=%d B=%lld not covered (R %% 4, C %% 4, strides %% 4, B <= 65535, 16-byte alignment)", R, C, B);
}

int univs_mask_decode_set_impl(int impl) {
  clear_sticky_error();
  if (impl < 0 || impl > 2) return invalid_argument(__func__, "impl=%d not in {0,1,2}", impl);
  {
    std::lock_guard<std::mutex> lock(g_cfg_mu);
    g_cfg.mask_decode_impl = impl;
  }
  return UNIVS_OK;
}

int univs_mask_decode_last_impl(void) { return mask_decode_last_impl(); }

int univs_msda_forward_f32(const float* value, const int64_t* spatial_shapes,
                           const int64_t* level_start, const float* sampling_loc,
                           const float* attn_weight, int N, int S, int M, int D, int L, int Lq,
                           int P, float* out, void* stream) {
  const Entry e("univs_msda_forward_f32", stream);
  if (N < 0 || S < 0 || M < 0 || D < 0 || Lq < 0 || P < 0) return e.invalid("negative dimension");
  if ((long long)N * Lq * M * D == 0) return UNIVS_OK;  // empty output
  if (!value || !sampling_loc || !attn_weight || !out) return e.null_pointer();
  LevelTable lv;
  int rc = make_levels(e, spatial_shapes, level_start, L, S, &lv);
  if (rc != UNIVS_OK) return rc;
  g_msda_gen = 0;
  if (config().msda_impl != 1) {
    // the LDS-tiled kernel for the encoder geometry on the standard layouts (msda_tiled2.hip: D == 32, P == 4, 3 <= L <= 4,
    // Lq == S); returns 0 when its preconditions fail.  (The module path uses univs_msda_forward_strips_f32.)
    rc = msda_forward_tiled2_f32(value, lv, sampling_loc, attn_weight, N, S, M, D, L, Lq, P, out, e.st);
    if (rc > 0) g_msda_last = g_msda_gen = 2;
    if (rc != 0) return rc < 0 ? rc : UNIVS_OK;
  }
  g_msda_last = 1;
  return msda_forward_generic_f32(value, lv, sampling_loc, attn_weight, N, S, M, D, L, Lq, P, out, e.st);
}

int univs_msda_forward_f64(const double* value, const int64_t* spatial_shapes,
                           const int64_t* level_start, const double* sampling_loc,
                           const double* attn_weight, int N, int S, int M, int D, int L, int Lq,
                           int P, double* out, void* stream) {
  const Entry e("univs_msda_forward_f64", stream);
  if (N < 0 || S < 0 || M < 0 || D < 0 || Lq < 0 || P < 0) return e.invalid("negative dimension");
  if ((long long)N * Lq * M * D == 0) return UNIVS_OK;
  if (!value || !sampling_loc || !attn_weight || !out) return e.null_pointer();
  LevelTable lv;
  const int rc = make_levels(e, spatial_shapes, level_start, L, S, &lv);
  if (rc != UNIVS_OK) return rc;
  return msda_forward_generic_f64(value, lv, sampling_loc, attn_weight, N, S, M, D, L, Lq, P, out, e.st);
}

int univs_msda_backward_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start,
                            const float* sampling_loc, const float* attn_weight, const float* grad_output, int N,
                            int S, int M, int D, int L, int Lq, int P, float* grad_value,
                            float* grad_sampling_loc, float* grad_attn_weight, void* stream) {
  const Entry e("univs_msda_backward_f32", stream);
  if (N < 0 || S < 0 || M < 0 || D < 0 || Lq < 0 || P < 0 || L < 0) return e.invalid("negative dimension");
  if ((long long)N * S * M * D > 0 && !grad_value) return e.invalid("NULL grad_value");
  const long long nsamp = (long long)N * Lq * M * L * P;
  if (nsamp > 0 && (!value || !sampling_loc || !attn_weight || !grad_output || !grad_sampling_loc || !grad_attn_weight))
    return e.null_pointer();
  LevelTable lv;
  const int rc = make_levels(e, spatial_shapes, level_start, L, S, &lv);
  if (rc != UNIVS_OK) return rc;
  if ((long long)N * S * M * D == 0) return UNIVS_OK;
  return msda_backward_f32(value, lv, sampling_loc, attn_weight, grad_output, N, S, M, D, L, Lq, P, grad_value, grad_sampling_loc,
                           grad_attn_weight, e.st);
}

int univs_mask_decode_f32(const float* mask_embed, const float* mask_features, int T, int Q, int C,
                          int HW, float* out, void* stream) {
  const Entry e("univs_mask_decode_f32", stream);
  if (T < 0 || Q < 0 || C <= 0 || HW < 0) return e.invalid("bad dimensions T=%d Q=%d C=%d HW=%d", T, Q, C, HW);
  if ((long long)T * Q * HW == 0) return UNIVS_OK;
  if (!mask_embed || !mask_features || !out) return e.null_pointer();
  return mask_decode_f32(mask_embed, mask_features, T, Q, C, HW, out, e.st);
}

int univs_mask_decode_attn_f32(const float* mask_embed, const float* feat_lowres, int T, int Q,
                               int C, int hw, uint8_t* attn_mask, uint32_t* row_any_ws,
                               void* stream) {
  const Entry e("univs_mask_decode_attn_f32", stream);
  if (T < 0 || Q < 0 || C <= 0 || hw < 0) return e.invalid("bad dimensions T=%d Q=%d C=%d hw=%d", T, Q, C, hw);
  if ((long long)T * Q * hw == 0) return UNIVS_OK;
  if (!mask_embed || !feat_lowres || !attn_mask || !row_any_ws) return e.null_pointer();
  return mask_decode_attn_f32(mask_embed, feat_lowres, T, Q, C, hw, attn_mask, row_any_ws, 0u, e.st);
}

int univs_mask_decode_attn_deferred_f32(const float* mask_embed, const float* feat_lowres, int T, int Q, int C, int hw, uint8_t* attn_mask,
                                        uint32_t* row_flags, uint32_t generation, void* stream) {
  const Entry e("univs_mask_decode_attn_deferred_f32", stream);
  if (T < 0 || Q < 0 || C <= 0 || hw < 0 || generation == 0)
    return e.invalid("bad arguments T=%d Q=%d C=%d hw=%d generation=%u (non-zero)", T, Q, C, hw, generation);
  if ((long long)T * Q * hw == 0) return UNIVS_OK;
  if (!mask_embed || !feat_lowres || !attn_mask || !row_flags) return e.null_pointer();
  return mask_decode_attn_f32(mask_embed, feat_lowres, T, Q, C, hw, attn_mask, row_flags, generation, e.st);
}

int univs_attn_mask_rows_reset(uint8_t* attn_mask, const uint32_t* row_flags, uint32_t generation, long long rows, long long hw,
                               void* stream) {
  const Entry e("univs_attn_mask_rows_reset", stream);
  if (rows < 0 || hw < 0 || rows > 0x7fffffffLL) return e.invalid("bad dimensions rows=%lld hw=%lld", rows, hw);
  if (rows * hw == 0) return UNIVS_OK;
  if (!attn_mask || !row_flags) return e.null_pointer();
  return attn_mask_rows_reset(attn_mask, row_flags, generation, rows, hw, e.st);
}

int univs_window_attention_f32(const float* qkv, const float* bias, const float* shift_mask,
                               int B_, int nW, int Ntok, int nH, int hd, float scale, float* out,
                               void* stream) {
  const Entry e("univs_window_attention_f32", stream);
  if (B_ < 0 || Ntok <= 0 || nH <= 0 || hd <= 0 || (shift_mask && (nW <= 0 || B_ % nW != 0)))
    return e.invalid("bad dimensions B_=%d nW=%d Ntok=%d nH=%d hd=%d", B_, nW, Ntok, nH, hd);
  if (B_ == 0) return UNIVS_OK;
  if (!qkv || !bias || !out) return e.null_pointer();
  return window_attention_f32(qkv, bias, shift_mask, B_, nW > 0 ? nW : 1, Ntok, nH, hd, scale, out, e.st);
}

int univs_bilinear_resample_f32(const float* in, const float* addend, float* out, long long planes, int Hin,
                                int Win, int Hout, int Wout, void* stream) {
  const Entry e("univs_bilinear_resample_f32", stream);
  if (planes < 0 || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1)
    return e.invalid("bad dimensions planes=%lld in=%dx%d out=%dx%d", planes, Hin, Win, Hout, Wout);
  if (planes == 0) return UNIVS_OK;
  if (!in || !out) return e.null_pointer();
  return bilinear_resample_f32(in, addend, out, planes, Hin, Win, Hout, Wout, e.st);
}

int univs_normalize_pad_f32(const float* x, const float* mean, const float* std, long long T, int C, int H, int W, int Hp, int Wp, float* out,
                            void* stream) {
  const Entry e("univs_normalize_pad_f32", stream);
  if (T < 0 || C < 1 || H < 1 || W < 1 || Hp < H || Wp < W) return e.invalid("bad dimensions T=%lld C=%d %dx%d -> %dx%d", T, C, H, W, Hp, Wp);
  if (T == 0) return UNIVS_OK;
  if (!x || !mean || !std || !out) return e.null_pointer();
  return e.covered(normalize_pad_f32(x, out, T, C, H, W, Hp, Wp, mean, std, e.st), "T * C = %lld planes not covered (<= 65535)", T * C);
}

int univs_bilinear_crop_nearest_f32(const float* in, int T, int C, int h, int w, int Hp, int Wp, int Hi, int Wi, int hc, int wc, int t_first,
                                    int t_step, int K, float* out, void* stream) {
  const Entry e("univs_bilinear_crop_nearest_f32", stream);
  if (T < 1 || C < 1 || h < 1 || w < 1 || Hp < 1 || Wp < 1 || Hi < 1 || Wi < 1 || hc < 1 || wc < 1 || Hi > Hp || Wi > Wp)
    return e.invalid("bad geometry in [%d, %d, %d, %d] padded %dx%d crop %dx%d out %dx%d", T, C, h, w, Hp, Wp, Hi, Wi, hc, wc);
  if (t_first < 0 || t_step < 1) return e.invalid("t_first=%d t_step=%d (t_first >= 0, t_step >= 1)", t_first, t_step);
  if (K <= 0) return UNIVS_OK;
  if ((long long)t_first + (long long)(K - 1) * t_step >= T)
    return e.invalid("frames %d + k * %d, k < %d, leave the %d frames of the input", t_first, t_step, K, T);
  if (!in || !out) return e.null_pointer();
  return e.covered(bilinear_crop_nearest_f32(in, out, C, h, w, Hp, Wp, Hi, Wi, hc, wc, t_first, t_step, K, e.st),
                   "not covered (h w < 2^31, hc wc < 2^31)");
}

int univs_upsample2x_add_f32(const float* in, const float* addend, const float* addend_affine, float* out, long long planes, int Hin,
                             int Win, void* stream) {
  const Entry e("univs_upsample2x_add_f32", stream);
  if (planes < 0 || Hin < 1 || Win < 1) return e.invalid("bad dimensions planes=%lld in=%dx%d", planes, Hin, Win);
  if (planes == 0) return UNIVS_OK;
  if (!in || !addend || !out) return e.null_pointer();
  return e.covered(upsample2x_add_f32(in, addend, addend_affine, out, planes, Hin, Win, e.st),
                   "%dx%d not covered (Win even; in 8-byte, addend / out 16-byte aligned)", Hin, Win);
}

int univs_group_norm_affine_f32(const float* x, const float* gamma, const float* beta, int N, int C, long long HW, int groups, float eps,
                                float* ws, long long ws_floats, float* affine, void* stream) {
  const Entry e("univs_group_norm_affine_f32", stream);
  if (N < 0 || C < 1 || HW < 0 || groups < 1 || C % groups != 0 || (long long)N * C > 0x7fffffffLL)
    return e.invalid("bad dimensions N=%d C=%d HW=%lld groups=%d", N, C, HW, groups);
  if ((long long)N * HW == 0) return UNIVS_OK;
  if (!x || !gamma || !beta || !ws || !affine) return e.null_pointer();
  return group_norm_affine_f32(x, gamma, beta, N, C, HW, groups, eps, ws, ws_floats, affine, e.st);
}

int univs_bilinear_pyramid3_f32(const float* in, long long planes, int H, int W, float* out2, float* out4, float* out8,
                                void* stream) {
  const Entry e("univs_bilinear_pyramid3_f32", stream);
  if (planes < 0 || H < 8 || W < 8) return e.invalid("bad dimensions planes=%lld in=%dx%d", planes, H, W);
  if (planes == 0) return UNIVS_OK;
  if (!in || !out2 || !out4 || !out8) return e.null_pointer();
  return e.covered(bilinear_pyramid3_f32(in, out2, out4, out8, planes, H, W, e.st), "%dx%d is not a multiple of 8 (or unaligned pointers)", H, W);
}

int univs_layer_norm_add_f32(const float* x, const float* residual, const float* gamma, const float* beta, const float* addend,
                             long long addend_rows, long long rows, int C, float eps, float* sum_out, float* out, float* out2,
                             void* stream) {
  const Entry e("univs_layer_norm_f32", stream);
  if (rows < 0 || C < 1) return e.invalid("bad dimensions rows=%lld C=%d", rows, C);
  if (rows == 0) return UNIVS_OK;
  if (!x || !gamma || !beta || !out || (sum_out && !residual) || ((addend != nullptr) != (out2 != nullptr)) ||
      (addend && (!residual || sum_out || addend_rows < 1 || rows % addend_rows != 0)))
    return e.invalid("NULL data pointer (sum_out needs a residual; addend / out2 come together, with a residual, "
                     "without sum_out; rows must be a multiple of addend_rows)");
  return e.covered(layer_norm_f32(x, residual, gamma, beta, rows, C, eps, sum_out, out, addend, out2, addend ? addend_rows : 1, e.st),
                   "C=%d not supported (C %% 4 == 0, C <= 3072)", C);
}

int univs_layer_norm_f32(const float* x, const float* residual, const float* gamma, const float* beta,
                         long long rows, int C, float eps, float* sum_out, float* out, void* stream) {
  return univs_layer_norm_add_f32(x, residual, gamma, beta, nullptr, 1, rows, C, eps, sum_out, out, nullptr, stream);
}

int univs_patch_merge_norm_f32(const float* x, const float* gamma, const float* beta, int B, int H, int W, int C, float eps, float* out,
                               void* stream) {
  const Entry e("univs_patch_merge_norm_f32", stream);
  if (B < 0 || H < 0 || W < 0 || C < 1) return e.invalid("bad dimensions B=%d H=%d W=%d C=%d", B, H, W, C);
  if ((long long)B * H * W == 0) return UNIVS_OK;
  if (!x || !gamma || !beta || !out || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta) |
                                        reinterpret_cast<uintptr_t>(out)) & 15))
    return e.invalid("NULL or misaligned data pointer (16 bytes)");
  return e.covered(patch_merge_norm_f32(x, gamma, beta, B, H, W, C, eps, out, e.st), "C=%d not supported (C %% 4 == 0, C <= 768)", C);
}

int univs_group_norm_f32(const float* x, const float* gamma, const float* beta, int N, int C, long long HW,
                         int groups, float eps, int relu, float* ws, long long ws_floats, float* out, void* stream) {
  const Entry e("univs_group_norm_f32", stream);
  if (N < 0 || C < 1 || HW < 0 || groups < 1 || C % groups != 0 || (long long)N * C > 0x7fffffffLL)
    return e.invalid("bad dimensions N=%d C=%d HW=%lld groups=%d", N, C, HW, groups);
  if ((long long)N * HW == 0) return UNIVS_OK;
  if (!x || !gamma || !beta || !ws || !out) return e.null_pointer();
  return group_norm_f32(x, gamma, beta, N, C, HW, groups, eps, relu, ws, ws_floats, out, e.st);
}

int univs_masked_softmax_f32(float* scores, const uint8_t* mask, int N, int h, int L, int S, void* stream) {
  const Entry e("univs_masked_softmax_f32", stream);
  if (N < 0 || h < 0 || L < 0 || S < 0) return e.invalid("negative dimension");
  if ((long long)N * h * L * S == 0) return UNIVS_OK;
  if (!scores) return e.invalid("NULL scores");
  return masked_softmax_f32(scores, mask, N, h, L, S, e.st);
}

int univs_proca_attention_f32(const float* qkv0, const float* kd, const float* vd, int Qp, int L, int T, int heads, int head_dim,
                              float scale, float* out, void* stream) {
  const Entry e("univs_proca_attention_f32", stream);
  if (Qp < 0 || L < 0 || T < 0 || heads < 1 || head_dim < 1)
    return e.invalid("bad dimensions Qp=%d L=%d T=%d heads=%d head_dim=%d", Qp, L, T, heads, head_dim);
  if ((long long)Qp * T == 0) return UNIVS_OK;
  if (!qkv0 || !out || (L > 0 && (!kd || !vd))) return e.null_pointer();
  return e.launched(proca_attention_f32(qkv0, kd, vd, Qp, L, T, heads, head_dim, scale, out, e.st),
                    "shape not covered (head_dim == 32, 1 + L <= 16384)");
}

int univs_prompt_prefix_f32(const float* masks, const float* boxes, int F, int n, int h, int w, int scale, float mask_thresh,
                            float* feat_masks, uint32_t* stats, uint8_t* sel, int32_t* rowcnt, uint8_t* fmb, int32_t* counts,
                            uint8_t* valid, uint8_t* visible, void* stream) {
  const Entry e("univs_prompt_prefix_f32", stream);
  if (F < 0 || n < 0 || h < 1 || w < 1 || scale < 1 || h % scale || w % scale || (long long)F * n > 65535)
    return e.invalid("bad dimensions F=%d n=%d h=%d w=%d scale=%d", F, n, h, w, scale);
  if ((long long)F * n == 0) return UNIVS_OK;
  if (!masks || !boxes || !feat_masks || !stats || !sel || !rowcnt || !fmb || !counts || !valid || !visible) return e.null_pointer();
  return prompt_prefix_f32(masks, boxes, F, n, h, w, scale, mask_thresh, feat_masks, stats, sel, rowcnt, fmb, counts, valid, visible, e.st);
}

int univs_prompt_draw(const uint8_t* sel, const int32_t* rowcnt, const uint8_t* fmb, const int32_t* counts, const float* u,
                      const float* keys, const int64_t* tab, int F, int n, int h, int w, int HW, int R, int64_t* point_idx,
                      int64_t* dense_idx, uint8_t* empty, float* point_coords, void* stream) {
  const Entry e("univs_prompt_draw", stream);
  if (F < 0 || n < 0 || h < 1 || w < 1 || HW < 1 || R < 1 || (long long)F * n > 65535)
    return e.invalid("bad dimensions F=%d n=%d h=%d w=%d HW=%d R=%d", F, n, h, w, HW, R);
  if ((long long)F * n == 0) return UNIVS_OK;
  if (!sel || !rowcnt || !fmb || !counts || !point_idx || !dense_idx || !empty || !point_coords) return e.null_pointer();
  if ((tab != nullptr) == (u != nullptr || keys != nullptr) || (!tab && (!u || !keys))) return e.invalid("either (u, keys) or tab");
  return e.launched(prompt_draw(sel, rowcnt, fmb, counts, u, keys, reinterpret_cast<const long long*>(tab), F, n, h, w, HW, R,
                                reinterpret_cast<long long*>(point_idx), reinterpret_cast<long long*>(dense_idx), empty, point_coords, e.st),
                    "the keys of one entity do not fit the LDS (HW = %d)", HW);
}

int univs_prompt_tokens_f32(const float* feats, const int64_t* feats_strides, const float* pos, const int64_t* pos_strides,
                            const float* qfeat, const float* qpe, const int64_t* dense_idx, const uint8_t* empty, const uint8_t* valid,
                            const float* boxes, const int64_t* kf, int F, int n, int R, int T, int C, int h_img, int w_img, float* fd,
                            float* pd, uint8_t* attn, void* stream) {
  const Entry e("univs_prompt_tokens_f32", stream);
  if (F < 0 || n < 0 || R < 1 || T < 1 || C < 1 || h_img < 1 || w_img < 1 || (long long)F * T * n > 65535)
    return e.invalid("bad dimensions F=%d n=%d R=%d T=%d C=%d h_img=%d w_img=%d", F, n, R, T, C, h_img, w_img);
  if ((long long)F * n == 0) return UNIVS_OK;
  if (!feats || !feats_strides || !pos || !pos_strides || !qfeat || !qpe || !dense_idx || !empty || !valid || !boxes || !kf || !fd || !pd ||
      !attn)
    return e.null_pointer();
  return prompt_tokens_f32(feats, reinterpret_cast<const long long*>(feats_strides), pos, reinterpret_cast<const long long*>(pos_strides),
                           qfeat, qpe, reinterpret_cast<const long long*>(dense_idx), empty, valid, boxes,
                           reinterpret_cast<const long long*>(kf), F, n, R, T, C, h_img, w_img, fd, pd, attn, e.st);
}

int univs_prompt_point_pe_f32(const float* xy, const float* z, const float* dim_t, const float* dim_tz, float scale, int F, int n, int Fq,
                              float* out, void* stream) {
  const Entry e("univs_prompt_point_pe_f32", stream);
  if (F < 0 || n < 0 || Fq < 1) return e.invalid("bad dimensions F=%d n=%d Fq=%d", F, n, Fq);
  if ((long long)F * n == 0) return UNIVS_OK;
  if (!xy || !z || !dim_t || !dim_tz || !out) return e.null_pointer();
  return prompt_point_pe_f32(xy, z, dim_t, dim_tz, scale, F, n, Fq, out, e.st);
}

int univs_mask_stats_strided_f32(const float* x, long long outer, int inner, long long stride_outer, long long stride_inner, int H, int W,
                                 int h_valid, int w_valid, float t_hi, float t_lo, float t_box, int32_t* out, void* stream) {
  const Entry e("univs_mask_stats_f32", stream);
  if (outer < 0 || inner < 1 || H < 1 || W < 1 || h_valid < 0 || w_valid < 0 || h_valid > H || w_valid > W || stride_outer < 0 ||
      stride_inner < (long long)H * W)
    return e.invalid("bad dimensions outer=%lld inner=%d H=%d W=%d h_valid=%d w_valid=%d strides %lld / %lld", outer, inner, H, W, h_valid,
                     w_valid, stride_outer, stride_inner);
  if (outer == 0) return UNIVS_OK;
  if (!x || !out) return e.null_pointer();
  return e.covered(mask_stats_f32(x, outer * inner, inner, stride_outer, stride_inner, H, W, h_valid, w_valid, t_hi, t_lo, t_box, out, e.st),
                   "planes=%lld not covered (<= 65535)", outer * inner);
}

int univs_mask_stats_f32(const float* x, long long planes, int H, int W, int h_valid, int w_valid, float t_hi, float t_lo, float t_box,
                         int32_t* out, void* stream) {
  if (planes > 0x7fffffffLL)
    return Entry("univs_mask_stats_f32", stream).covered(UNIVS_ERR_NOT_IMPLEMENTED, "planes=%lld not covered (<= 65535)", planes);
  return univs_mask_stats_strided_f32(x, planes > 0 ? 1 : 0, (int)std::max<long long>(planes, 1), 0, (long long)H * W, H, W, h_valid, w_valid, t_hi,
                                      t_lo, t_box, out, stream);
}

int univs_token_mean_f32(const float* x, const float* add, int n, int L, int T, int C, float* out, void* stream) {
  const Entry e("univs_token_mean_f32", stream);
  if (n < 0 || L < 0 || T < 0 || C < 1) return e.invalid("bad dimensions n=%d L=%d T=%d C=%d", n, L, T, C);
  if ((long long)n * T == 0) return UNIVS_OK;
  if (!x || !out) return e.null_pointer();
  return e.launched(token_mean_f32(x, add, n, L, T, C, out, e.st), "shape not covered (C <= 1024, L <= 15360)");
}

// ---- per-image post-processing (csrc/image_post.hip) ----
// the geometry every entry shares: L [Q, h, w] resized to (Hp, Wp), crop [0, hi) x [0, wi); a (Hp, Wp) below (h, w) is a
// down-sampling, which the reference never asks for -- it is accepted all the same (the taps stay inside L)
static bool image_geometry_ok(const Entry& e, int Q, int h, int w, int Hp, int Wp, int hi, int wi) {
  if (Q < 1 || h < 1 || w < 1 || Hp < 1 || Wp < 1 || hi < 1 || wi < 1 || hi > Hp || wi > Wp || (long long)Hp * Wp > INT32_MAX ||
      (long long)Q * h * w > (1LL << 40)) {
    e.invalid("bad geometry Q=%d low-res %dx%d padded %dx%d crop %dx%d", Q, h, w, Hp, Wp, hi, wi);
    return false;
  }
  return true;
}

int univs_image_mask_stats_f32(const float* logits, int Q, int h, int w, int Hp, int Wp, int hi, int wi, int32_t* out, void* stream) {
  const Entry e("univs_image_mask_stats_f32", stream);
  if (!image_geometry_ok(e, Q, h, w, Hp, Wp, hi, wi)) return UNIVS_ERR_INVALID_ARGUMENT;
  if (!logits || !out) return e.null_pointer();
  return e.covered(image_mask_stats_f32(logits, Q, h, w, Hp, Wp, hi, wi, out, e.st), "not covered (Q <= 65535)");
}

int univs_image_panoptic_ids_f32(const float* logits, int Q, int h, int w, int Hp, int Wp, int hi, int wi, const int32_t* planes,
                                 const float* scores, int K, int32_t* ids, int32_t* counts, void* stream) {
  const Entry e("univs_image_panoptic_ids_f32", stream);
  if (K < 1) return e.invalid("K=%d", K);
  if (!image_geometry_ok(e, Q, h, w, Hp, Wp, hi, wi)) return UNIVS_ERR_INVALID_ARGUMENT;
  if (!logits || !planes || !scores || !ids || !counts) return e.null_pointer();
  return e.covered(image_panoptic_ids_f32(logits, Q, h, w, Hp, Wp, hi, wi, planes, scores, K, ids, counts, e.st), "not covered (K <= UNIVS_IMAGE_MAX_KEPT)");
}

int univs_image_panoptic_paint_i32(const int32_t* ids, int hi, int wi, const int32_t* lut, int K, int H0, int W0, int32_t* out, int32_t* seen,
                                   void* stream) {
  const Entry e("univs_image_panoptic_paint_i32", stream);
  if (hi < 1 || wi < 1 || K < 1 || H0 < 1 || W0 < 1 || (long long)hi * wi > INT32_MAX || (long long)H0 * W0 > INT32_MAX)
    return e.invalid("bad dimensions ids %dx%d K=%d out %dx%d", hi, wi, K, H0, W0);
  if (!ids || !lut || !out || !seen) return e.null_pointer();
  return e.covered(image_panoptic_paint_i32(ids, hi, wi, lut, K, H0, W0, out, seen, e.st), "not covered (K <= UNIVS_IMAGE_MAX_KEPT)");
}

int univs_image_semseg_f32(const float* logits, int Q, int h, int w, int Hp, int Wp, int hi, int wi, const int32_t* planes,
                           const float* probs, int Qs, int C, float* out, void* stream) {
  const Entry e("univs_image_semseg_f32", stream);
  if (Qs < 0 || C < 1) return e.invalid("Qs=%d C=%d", Qs, C);
  if (!image_geometry_ok(e, Q, h, w, Hp, Wp, hi, wi)) return UNIVS_ERR_INVALID_ARGUMENT;
  if (!logits || !out || (Qs > 0 && (!planes || !probs))) return e.null_pointer();
  return e.covered(image_semseg_f32(logits, Q, h, w, Hp, Wp, hi, wi, planes, probs, Qs, C, out, e.st), "not covered (C <= 65535 * 160)");
}

int univs_image_instance_masks_u8(const float* logits, int Q, int h, int w, int Hp, int Wp, int hi, int wi, const int32_t* planes, int N,
                                  int H0, int W0, uint8_t* masks, int32_t* boxes, void* stream) {
  const Entry e("univs_image_instance_masks_u8", stream);
  if (!image_geometry_ok(e, Q, h, w, Hp, Wp, hi, wi) || N < 0 || H0 < 1 || W0 < 1 || (long long)H0 * W0 > INT32_MAX)
    return e.invalid("bad dimensions N=%d out %dx%d", N, H0, W0);
  if (N == 0) return UNIVS_OK;
  if (!logits || !planes || !masks || !boxes) return e.null_pointer();
  return e.covered(image_instance_masks_u8(logits, Q, h, w, Hp, Wp, hi, wi, planes, N, H0, W0, masks, boxes, e.st), "not covered (N <= 65535)");
}

// ---- video post-processing of the MinVIS-style clip loop (csrc/video_post.hip) ----
static bool video_geometry_ok(const Entry& e, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi) {
  if (V < 1 || !image_geometry_ok(e, Q, h, w, Hp, Wp, hi, wi) || (long long)Q * V * h * w > (1LL << 40) ||
      (long long)V * hi * wi > INT32_MAX) {
    e.invalid("bad geometry Q=%d V=%d low-res %dx%d padded %dx%d crop %dx%d", Q, V, h, w, Hp, Wp, hi, wi);
    return false;
  }
  return true;
}

int univs_minvis_accumulate_f32(float* S, int Q, int V, int h, int w, const float* M, int Qm, int T, const int32_t* perm, int i,
                                void* stream) {
  const Entry e("univs_minvis_accumulate_f32", stream);
  if (Q < 0 || V < 1 || h < 1 || w < 1 || Qm < 1 || T < 1 || i < 0 || i >= V || (long long)Q * V * h * w > (1LL << 40) ||
      (long long)Qm * T * h * w > (1LL << 40))
    return e.invalid("bad dimensions Q=%d V=%d %dx%d Qm=%d T=%d i=%d", Q, V, h, w, Qm, T, i);
  if (Q == 0) return UNIVS_OK;
  if (!S || !M || !perm) return e.null_pointer();
  return minvis_accumulate_f32(S, Q, V, h, w, M, Qm, T, perm, i, e.st);
}

int univs_video_mask_stats_f32(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int32_t* rows, int K,
                               int step, int32_t* counts, void* stream) {
  const Entry e("univs_video_mask_stats_f32", stream);
  if (K < 0 || step < 1) return e.invalid("K=%d step=%d", K, step);
  if (!video_geometry_ok(e, Q, V, h, w, Hp, Wp, hi, wi)) return UNIVS_ERR_INVALID_ARGUMENT;
  if (K == 0) return UNIVS_OK;
  if (!M || !rows || !counts) return e.null_pointer();
  return e.covered(video_mask_stats_f32(M, Q, V, h, w, Hp, Wp, hi, wi, rows, K, step, counts, e.st), "not covered (K <= 65535, sampled frames x crop < 2^31)");
}

int univs_video_instance_masks_u8(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int32_t* rows, int N,
                                  int H0, int W0, uint8_t* masks, void* stream) {
  const Entry e("univs_video_instance_masks_u8", stream);
  if (!video_geometry_ok(e, Q, V, h, w, Hp, Wp, hi, wi) || N < 0 || H0 < 1 || W0 < 1 || (long long)H0 * W0 > INT32_MAX)
    return e.invalid("bad dimensions N=%d out %dx%d", N, H0, W0);
  if (N == 0) return UNIVS_OK;
  if (!M || !rows || !masks) return e.null_pointer();
  return e.covered(video_instance_masks_u8(M, Q, V, h, w, Hp, Wp, hi, wi, rows, N, H0, W0, masks, e.st), "not covered (N V <= 65535)");
}

int univs_video_panoptic_ids_i32(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int32_t* rows,
                                 const float* scores, int K, int32_t* ids, void* stream) {
  const Entry e("univs_video_panoptic_ids_i32", stream);
  if (K < 1) return e.invalid("K=%d", K);
  if (!video_geometry_ok(e, Q, V, h, w, Hp, Wp, hi, wi)) return UNIVS_ERR_INVALID_ARGUMENT;
  if (!M || !rows || !scores || !ids) return e.null_pointer();
  return video_panoptic_ids_i32(M, Q, V, h, w, Hp, Wp, hi, wi, rows, scores, K, ids, e.st);
}

int univs_video_panoptic_counts_i32(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int32_t* rows, int K,
                                    const int32_t* ids, int H0, int W0, int32_t* counts, void* stream) {
  const Entry e("univs_video_panoptic_counts_i32", stream);
  if (!video_geometry_ok(e, Q, V, h, w, Hp, Wp, hi, wi) || K < 1 || H0 < 1 || W0 < 1)
    return e.invalid("bad dimensions K=%d out %dx%d", K, H0, W0);
  if (!M || !rows || !ids || !counts) return e.null_pointer();
  return e.covered(video_panoptic_counts_i32(M, Q, V, h, w, Hp, Wp, hi, wi, rows, K, ids, H0, W0, counts, e.st), "not covered (K <= UNIVS_IMAGE_MAX_KEPT, V H0 W0 < 2^31)");
}

int univs_video_panoptic_paint_i32(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int32_t* rows, int K,
                                   const int32_t* ids, const int32_t* lut, int H0, int W0, int32_t* out, void* stream) {
  const Entry e("univs_video_panoptic_paint_i32", stream);
  if (!video_geometry_ok(e, Q, V, h, w, Hp, Wp, hi, wi) || K < 1 || H0 < 1 || W0 < 1 || (long long)V * H0 * W0 > (1LL << 40))
    return e.invalid("bad dimensions K=%d out %dx%d", K, H0, W0);
  if (!M || !rows || !ids || !lut || !out) return e.null_pointer();
  return video_panoptic_paint_i32(M, Q, V, h, w, Hp, Wp, hi, wi, rows, K, ids, lut, H0, W0, out, e.st);
}

int univs_panoptic_pair_counts(const void* gt, int gt_rgb, const void* pred, int pred_rgb, int T, int H, int W, const int32_t* gt_ids, int G,
                               const int32_t* pred_ids, int P, int32_t* counts, int32_t* first_unknown, void* stream) {
  const Entry e("univs_panoptic_pair_counts", stream);
  if (T < 1 || H < 1 || W < 1 || G < 1 || P < 1 || (long long)T * H * W > (1LL << 40))
    return e.invalid("bad dimensions T=%d H=%d W=%d G=%d P=%d", T, H, W, G, P);
  if (!gt || !pred || !gt_ids || !pred_ids || !counts || !first_unknown) return e.null_pointer();
  return e.covered(panoptic_pair_counts(gt, gt_rgb, pred, pred_rgb, T, H, W, gt_ids, G, pred_ids, P, counts, first_unknown, e.st),
                   "not covered (G, P <= 1024, (G + 1)(P + 1) <= 16384, T <= 65535, H W < 2^31, dword-aligned maps)");
}

int univs_vss_video_counts(const uint8_t* gt, const uint8_t* pred, int T, int H, int W, int num_classes, int32_t* confusion,
                           int32_t* windows, int32_t* overflow, void* stream) {
  const Entry e("univs_vss_video_counts", stream);
  if (T < 1 || H < 1 || W < 1 || num_classes < 1)      // (any size beyond the kernel's is "not covered", not an error)
    return e.invalid("bad dimensions T=%d H=%d W=%d num_classes=%d", T, H, W, num_classes);
  if (!gt || !pred || !confusion || !windows || !overflow) return e.null_pointer();
  return e.covered(vss_video_counts(gt, pred, T, H, W, num_classes, confusion, windows, overflow, e.st), "not covered (num_classes^2 <= 16384, T <= 1024, T H W < 2^31 - 4, dword-aligned maps)");
}

int univs_davis_counts(const uint8_t* gt, const uint8_t* pred, int T, int H, int W, int G, int P, int radius, int use_void,
                       int32_t* region, int32_t* n_gt, int32_t* n_fg, int32_t* match, void* stream) {
  const Entry e("univs_davis_counts", stream);
  if (T < 1 || H < 1 || W < 1 || G < 1 || P < 1 || radius < 1 || (use_void != 0 && use_void != 1))   // (beyond the kernel's sizes: "not covered")
    return e.invalid("bad arguments T=%d H=%d W=%d G=%d P=%d radius=%d use_void=%d", T, H, W, G, P, radius, use_void);
  if (!gt || !pred || !region || !n_gt || !n_fg || !match) return e.null_pointer();
  return e.covered(davis_counts(gt, pred, T, H, W, G, P, radius, use_void, region, n_gt, n_fg, match, e.st), "not covered (G, P <= 32, radius <= 36, T H W < 2^31)");
}

// (include/univs_eval_hip.h)
int univs_vis_overlap_counts(const int32_t* dt_bounds, const int32_t* dt_starts, const int32_t* gt_bounds, const int32_t* gt_ones,
                             const int32_t* gt_starts, int D, int G, int T, int H, int W, int gt_max_bounds, int32_t* inter, void* stream) {
  const Entry e("univs_vis_overlap_counts", stream);
  if (D < 1 || G < 1 || T < 1 || H < 1 || W < 1 || gt_max_bounds < 0 || (long long)D * G * T >= (1LL << 31))
    return e.invalid("bad arguments D=%d G=%d T=%d H=%d W=%d gt_max_bounds=%d (D G T < 2^31)", D, G, T, H, W, gt_max_bounds);
  if (!dt_bounds || !dt_starts || !gt_bounds || !gt_ones || !gt_starts || !inter) return e.null_pointer();
  return e.covered(vis_overlap_counts(dt_bounds, dt_starts, gt_bounds, gt_ones, gt_starts, D, G, T, H, W, gt_max_bounds, inter, e.st),
                   "not covered (H W < 2^31, T <= 65535, at most 16384 boundaries per ground-truth mask: 128 KB of LDS)");
}

// (include/univs_pvos_hip.h)
int univs_pvos_counts(const uint8_t* gt, const uint8_t* pred, int T, int H, int W, int d, int K, int32_t* counts, void* stream) {
  const Entry e("univs_pvos_counts", stream);
  if (T < 1 || H < 1 || W < 1 || d < 1 || K < 1)                  // (beyond the kernel's sizes: "not covered")
    return e.invalid("bad arguments T=%d H=%d W=%d d=%d K=%d", T, H, W, d, K);
  if (!gt || !pred || !counts) return e.null_pointer();
  return e.covered(pvos_counts(gt, pred, T, H, W, d, K, counts, e.st), "not covered (d <= 88, K <= 255, T H W < 2^31)");
}

// (include/univs_semantic_hip.h)
int univs_semantic_quality_counts_f32(const float* mask_embed, const float* features, int T, int N, int C, int HW, int t_step, float t_hi,
                                      float t_lo, int32_t* counts, void* stream) {
  const Entry e("univs_semantic_quality_counts_f32", stream);
  if (T < 1 || N < 1 || C < 1 || HW < 1 || t_step < 1)            // (beyond the kernel's sizes: "not covered")
    return e.invalid("bad arguments T=%d N=%d C=%d HW=%d t_step=%d", T, N, C, HW, t_step);
  if (!mask_embed || !features || !counts) return e.null_pointer();
  return e.covered(semantic_quality_counts_f32(mask_embed, features, T, N, C, HW, t_step, t_hi, t_lo, counts, e.st),
                   "not covered (ceil(T / t_step) HW < 2^31, C HW 4 < 2^31, ceil(T / t_step) <= 65535, N <= 2097120, C <= 315, or up to "
                   "1239 where few rows make a smaller LDS tile)");
}

// (include/univs_frames_hip.h)
int univs_resize_frames_u8(const uint8_t* src, int T, int Hi, int Wi, int Ho, int Wo, const int32_t* first_x, const int32_t* count_x,
                           const int32_t* coef_x, int ksize_x, const int32_t* first_y, const int32_t* count_y, const int32_t* coef_y,
                           int ksize_y, int swap_rb, uint8_t* out, void* stream) {
  const Entry e("univs_resize_frames_u8", stream);
  if (T < 1 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1) return e.invalid("bad arguments T=%d Hi=%d Wi=%d Ho=%d Wo=%d", T, Hi, Wi, Ho, Wo);
  // 2 ceil(max(n_in / n_out, 1)) + 1 in integers
  const long long kx = 2 * (((long long)(Wi > Wo ? Wi : Wo) + Wo - 1) / Wo) + 1, ky = 2 * (((long long)(Hi > Ho ? Hi : Ho) + Ho - 1) / Ho) + 1;
  if (ksize_x != kx || ksize_y != ky)
    return e.invalid("ksize_x=%d ksize_y=%d, but %d -> %d columns have %lld slots and %d -> %d rows %lld", ksize_x, ksize_y, Wi, Wo, kx, Hi, Ho,
                     ky);
  if (!src || !out || (Wi != Wo && (!first_x || !count_x || !coef_x)) || (Hi != Ho && (!first_y || !count_y || !coef_y)))
    return e.null_pointer();
  return e.covered(resize_frames_u8(src, T, Hi, Wi, Ho, Wo, first_x, count_x, coef_x, ksize_x, first_y, count_y, coef_y, ksize_y, swap_rb, out,
                                    e.st),
                   "not covered (ksize_x <= 9 and ksize_y <= 9: a down-scale up to 4; T Hi Wi 3 < 2^31, T 3 Ho Wo < 2^31)");
}

// (include/univs_prompts_hip.h)
int univs_resize_rle_masks_u8(const int32_t* bounds, const int32_t* starts, long long n_bounds, int N, int H, int W, const int32_t* ty,
                              const int32_t* tx, int Ho, int Wo, uint8_t* masks, int32_t* boxes, void* stream) {
  const Entry e("univs_resize_rle_masks_u8", stream);
  if (N < 0 || n_bounds < 0 || H < 1 || W < 1 || Ho < 1 || Wo < 1)
    return e.invalid("bad arguments n_bounds=%lld N=%d H=%d W=%d Ho=%d Wo=%d", n_bounds, N, H, W, Ho, Wo);
  if (N == 0) return UNIVS_OK;
  if (!bounds || !starts || !ty || !tx || !masks || !boxes) return e.null_pointer();
  return e.covered(resize_rle_masks_u8(bounds, starts, n_bounds, N, H, W, ty, tx, Ho, Wo, masks, boxes, e.st),
                   "not covered (H W < 2^31, n_bounds < 2^31, N Ho Wo < 2^31)");
}

// (include/univs_idmap_hip.h)
int univs_idmap_census_u8(const uint8_t* ids, int F, int H, int W, int32_t* count, int32_t* box, void* stream) {
  const Entry e("univs_idmap_census_u8", stream);
  if (F < 0 || H < 1 || W < 1) return e.invalid("bad arguments F=%d H=%d W=%d", F, H, W);
  if (F == 0) return UNIVS_OK;
  if (!ids || !count || !box) return e.null_pointer();
  return e.covered(idmap_census_u8(ids, F, H, W, count, box, e.st), "not covered (F H W < 2^31)");
}

int univs_idmap_prompts_u8(const uint8_t* ids, int F, int H, int W, const int32_t* frame, const int32_t* value, int N, const int32_t* ty,
                           const int32_t* tx, int Ho, int Wo, uint8_t* masks, int32_t* boxes, void* stream) {
  const Entry e("univs_idmap_prompts_u8", stream);
  if (N < 0 || F < 0 || (N > 0 && F == 0) || H < 1 || W < 1 || Ho < 1 || Wo < 1)
    return e.invalid("bad arguments F=%d H=%d W=%d N=%d Ho=%d Wo=%d", F, H, W, N, Ho, Wo);
  if (N == 0) return UNIVS_OK;
  if (!ids || !frame || !value || !ty || !tx || !masks || !boxes) return e.null_pointer();
  return e.covered(idmap_prompts_u8(ids, F, H, W, frame, value, N, ty, tx, Ho, Wo, masks, boxes, e.st),
                   "not covered (F H W < 2^31, N Ho Wo < 2^31)");
}

// (include/univs_imagelabels_hip.h)
int univs_semseg_labels_f32(const float* r, int C, int hi, int wi, int H, int W, uint8_t* labels, void* stream) {
  const Entry e("univs_semseg_labels_f32", stream);
  if (C < 1 || hi < 1 || wi < 1 || H < 1 || W < 1) return e.invalid("bad arguments C=%d hi=%d wi=%d H=%d W=%d", C, hi, wi, H, W);
  if (!r || !labels) return e.null_pointer();
  return e.covered(semseg_labels_f32(r, C, hi, wi, H, W, labels, e.st), "not covered (C <= 256, H W < 2^31, hi wi < 2^31)");
}

int univs_label_confusion_u8(const uint8_t* gt, const uint8_t* pred, long long n, int num_classes, int ignore_label, long long* conf,
                             long long* stray, void* stream) {
  const Entry e("univs_label_confusion_u8", stream);
  if (n < 0 || num_classes < 1 || ignore_label < -1 || ignore_label > 255 || (ignore_label >= 0 && ignore_label < num_classes))
    return e.invalid("bad arguments n=%lld num_classes=%d ignore_label=%d", n, num_classes, ignore_label);
  if (n == 0) return UNIVS_OK;
  if (!gt || !pred || !conf || !stray) return e.null_pointer();
  return e.covered(label_confusion_u8(gt, pred, n, num_classes, ignore_label, conf, stray, e.st),
                   "not covered ((num_classes + 1)^2 <= 32768, n < 2^31 - 4, dword-aligned maps, 8-byte aligned counts)");
}

// (include/univs_text_hip.h)
int univs_text_attention_f32(const float* qkv, const int* start, int S, long long Ntok, int E, int heads, int Lmax, float scale, float* out,
                             void* stream) {
  const Entry e("univs_text_attention_f32", stream);
  if (S < 0 || Ntok < 0 || E < 1 || heads < 1 || E % heads != 0 || Lmax < 1)
    return e.invalid("bad arguments S=%d Ntok=%lld E=%d heads=%d Lmax=%d", S, Ntok, E, heads, Lmax);
  if (S == 0 || Ntok == 0) return UNIVS_OK;
  if (!qkv || !start || !out) return e.null_pointer();
  return e.covered(text_attention_f32(qkv, start, S, Ntok, E, heads, Lmax, scale, out, e.st),
                   "not covered (E / heads in {16, 32, 64}, Lmax <= 128, Ntok 3 E < 2^31, S heads < 2^31)");
}

// (include/univs_polygons_hip.h)
int univs_polygons_to_runs(const double* xy, const int* poly_start, const int* obj_start, const int* size, const long long* slot,
                           long long n_points, int P, int N, long long cap_total, int* bounds, int* ones, int* count, int* status,
                           void* stream) {
  const Entry e("univs_polygons_to_runs", stream);
  if (N < 0 || P < 0 || n_points < 0 || cap_total < 0)
    return e.invalid("bad arguments n_points=%lld P=%d N=%d cap_total=%lld", n_points, P, N, cap_total);
  if (N == 0) return UNIVS_OK;
  if (!xy || !poly_start || !obj_start || !size || !slot || !bounds || !ones || !count || !status) return e.null_pointer();
  if (n_points >= (1LL << 31) || cap_total >= (1LL << 31))
    return e.covered(UNIVS_ERR_NOT_IMPLEMENTED, "not covered (n_points < 2^31, cap_total < 2^31)");
  return polygons_to_runs(xy, poly_start, obj_start, size, slot, n_points, P, N, cap_total, bounds, ones, count, status, e.st);
}

// (include/univs_seam_hip.h)
int univs_small_seam_presplit_f32(const float* x, const void* wpa, const float* winv_a, const float* bias_a, const float* residual,
                                  const float* ln_weight, const float* ln_bias, float ln_eps, float* t, const float* add, const void* wpb,
                                  const float* winv_b, const float* bias_b, int n_wb, int f_off, long long M, int Ka, int Na, int Nb, int relu,
                                  int add_features, float* y, void* stream) {
  const Entry e("univs_small_seam_presplit_f32", stream);
  if (M < 0 || Nb < 0 || Ka < 1 || Na < 1 || n_wb < 1 || f_off < 0 || f_off + Nb > n_wb)
    return e.invalid("bad arguments M=%lld Ka=%d Na=%d Nb=%d n_wb=%d f_off=%d", M, Ka, Na, Nb, n_wb, f_off);
  if (M == 0 || Nb == 0) return UNIVS_OK;
  if (!x || !wpa || !winv_a || !residual || !ln_weight || !t || !wpb || !winv_b || !y) return e.null_pointer();
  return e.covered(small_seam_f32(x, wpa, winv_a, bias_a, residual, ln_weight, ln_bias, ln_eps, t, add, wpb, winv_b, bias_b, n_wb, f_off, y, M,
                                  Ka, Na, Nb, relu, add_features, e.st),
                   "M=%lld Ka=%d Na=%d Nb=%d not covered (Ka == Na == 256, Nb %% 256 == 0, f_off %% 4 == 0, add_features %% 32 == 0, "
                   "M <= 1 048 560, 16-byte aligned pointers)", M, Ka, Na, Nb);
}

int univs_small_mlp_seam_presplit_f32(const float* x, const float* pre_residual, const float* pre_ln_weight, const float* pre_ln_bias,
                                      float pre_ln_eps, float* x_out, const float* side_add, const void* side_wp, const float* side_winv,
                                      const float* side_bias, int side_n_w, int side_f_off, float* side_y, int stages,
                                      const void* const* wp, const float* const* winv, const float* const* bias, const int* relu,
                                      const float* in_ln_weight, const float* in_ln_bias, float in_ln_eps, float* x_normed, long long M,
                                      int out_T, float* y, void* stream) {
  const Entry e("univs_small_mlp_seam_presplit_f32", stream);
  if (M < 0 || stages < 1 || stages > 3 || out_T < 0 || (side_wp && (side_n_w < 1 || side_f_off < 0 || side_f_off + 256 > side_n_w)))
    return e.invalid("bad arguments M=%lld stages=%d out_T=%d side_n_w=%d side_f_off=%d", M, stages, out_T, side_n_w, side_f_off);
  if (M == 0) return UNIVS_OK;
  if (!x || !y || !wp || !winv || !bias || !relu) return e.invalid("NULL pointer");
  return e.covered(small_chain_seam_f32(x, pre_residual, pre_ln_weight, pre_ln_bias, pre_ln_eps, x_out, side_add, side_wp, side_winv, side_bias,
                                        side_n_w, side_f_off, side_y, stages, wp, winv, bias, relu, in_ln_weight, in_ln_bias, in_ln_eps, x_normed, y, M, out_T, e.st),
                   "M=%lld not covered (M <= 1 048 560, out_T | M, 16-byte aligned pointers, x_normed / bias only with a LayerNorm, the "
                   "pre-LayerNorm with weight, bias and x_out, the side stage with its weights and side_y)", M);
}

// (include/univs_png_hip.h)
int univs_png_deflate_maps(const void* src, int src_is_i32, int N, int H, int W, const uint8_t* lut, int K, int C, int rows_per_stripe,
                           uint8_t* scratch, uint8_t* out, long long* offsets, void* stream) {
  const Entry e("univs_png_deflate_maps", stream);
  if (N < 0 || H < 1 || W < 1 || C < 1 || rows_per_stripe < 1 || (lut && K < 1) || (!lut && (src_is_i32 || C != 1)))
    return e.invalid("bad arguments src_is_i32=%d N=%d H=%d W=%d lut=%s K=%d C=%d rows_per_stripe=%d", src_is_i32, N, H, W,
                     lut ? "given" : "NULL", K, C, rows_per_stripe);
  if (N == 0) return UNIVS_OK;
  if (!src || !scratch || !out || !offsets) return e.null_pointer();
  return e.covered(png_deflate_maps(src, src_is_i32, N, H, W, lut, K, C, rows_per_stripe, scratch, out, offsets, e.st),
                   "not covered (C in {1, 3}, rows_per_stripe (W C + 1) <= 24576, N H (W C + 1) < 2^31)");
}

// (include/univs_pngread_hip.h)
int univs_png_read(const uint8_t* streams, const long long* stream_offsets, const int* desc, const uint8_t* palettes, int P,
                   const long long* filt_offsets, const long long* out_offsets, int N, long long streams_total, long long filt_total,
                   long long out_total, int max_rowbytes, uint8_t* filtered, uint8_t* out, int* status, void* stream) {
  const Entry e("univs_png_read", stream);
  if (N < 0 || P < 0 || streams_total < 0 || filt_total < 0 || out_total < 0 || max_rowbytes < 1 || (P > 0 && !palettes))
    return e.invalid("bad arguments N=%d P=%d palettes=%s streams_total=%lld filt_total=%lld out_total=%lld max_rowbytes=%d", N, P,
                     palettes ? "given" : "NULL", streams_total, filt_total, out_total, max_rowbytes);
  if (N == 0) return UNIVS_OK;
  if (!streams || !stream_offsets || !desc || !filt_offsets || !out_offsets || !filtered || !out || !status) return e.null_pointer();
  return e.covered(png_read(streams, stream_offsets, desc, palettes, P, filt_offsets, out_offsets, N, streams_total, filt_total, out_total,
                            max_rowbytes, filtered, out, status, e.st),
                   "not covered (max_rowbytes <= 24576, streams_total, filt_total and out_total < 2^31)");
}

// (include/univs_jpeg_hip.h)
int univs_jpeg_decode(const uint8_t* src, const long long* src_off, const int* ri, const uint8_t* huff, const uint16_t* quant, int N, int W,
                      int H, int ncomp, int h, int v, int subseq_bits, int max_intervals, long long src_total, int phases, uint8_t* comp,
                      int* ivl, int16_t* blocks, uint8_t* planes, uint8_t* out, int* status, int* rounds, void* stream) {
  const Entry e("univs_jpeg_decode", stream);
  if (N < 0 || src_total < 0 || max_intervals < 1 || phases < 1 || phases > 3)
    return e.invalid("bad arguments N=%d src_total=%lld max_intervals=%d phases=%d", N, src_total, max_intervals, phases);
  if (N == 0) return UNIVS_OK;
  if (!src || !src_off || !ri || !huff || !quant || !comp || !ivl || !blocks || !planes || !out || !status || !rounds) return e.null_pointer();
  return e.covered(jpeg_decode(src, src_off, ri, huff, quant, N, W, H, ncomp, h, v, subseq_bits, max_intervals, src_total, phases, comp, ivl,
                               blocks, planes, out, status, rounds, e.st),
                   "not covered (16 <= W, H <= 16384, (ncomp, h, v) in {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}, subseq_bits a multiple of "
                   "32 in [32, 2^20], max_intervals <= 2^20, src_total and 3 N H W < 2^31, out 4-byte and planes 8-byte aligned)");
}

// (include/univs_jpegenc_hip.h)
int univs_jpeg_encode(const uint8_t* rgb, const void* ids, int ids_is_i32, const uint8_t* lut, int K, int edge, int N, int H, int W, int h,
                      int v, int quality, int phases, int16_t* blocks, uint32_t* sizes, long long* bit_off, long long* totals,
                      const long long* raw_off, long long raw_total, uint8_t* raw, uint8_t* out, long long* out_len, int* status, void* stream) {
  const Entry e("univs_jpeg_encode", stream);
  if (N < 0 || phases < 1 || phases > 3 || raw_total < 0 || (ids && (K < 1 || edge < -1 || edge > 0xFFFFFF)))
    return e.invalid("bad arguments N=%d phases=%d raw_total=%lld ids=%s K=%d edge=%d", N, phases, raw_total, ids ? "given" : "NULL", K, edge);
  if (N == 0) return UNIVS_OK;
  if (!rgb || (ids && !lut) || !blocks || !sizes || !bit_off || !totals || !status || ((phases & 2) && (!raw_off || !raw || !out || !out_len)))
    return e.null_pointer();
  return e.covered(jpeg_encode(rgb, ids, ids_is_i32, lut, K, edge, N, H, W, h, v, quality, phases, blocks, sizes, bit_off, totals, raw_off,
                               raw_total, raw, out, out_len, status, e.st),
                   "not covered (1 <= W, H <= 16384, (h, v) in {(1, 1), (2, 1), (2, 2)}, 1 <= quality <= 100, 3 N H W < 2^31, raw_total < 2^40, "
                   "blocks 16-byte and raw 4-byte aligned)");
}

// (include/univs_hota_hip.h)
int univs_hota_counts(const int32_t* inter, const int32_t* gt_area, const int32_t* tr_area, int D, int G, int T, const int32_t* gt_ids,
                      const int32_t* gt_starts, const int32_t* tr_ids, const int32_t* tr_starts, int C, int max_g, int max_p,
                      const double* thresholds, int A, int32_t* tp_fn_fp, int32_t* matches, double* loca_sum, int32_t* gt_id_count,
                      int32_t* tracker_id_count, int32_t* match_col, void* stream) {
  const Entry e("univs_hota_counts", stream);
  if (D < 1 || G < 1 || T < 1 || C < 1 || A < 1 || max_g < 0 || max_p < 0)
    return e.invalid("bad arguments D=%d G=%d T=%d C=%d max_g=%d max_p=%d A=%d", D, G, T, C, max_g, max_p, A);
  if (!inter || !gt_area || !tr_area || !gt_ids || !gt_starts || !tr_ids || !tr_starts || !thresholds || !tp_fn_fp || !matches || !loca_sum ||
      !gt_id_count || !tracker_id_count || !match_col)
    return e.null_pointer();
  return e.covered(hota_counts(inter, gt_area, tr_area, D, G, T, gt_ids, gt_starts, tr_ids, tr_starts, C, max_g, max_p, thresholds, A, tp_fn_fp,
                               matches, loca_sum, gt_id_count, tracker_id_count, match_col, e.st),
                   "not covered (at most 64 ids per side of a class, A <= 32, T <= 65535, D G T < 2^31)");
}

int univs_lsa_max_f64(const double* score, const int32_t* rows, const int32_t* cols, int B, int32_t* col_of_row, void* stream) {
  const Entry e("univs_lsa_max_f64", stream);
  if (B < 0) return e.invalid("bad arguments B=%d", B);
  if (B == 0) return UNIVS_OK;
  if (!score || !rows || !cols || !col_of_row) return e.null_pointer();
  return lsa_max_f64(score, rows, cols, B, col_of_row, e.st);
}

// The two window-attention entries on image-layout operands share their checks
static int window_image_checks(const Entry& e, const float* qkv, const float* bias, const float* out, int B, int H, int W, int ws, int shift, int nH,
                               int hd) {
  if (B < 0 || H < 1 || W < 1 || ws < 1 || shift < 0 || shift >= ws || nH < 1 || hd < 1)
    return e.invalid("bad dimensions B=%d H=%d W=%d ws=%d shift=%d nH=%d hd=%d", B, H, W, ws, shift, nH, hd);
  if (B > 0 && (!qkv || !bias || !out)) return e.null_pointer();
  return UNIVS_OK;
}

int univs_window_attention_image_f32(const float* qkv, const float* qkv_bias, const float* bias,
                                     const float* shift_mask, int B, int H, int W, int ws, int shift, int nH,
                                     int hd, float scale, float* out, void* stream) {
  const Entry e("univs_window_attention_image_f32", stream);
  const int rc = window_image_checks(e, qkv, bias, out, B, H, W, ws, shift, nH, hd);
  if (rc != UNIVS_OK || B == 0) return rc;
  return window_attention_image_f32(qkv, qkv_bias, bias, shift_mask, B, H, W, ws, shift, nH, hd, scale, out, e.st);
}

int univs_window_attention_image_mma(const float* qkv, const float* qkv_bias, const float* bias,
                                     const float* shift_mask, int B, int H, int W, int ws, int shift, int nH,
                                     int hd, float scale, int mma, float* out, void* stream) {
  if (mma == UNIVS_MMA_F32)
    return univs_window_attention_image_f32(qkv, qkv_bias, bias, shift_mask, B, H, W, ws, shift, nH, hd, scale, out, stream);
  const Entry e("univs_window_attention_image_mma", stream);
  if (mma != UNIVS_MMA_F16 && mma != UNIVS_MMA_F16X3)
    return e.invalid("mma=%d (UNIVS_MMA_F32 = 0, UNIVS_MMA_F16 = 1 or UNIVS_MMA_F16X3 = 2)", mma);
  int rc = window_image_checks(e, qkv, bias, out, B, H, W, ws, shift, nH, hd);
  if (rc != UNIVS_OK || B == 0) return rc;
  rc = window_attention_image_f16mma(qkv, qkv_bias, bias, shift_mask, B, H, W, ws, shift, nH, hd, scale, mma == UNIVS_MMA_F16X3 ? 3 : 1, out,
                                     e.st);
  if (rc == UNIVS_ERR_NOT_IMPLEMENTED && mma == UNIVS_MMA_F16X3)      // windows beyond 9 x 9: the exact kernel (same accuracy class)
    return univs_window_attention_image_f32(qkv, qkv_bias, bias, shift_mask, B, H, W, ws, shift, nH, hd, scale, out, stream);
  return rc;
}

int univs_swin_window_attention_qkv_presplit_f32(const float* x, const void* wp, const float* winv, const float* qkv_bias,
                                                 const float* rel_bias, const float* shift_mask, int B, int H, int W, int ws, int shift,
                                                 int nH, int C, float scale, float* out, void* stream) {
  const Entry e("univs_swin_window_attention_qkv_presplit_f32", stream);
  if (B < 0 || H < 1 || W < 1 || ws < 1 || shift < 0 || shift >= ws || nH < 1 || C < 1)
    return e.invalid("bad dimensions B=%d H=%d W=%d ws=%d shift=%d nH=%d C=%d", B, H, W, ws, shift, nH, C);
  if (B == 0) return UNIVS_OK;
  if (!x || !wp || !winv || !rel_bias || !out) return e.null_pointer();
  return e.launched(window_attention_qkv_f16x3(x, wp, winv, qkv_bias, rel_bias, shift ? shift_mask : nullptr, B, H, W, ws, shift, nH, C, scale,
                                               out, e.st),
                    "not covered (7 x 7 windows, C == 32 nH in {96, 192}, x and the weight image 16-byte aligned, B H W C 4 < 2^31 - 1)");
}

int univs_msda_prepare_f32(const float* proj, int row_stride, int n_off, const float* ref_points,
                           long long ref_batch_stride, const int64_t* spatial_shapes, int N, int Lq, int M, int L,
                           int P, float* loc, float* attn, void* stream) {
  const Entry e("univs_msda_prepare_f32", stream);
  if (N < 0 || Lq < 0 || M < 1 || L < 1 || L > UNIVS_MAX_LEVELS || P < 1 || row_stride < M * L * P * 3 || n_off < M * L * P * 2 ||
      n_off + M * L * P > row_stride || ref_batch_stride < 0)
    return e.invalid("bad dimensions N=%d Lq=%d M=%d L=%d P=%d row_stride=%d n_off=%d", N, Lq, M, L, P, row_stride, n_off);
  if ((long long)N * Lq == 0) return UNIVS_OK;
  if (!proj || !ref_points || !spatial_shapes || !loc || !attn) return e.invalid("NULL pointer");
  LevelTable lv;
  for (int l = 0; l < UNIVS_MAX_LEVELS; ++l) {
    lv.H[l] = l < L ? (int)spatial_shapes[2 * l] : 0;
    lv.W[l] = l < L ? (int)spatial_shapes[2 * l + 1] : 0;
    lv.start[l] = 0;
    if (l < L && (lv.H[l] < 1 || lv.W[l] < 1)) return e.invalid("level %d has an empty shape", l);
  }
  return e.covered(msda_prepare_f32(proj, row_stride, n_off, ref_points, ref_batch_stride, lv, N, Lq, M, L, P, loc, attn, e.st),
                   "(L=%d, P=%d) not instantiated (P == 4, L <= 4)", L, P);
}

int univs_linear_blocked_f32(const float* x, const float* weight, const float* bias, long long M, int N, int K,
                             int rows_per_batch, int col_block, float* y, void* stream) {
  const Entry e("univs_linear_blocked_f32", stream);
  return linear_blocked_entry(e, M, N, K, rows_per_batch, col_block, x && weight && y, [&] {
    return linear_split_f32(x, weight, bias, nullptr, y, M, N, K, /*LS_EPI_BLOCKED=*/4, e.st, rows_per_batch, col_block);
  });
}

// The two head-major MSDA entry points differ in the kernel (`forward`, generation `gen`) and in what it covers (`covers`).
typedef int (*MsdaHeadMajorFn)(const float*, const LevelTable&, const float*, const float*, long long, int, int, int, int, int, int, int,
                               float*, hipStream_t);
static int msda_forward_head_major(const Entry& e, MsdaHeadMajorFn forward, int gen, const char* covers, const float* value_hm,
                                   const int64_t* spatial_shapes, const int64_t* level_start, const float* proj_hm,
                                   const float* ref_points, long long ref_batch_stride, int N, int S, int M, int D, int L, int Lq, int P,
                                   float* out) {
  if (N < 0 || S < 0 || M < 1 || D < 0 || Lq < 0 || P < 1 || L < 1 || L > UNIVS_MAX_LEVELS || ref_batch_stride < 0)
    return e.invalid("bad dimensions N=%d S=%d M=%d D=%d L=%d Lq=%d P=%d", N, S, M, D, L, Lq, P);
  if ((long long)N * Lq * M * D == 0) return UNIVS_OK;
  g_msda_gen = 0;
  if (!value_hm || !proj_hm || !ref_points || !out) return e.null_pointer();
  LevelTable lv;
  int rc = make_levels(e, spatial_shapes, level_start, L, S, &lv);
  if (rc != UNIVS_OK) return rc;
  // the generic kernel was forced: it has no head-major variant, the caller takes the two-operator path
  if (config().msda_impl == 1) return e.covered(UNIVS_ERR_NOT_IMPLEMENTED, "generic implementation forced (univs_msda_set_impl(1))");
  rc = forward(value_hm, lv, proj_hm, ref_points, ref_batch_stride, N, S, M, D, L, Lq, P, out, e.st);
  if (rc > 0) {
    g_msda_last = 2;
    g_msda_gen = gen;
  }
  return e.launched(rc, "geometry not covered (%s)", covers);
}

int univs_msda_forward_strips_f32(const float* value_hm, const int64_t* spatial_shapes, const int64_t* level_start,
                                  const float* proj_hm, const float* ref_points, long long ref_batch_stride, int N, int S, int M,
                                  int D, int L, int Lq, int P, float* out, void* stream) {
  return msda_forward_head_major(Entry("univs_msda_forward_strips_f32", stream), msda_forward_strips_f32, 5,
                                 "D == 32, P == 4, 1 <= L <= 4, Lq == S, windows within 80 KB of LDS", value_hm, spatial_shapes,
                                 level_start, proj_hm, ref_points, ref_batch_stride, N, S, M, D, L, Lq, P, out);
}

int univs_msda_forward_heads_f32(const float* value_hm, const int64_t* spatial_shapes, const int64_t* level_start,
                                 const float* proj_hm, const float* ref_points, long long ref_batch_stride, int N, int S, int M,
                                 int D, int L, int Lq, int P, float* out, void* stream) {
  return msda_forward_head_major(Entry("univs_msda_forward_heads_f32", stream), msda_forward_heads_f32, 6,
                                 "D == 32, P == 4, 1 <= L <= 4, Lq == S, windows within 160 KB of LDS", value_hm, spatial_shapes,
                                 level_start, proj_hm, ref_points, ref_batch_stride, N, S, M, D, L, Lq, P, out);
}

}  // extern "C"
