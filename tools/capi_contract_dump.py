"""The host contract of the C ABI, one line per call: `name | scalar arguments | return code | univs_last_error()`.

Every entry of include/univs_hip.h is called through ctypes with EVERY DATA POINTER NULL, so no call gets past an entry's NULL check
and nothing is launched -- the table can be printed on any machine.  (The one pointer ever set is univs_configure's `cfg`, a host
struct: its rows give the members to set, `size` defaulting to sizeof(UnivsConfig).)  Per entry: the integer arguments set uniformly
to -1, 0, 1 and 32 (floats are 1), then hand-picked rows (`ROWS`: overrides on the all-ones row) that reach each distinct message an
entry reports before its NULL check and each empty-shape UNIVS_OK.  The process's settings are put back at the end.
tests/test_capi_contract_cpu.py compares the output with tests/capi_contract_table.txt, which was printed at the commit before the
entries of csrc/capi.hip were folded.

    python tools/capi_contract_dump.py            (UNIVS_HIP_LIB=... for another build of the library)
"""
import ctypes
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from univs_amd import _lib  # noqa: E402

BIG = 0x80000000   # one past INT32_MAX, for the long long arguments

ROWS = [
    ("univs_get_config", {}), ("univs_configure", {}), ("univs_configure", dict(cfg=dict(size=4))), ("univs_configure", dict(cfg=dict(size=8))),
    ("univs_configure", dict(cfg=dict(size=84))), ("univs_configure", dict(cfg=dict(msda_impl=3))), ("univs_configure", dict(cfg=dict(msda_halo=65))),
    ("univs_configure", dict(cfg=dict(mask_decode_ct=3))), ("univs_configure", dict(cfg=dict(linear_terms=4))),
    ("univs_configure", dict(cfg=dict(mask_decode_wave_tiles=65))), ("univs_configure", dict(cfg=dict(msda_impl=2, msda_halo=64, linear_terms=6))),
    ("univs_linear_fused_f32", dict(M=0)), ("univs_linear_fused_f32", dict(N=0)), ("univs_linear_fused_f32", dict(act=3)),
    ("univs_linear_presplit_f32", dict(M=0)), ("univs_linear_presplit_f32", dict(N=0)), ("univs_linear_presplit_f32", dict(K=0)),
    ("univs_linear_resident_presplit_f32", dict(M=0)), ("univs_linear_resident_presplit_f32", dict(N=0)),
    ("univs_linear_blocked_f32", dict(N=4, col_block=4)), ("univs_linear_blocked_f32", dict(M=0, N=4, col_block=4)),
    ("univs_linear_blocked_f32", dict(M=3, rows_per_batch=2, N=4, col_block=4)), ("univs_linear_blocked_f32", dict(N=6, col_block=4)),
    ("univs_linear_blocked_presplit_f32", dict(N=4, col_block=4)), ("univs_linear_blocked_presplit_f32", dict(M=0, N=4, col_block=4)),
    ("univs_presplit_weights_f32", dict(N=1, K=32, conv=0)), ("univs_presplit_weights_f32", dict(N=0, K=32, conv=0)),
    ("univs_presplit_weights_f32", dict(N=1, K=32, conv=1)), ("univs_presplit_weights_f32", dict(N=1, K=288, conv=1)),
    ("univs_presplit_weights_f32", dict(N=1, K=32, conv=3)),
    ("univs_conv1x1_presplit_f32", dict(T=0)), ("univs_conv1x1_presplit_f32", dict(Cout=0)), ("univs_conv1x1_presplit_f32", dict(Cin=0)),
    ("univs_conv3x3_presplit_f32", dict(T=0)), ("univs_conv3x3_presplit_f32", dict(H=0)),
    ("univs_conv3x3_nhwc_presplit_f32", dict(T=0)), ("univs_conv3x3_nhwc_presplit_f32", dict(W=0)),
    ("univs_cross_attention_f32", dict(L=0)), ("univs_cross_attention_f32", dict(N=0)), ("univs_cross_attention_f32", dict(head_dim=0)),
    ("univs_cross_attention_flagged_f32", dict(L=0)), ("univs_cross_attention_flagged_f32", dict(N=0)),
    ("univs_mlp_presplit_f32", dict(M=0)), ("univs_mlp_presplit_f32", dict(act=2)), ("univs_mlp_presplit_f32", dict(act=0)),
    ("univs_mlp_presplit_v2_f32", dict(M=0)), ("univs_mlp_presplit_v2_f32", dict(act=3)), ("univs_mlp_presplit_v2_f32", dict(flags=4, act=2)),
    ("univs_small_linear_presplit_f32", dict(f_off=0)), ("univs_small_linear_presplit_f32", dict(f_off=0, M=0)),
    ("univs_small_linear_presplit_f32", dict(f_off=0, N=0)), ("univs_small_linear_presplit_f32", dict(f_off=0, n_w=0)),
    ("univs_small_mlp_presplit_f32", dict(M=0)), ("univs_small_mlp_presplit_f32", dict(stages=4)), ("univs_small_mlp_presplit_f32", dict(stages=3)),
    ("univs_patch_embed4_f32", dict(T=0)), ("univs_patch_embed4_f32", dict(H=0)), ("univs_patch_embed4_f32", dict(W=0)),
    ("univs_decoder_memory_f32", dict(C=0)), ("univs_decoder_memory_f32", dict(HW=0)),
    ("univs_transpose_f32", dict(B=0)), ("univs_transpose_f32", dict(R=0)),
    ("univs_transpose_strided_f32", dict(R=2, C=2, in_batch_stride=3)), ("univs_transpose_strided_f32", dict(R=2, C=2, in_batch_stride=4)),
    ("univs_transpose_strided_f32", dict(C=0, in_batch_stride=0)),
    ("univs_transpose_ex_f32", dict(R=2, C=2, in_batch_stride=0, out_batch_stride=3)),
    ("univs_transpose_ex_f32", dict(R=2, C=2, in_batch_stride=4, out_batch_stride=0)), ("univs_transpose_ex_f32", dict(B=0)),
    ("univs_msda_forward_f32", dict(D=0)), ("univs_msda_forward_f32", dict(P=-1)),
    ("univs_msda_forward_f64", dict(Lq=0)), ("univs_msda_forward_f64", dict(S=-1)),
    ("univs_msda_backward_f32", dict(S=0)), ("univs_msda_backward_f32", dict(N=0)), ("univs_msda_backward_f32", dict(N=0, L=9)),
    ("univs_msda_backward_f32", dict(L=-1)),
    ("univs_msda_forward_strips_f32", dict(N=0)), ("univs_msda_forward_strips_f32", dict(L=9)), ("univs_msda_forward_strips_f32", dict(D=0)),
    ("univs_msda_forward_heads_f32", dict(N=0)), ("univs_msda_forward_heads_f32", dict(ref_batch_stride=-1)), ("univs_msda_forward_heads_f32", dict(Lq=0)),
    ("univs_msda_prepare_f32", dict(row_stride=3, n_off=2)), ("univs_msda_prepare_f32", dict(row_stride=3, n_off=2, N=0)),
    ("univs_msda_prepare_f32", dict(row_stride=3, n_off=2, Lq=0)), ("univs_msda_prepare_f32", dict(row_stride=3, n_off=3)),
    ("univs_msda_prepare_f32", dict(row_stride=27, n_off=18, L=9)),
    ("univs_mask_decode_f32", dict(T=0)), ("univs_mask_decode_f32", dict(HW=0)), ("univs_mask_decode_f32", dict(Q=0, C=0)),
    ("univs_mask_decode_attn_f32", dict(Q=0)), ("univs_mask_decode_attn_f32", dict(hw=0)),
    ("univs_mask_decode_attn_deferred_f32", dict(T=0)), ("univs_mask_decode_attn_deferred_f32", dict(generation=0)),
    ("univs_attn_mask_rows_reset", dict(rows=BIG)), ("univs_attn_mask_rows_reset", dict(hw=0)), ("univs_attn_mask_rows_reset", dict(rows=0x7fffffff)),
    ("univs_window_attention_f32", dict(B_=0)), ("univs_window_attention_f32", dict(B_=2, nW=0)), ("univs_window_attention_f32", dict(hd=0)),
    ("univs_window_attention_image_f32", dict(shift=0)), ("univs_window_attention_image_f32", dict(shift=0, B=0)),
    ("univs_window_attention_image_f32", dict(shift=2, ws=2)),
    ("univs_window_attention_image_mma", dict(shift=0, mma=0)), ("univs_window_attention_image_mma", dict(shift=0, mma=1)),
    ("univs_window_attention_image_mma", dict(shift=0, mma=2)), ("univs_window_attention_image_mma", dict(shift=0, mma=3)),
    ("univs_window_attention_image_mma", dict(shift=0, mma=2, B=0)), ("univs_window_attention_image_mma", dict(shift=0, mma=0, B=0)),
    ("univs_window_attention_image_mma", dict(mma=2)), ("univs_window_attention_image_mma", dict(mma=0)),
    ("univs_bilinear_resample_f32", dict(planes=0)), ("univs_bilinear_resample_f32", dict(Wout=0)),
    ("univs_normalize_pad_f32", dict(T=0)), ("univs_normalize_pad_f32", dict(H=2)), ("univs_normalize_pad_f32", dict(Hp=2, Wp=3)),
    ("univs_bilinear_crop_nearest_f32", dict(t_first=0)), ("univs_bilinear_crop_nearest_f32", dict(t_first=0, K=0)),
    ("univs_bilinear_crop_nearest_f32", dict(t_first=-1)), ("univs_bilinear_crop_nearest_f32", dict(t_first=0, t_step=0)),
    ("univs_bilinear_crop_nearest_f32", dict(t_first=0, K=2)), ("univs_bilinear_crop_nearest_f32", dict(T=3, t_first=0, t_step=2, K=2)),
    ("univs_bilinear_crop_nearest_f32", dict(t_first=0, Hi=2)), ("univs_bilinear_crop_nearest_f32", dict(t_first=5, K=-1)),
    ("univs_bilinear_crop_nearest_f32", dict(T=0, t_first=-1, K=0)),
    ("univs_upsample2x_add_f32", dict(planes=0)), ("univs_upsample2x_add_f32", dict(Win=0)),
    ("univs_group_norm_affine_f32", dict(N=0)), ("univs_group_norm_affine_f32", dict(HW=0)), ("univs_group_norm_affine_f32", dict(C=3, groups=2)),
    ("univs_group_norm_affine_f32", dict(N=65536, C=32768)),
    ("univs_group_norm_f32", dict(N=0)), ("univs_group_norm_f32", dict(HW=0)), ("univs_group_norm_f32", dict(C=3, groups=2)),
    ("univs_group_norm_f32", dict(N=65536, C=32768)),
    ("univs_bilinear_pyramid3_f32", dict(H=8, W=8)), ("univs_bilinear_pyramid3_f32", dict(planes=0, H=8, W=8)), ("univs_bilinear_pyramid3_f32", dict(H=8, W=7)),
    ("univs_layer_norm_f32", dict(rows=0)), ("univs_layer_norm_add_f32", dict(rows=0)), ("univs_layer_norm_add_f32", dict(rows=0, C=0)),
    ("univs_patch_merge_norm_f32", dict(B=0)), ("univs_patch_merge_norm_f32", dict(H=0)), ("univs_patch_merge_norm_f32", dict(W=0)),
    ("univs_masked_softmax_f32", dict(S=0)), ("univs_masked_softmax_f32", dict(N=0, S=-1)),
    ("univs_proca_attention_f32", dict(Qp=0)), ("univs_proca_attention_f32", dict(T=0)), ("univs_proca_attention_f32", dict(L=0)),
    ("univs_prompt_prefix_f32", dict(F=0)), ("univs_prompt_prefix_f32", dict(n=0)), ("univs_prompt_prefix_f32", dict(h=3, scale=2)),
    ("univs_prompt_prefix_f32", dict(F=256, n=256)), ("univs_prompt_prefix_f32", dict(F=255, n=257)),
    ("univs_prompt_draw", dict(F=0)), ("univs_prompt_draw", dict(n=0)), ("univs_prompt_draw", dict(F=256, n=256)), ("univs_prompt_draw", dict(R=0)),
    ("univs_prompt_tokens_f32", dict(F=0)), ("univs_prompt_tokens_f32", dict(n=0)), ("univs_prompt_tokens_f32", dict(F=256, n=256)),
    ("univs_prompt_tokens_f32", dict(F=0, T=0)),
    ("univs_prompt_point_pe_f32", dict(F=0)), ("univs_prompt_point_pe_f32", dict(n=0)), ("univs_prompt_point_pe_f32", dict(F=0, Fq=0)),
    ("univs_token_mean_f32", dict(n=0)), ("univs_token_mean_f32", dict(T=0)), ("univs_token_mean_f32", dict(L=0)),
    ("univs_mask_stats_f32", dict(planes=0)), ("univs_mask_stats_f32", dict(planes=BIG)), ("univs_mask_stats_f32", dict(h_valid=2)),
    ("univs_mask_stats_f32", dict(planes=70000)),
    ("univs_mask_stats_strided_f32", dict(outer=0)), ("univs_mask_stats_strided_f32", dict(H=2, W=2, stride_inner=3)),
    ("univs_mask_stats_strided_f32", dict(H=2, W=2, stride_inner=4)), ("univs_mask_stats_strided_f32", dict(w_valid=2)),
    ("univs_image_mask_stats_f32", dict(hi=2)), ("univs_image_mask_stats_f32", dict(Hp=65536, Wp=65536)),
    ("univs_image_panoptic_ids_f32", dict(K=0)), ("univs_image_panoptic_ids_f32", dict(K=0, Q=0)), ("univs_image_panoptic_ids_f32", dict(Q=0)),
    ("univs_image_panoptic_paint_i32", dict(K=0)), ("univs_image_panoptic_paint_i32", dict(H0=65536, W0=65536)),
    ("univs_image_semseg_f32", dict(Qs=-1)), ("univs_image_semseg_f32", dict(C=0)), ("univs_image_semseg_f32", dict(Qs=0)),
    ("univs_image_semseg_f32", dict(Q=0)), ("univs_image_semseg_f32", dict(Q=0, C=0)),
    ("univs_image_instance_masks_u8", dict(N=0)), ("univs_image_instance_masks_u8", dict(N=-1)), ("univs_image_instance_masks_u8", dict(Q=0)),
    ("univs_image_instance_masks_u8", dict(H0=65536, W0=65536)), ("univs_image_instance_masks_u8", dict(N=0, W0=0)),
    ("univs_minvis_accumulate_f32", dict(i=0)), ("univs_minvis_accumulate_f32", dict(i=0, Q=0)), ("univs_minvis_accumulate_f32", dict(V=2)),
    ("univs_minvis_accumulate_f32", dict(i=0, Q=0, T=0)),
    ("univs_video_mask_stats_f32", dict(K=0)), ("univs_video_mask_stats_f32", dict(K=-1)), ("univs_video_mask_stats_f32", dict(step=0)),
    ("univs_video_mask_stats_f32", dict(V=0)), ("univs_video_mask_stats_f32", dict(V=0, K=-1)), ("univs_video_mask_stats_f32", dict(Q=0)),
    ("univs_video_mask_stats_f32", dict(Q=0, K=0, step=0)),
    ("univs_video_instance_masks_u8", dict(N=0)), ("univs_video_instance_masks_u8", dict(N=-1)), ("univs_video_instance_masks_u8", dict(V=0)),
    ("univs_video_instance_masks_u8", dict(N=0, H0=0)),
    ("univs_video_panoptic_ids_i32", dict(K=0)), ("univs_video_panoptic_ids_i32", dict(V=0)), ("univs_video_panoptic_ids_i32", dict(V=0, K=0)),
    ("univs_video_panoptic_ids_i32", dict(hi=2)),
    ("univs_video_panoptic_counts_i32", dict(K=0)), ("univs_video_panoptic_counts_i32", dict(V=0)), ("univs_video_panoptic_counts_i32", dict(H0=0)),
    ("univs_video_panoptic_paint_i32", dict(K=0)), ("univs_video_panoptic_paint_i32", dict(V=0)), ("univs_video_panoptic_paint_i32", dict(W0=0)),
    ("univs_panoptic_pair_counts", dict(G=0)), ("univs_panoptic_pair_counts", dict(T=0)),
    ("univs_vss_video_counts", dict(num_classes=0)), ("univs_vss_video_counts", dict(T=0)),
    ("univs_davis_counts", dict(use_void=2)), ("univs_davis_counts", dict(use_void=0)), ("univs_davis_counts", dict(radius=0)),
]


def parameters(name, header):
    """[(parameter name, ctypes type)] of the prototype `name`."""
    params = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", header).group(1)
    names = [] if params.strip() == "void" else [p.replace("*", " ").split()[-1] for p in params.split(",")]
    return list(zip(names, _lib.SIGNATURES[name][1]))


class UnivsConfig(ctypes.Structure):
    _fields_ = _lib.CONFIG_FIELDS


def main():
    lib = _lib.load()
    before = UnivsConfig()                 # the process's settings: put back at the end
    lib.univs_get_config(ctypes.byref(before))
    header = _lib.strip_header(open(_lib.HEADER_PATH).read())
    rows = [(n, v) for n in _lib.SIGNATURES for v in (-1, 0, 1, 32)] + ROWS
    done = set()
    for name, how in sorted(rows, key=lambda r: r[0]):     # stable: uniform rows first, then ROWS in their order
        params = parameters(name, header)
        unknown = set(how) - {p for p, _ in params} if isinstance(how, dict) else ()
        if unknown:
            raise KeyError(f"{name}: no parameter {sorted(unknown)}")
        values, shown = [], []
        for p, t in params:
            v = (how.get(p) if isinstance(how, dict) else None) if t is ctypes.c_void_p else (how.get(p, 1) if isinstance(how, dict) else how)
            if isinstance(v, dict):        # univs_configure's host struct
                shown.append(f"{p}={{{' '.join(f'{k}={x}' for k, x in v.items())}}}")
                v = ctypes.pointer(UnivsConfig(**{"size": ctypes.sizeof(UnivsConfig), **v}))
            elif v is not None:
                v = 1.0 if t is ctypes.c_float else v
                shown.append(f"{p}={v:g}" if isinstance(v, float) else f"{p}={v}")
            values.append(v)
        shown = " ".join(shown)
        if (name, shown) in done:          # an entry without integer arguments has one uniform row, not four
            continue
        done.add((name, shown))
        rc = getattr(lib, name)(*values)
        if isinstance(rc, bytes):
            rc = rc.decode()
        err = lib.univs_last_error().decode() if isinstance(rc, int) and rc < 0 else ""
        print(f"{name} | {shown} | {rc} | {err}")
        lib.univs_configure(None)          # the settings entries change process-wide state
    lib.univs_configure(ctypes.byref(before))


if __name__ == "__main__":
    main()
