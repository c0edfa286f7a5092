"""GPU: every entry whose "not covered" text csrc/capi.hip composes, called once through ctypes with the smallest shape outside the stated
limit: UNIVS_ERR_NOT_IMPLEMENTED and the exact message, copied as a literal from capi.hip as it stood before its entries were folded
into one skeleton.  Every tensor is real device memory sized for the shape passed, so a case that turned out to be covered would run
its kernel on valid memory.  Not here: univs_bilinear_crop_nearest_f32, whose smallest uncovered plane holds 2^31 floats (8 GiB).
The limits at 65 535 planes / rows and at C > 65535 * 160 need 0.25 - 42 MB of (never touched) memory; the rest a few KB."""
import ctypes

import pytest
import torch

from univs_amd import _lib

pytestmark = pytest.mark.gpu

F32, I32, U8, I64 = torch.float32, torch.int32, torch.uint8, torch.int64


class Mem:
    """Device tensors of a case, kept alive until the call has returned."""

    def __init__(self, dev):
        self.dev, self.keep = dev, []

    def __call__(self, n, dtype=F32):
        t = torch.zeros(max(int(n), 1), dtype=dtype, device=self.dev)
        self.keep.append(t)
        return t.data_ptr()

    def host(self, ctype, values):
        a = (ctype * len(values))(*values)
        self.keep.append(a)
        return a


def linear(name, presplit, blocked=False):
    M, N, K = 8, 8, 32                                            # M < 2048

    def args(d):
        w = [d(N * K), d(N)] if presplit else [d(N * K)]
        if blocked:
            return [d(M * K), *w, d(N), M, N, K, 8, 4, d(M * N)]
        return [d(M * K), *w, d(N), None, M, N, K, 0, d(M * N)]
    tail = " (K == 256, M >= 2048)" if blocked else ""
    return pytest.param(name, args, f"{name}: shape M=8 N=8 K=32 (or alignment) is not covered{tail}", id=name)


def conv(name, taps, covers):
    T, Cin, Cout, H, W = 1, 8, 16, 4, 4                           # Cin % 96, % 128 != 0, 16 pixels

    def args(d):
        bias = [d(Cout)] if taps == 1 else []
        return [d(T * Cin * H * W), d(Cout * Cin * taps), d(Cout), *bias, T, Cin, Cout, H, W, d(T * Cout * H * W)]
    return pytest.param(name, args, f"{name}: T=1 Cin=8 Cout=16 H=4 W=4 not covered ({covers})", id=name)


def mlp(name, v2):
    M, C, Hd = 8, 64, 32                                          # C not in 96 / 128 / 192 / 256 / 384

    def args(d):
        return [d(M * C), d(Hd * C), d(Hd), d(Hd), d(C * Hd), d(C), d(C), None, *([0] if v2 else []), None, None, 1e-5, None, None, 1e-5,
                None, 0, None, M, C, Hd, 1, d(M * C)]
    return pytest.param(name, args, "univs_mlp_presplit_f32: shape M=8 C=64 Hd=32 (or alignment) is not covered (C in 96 / 128 / 192 / 256 / 384, "
                        "Hd % 32 == 0, M >= 2048)", id=name)


def layer_norm(name, add):
    rows, C = 2, 6                                                # C % 4 != 0

    def args(d):
        if add:
            return [d(rows * C), d(rows * C), d(C), d(C), d(C), 1, rows, C, 1e-5, None, d(rows * C), d(rows * C)]
        return [d(rows * C), None, d(C), d(C), rows, C, 1e-5, None, d(rows * C)]
    return pytest.param(name, args, "univs_layer_norm_f32: C=6 not supported (C % 4 == 0, C <= 3072)", id=name)


def msda_head_major(name, lds, D, forced):
    N, S, M, L, P = 1, 4, 1, 1, 4                                 # one 2 x 2 level; D != 32, or the generic kernel forced

    def args(d):
        return [d(N * M * S * D), d.host(ctypes.c_int64, [2, 2]), d.host(ctypes.c_int64, [0]), d(N * M * S * P * 3 * L), d(S * 2), 0,
                N, S, M, D, L, S, P, d(N * S * M * D)]
    text = "generic implementation forced (univs_msda_set_impl(1))" if forced else \
        f"geometry not covered (D == 32, P == 4, 1 <= L <= 4, Lq == S, windows within {lds} KB of LDS)"
    return pytest.param(name, args, f"{name}: {text}", id=name + ("-forced" if forced else ""))


K_KEPT = 4097           # UNIVS_IMAGE_MAX_KEPT + 1
MANY = 65536            # one more than a grid dimension

CASES = [
    linear("univs_linear_fused_f32", False), linear("univs_linear_presplit_f32", True), linear("univs_linear_resident_presplit_f32", True),
    linear("univs_linear_blocked_f32", False, blocked=True), linear("univs_linear_blocked_presplit_f32", True, blocked=True),
    conv("univs_conv1x1_presplit_f32", 1, "Cin % 96 or % 128, Cout % 16, >= 4096 pixels"),
    conv("univs_conv3x3_presplit_f32", 9, "Cin % 128, Cout % 16, >= 4096 pixels"),
    conv("univs_conv3x3_nhwc_presplit_f32", 9, "Cin % 128, Cout % 16, >= 4096 pixels"),
    pytest.param("univs_cross_attention_f32",                    # head_dim 16; L=4 S=32 N=1 H=1
                 lambda d: [d(4 * 16), d(32 * 16), d(32 * 16), None, 4, 32, 1, 1, 16, 0, 0, 0, 0.25,
                            d(_lib.load().univs_cross_attention_workspace(4, 32, 1, 1)), d(4 * 16)],
                 "univs_cross_attention_f32: L=4 S=32 N=1 H=1 head_dim=16 not covered (head_dim == 32, S >= 32, with a mask S % 4 == 0, "
                 "N * H <= 65535, 16-byte aligned pointers)", id="univs_cross_attention_f32"),
    pytest.param("univs_cross_attention_flagged_f32",
                 lambda d: [d(4 * 16), d(32 * 16), d(32 * 16), d(4 * 32, U8), d(4, I32), 1, 4, 32, 1, 1, 16, 0, 0, 0, 0.25,
                            d(_lib.load().univs_cross_attention_workspace(4, 32, 1, 1)), d(4 * 16)],
                 "univs_cross_attention_f32: L=4 S=32 N=1 H=1 head_dim=16 not covered (head_dim == 32, S >= 32, with a mask S % 4 == 0, "
                 "N * H <= 65535, 16-byte aligned pointers)", id="univs_cross_attention_flagged_f32"),
    mlp("univs_mlp_presplit_f32", False), mlp("univs_mlp_presplit_v2_f32", True),
    pytest.param("univs_small_linear_presplit_f32",              # K = 16: K % 32 != 0
                 lambda d: [d(4 * 16), None, d(16 * 16), d(16), d(16), 16, 0, None, None, None, 1e-5, 4, 16, 16, 0, 0, 0, d(4 * 16)],
                 "univs_small_linear_presplit_f32: M=4 N=16 K=16 not covered (K % 32 == 0, N % 16 == 0, f_off % 4 == 0, with a LayerNorm "
                 "N == 256, M <= 1 048 560, 16-byte aligned pointers)", id="univs_small_linear_presplit_f32"),
    pytest.param("univs_small_mlp_presplit_f32",                 # out_T = 3 does not divide M = 4; one 256 -> 256 stage
                 lambda d: [d(4 * 256), 1, d.host(ctypes.c_void_p, [d(256 * 256)]), d.host(ctypes.c_void_p, [d(256)]),
                            d.host(ctypes.c_void_p, [d(256)]), d.host(ctypes.c_int, [0]), None, None, 1e-5, None, 4, 3, d(4 * 256)],
                 "univs_small_mlp_presplit_f32: M=4 not covered (M <= 1 048 560, out_T | M, 16-byte aligned pointers, x_normed / bias only "
                 "with a LayerNorm)", id="univs_small_mlp_presplit_f32"),
    pytest.param("univs_patch_embed4_f32",                       # E = 64
                 lambda d: [d(3 * 4 * 4), d(64 * 3 * 4 * 4), d(64), d(64), d(64), 1e-5, 1, 4, 4, 64, d(64)],
                 "univs_patch_embed4_f32: T=1 H=4 W=4 E=64 not covered (E in 96 / 128 / 192, H % 4, W % 4, 16-byte alignment)",
                 id="univs_patch_embed4_f32"),
    pytest.param("univs_decoder_memory_f32",                     # C = 6
                 lambda d: [d(6 * 4), d(6), d(4 * 6), d(6), 1, 6, 4, d(4 * 6), d(4 * 6)],
                 "univs_decoder_memory_f32: T=1 C=6 HW=4 not covered (C % 4, HW % 4, 16-byte alignment)", id="univs_decoder_memory_f32"),
    pytest.param("univs_transpose_f32", lambda d: [d(3 * 4), 1, 3, 4, d(3 * 4)],                       # R = 3
                 "univs_transpose_f32: R=3 C=4 B=1 not covered (R % 4, C % 4, strides % 4, B <= 65535, 16-byte alignment)",
                 id="univs_transpose_f32"),
    pytest.param("univs_transpose_ex_f32", lambda d: [d(4 * 6), 1, 4, 6, 0, None, d(4 * 6), 0, None, None],   # C = 6
                 "univs_transpose_f32: R=4 C=6 B=1 not covered (R % 4, C % 4, strides % 4, B <= 65535, 16-byte alignment)",
                 id="univs_transpose_ex_f32"),
    pytest.param("univs_normalize_pad_f32", lambda d: [d(MANY), d(1), d(1), MANY, 1, 1, 1, 1, 1, d(MANY)],
                 "univs_normalize_pad_f32: T * C = 65536 planes not covered (<= 65535)", id="univs_normalize_pad_f32"),
    pytest.param("univs_upsample2x_add_f32", lambda d: [d(2 * 3), d(4 * 6), None, d(4 * 6), 1, 2, 3],  # odd Win
                 "univs_upsample2x_add_f32: 2x3 not covered (Win even; in 8-byte, addend / out 16-byte aligned)", id="univs_upsample2x_add_f32"),
    pytest.param("univs_bilinear_pyramid3_f32", lambda d: [d(12 * 8), 1, 12, 8, d(6 * 4), d(3 * 2), d(1)],
                 "univs_bilinear_pyramid3_f32: 12x8 is not a multiple of 8 (or unaligned pointers)", id="univs_bilinear_pyramid3_f32"),
    layer_norm("univs_layer_norm_f32", False), layer_norm("univs_layer_norm_add_f32", True),
    pytest.param("univs_patch_merge_norm_f32", lambda d: [d(2 * 2 * 6), d(24), d(24), 1, 2, 2, 6, 1e-5, d(24)],
                 "univs_patch_merge_norm_f32: C=6 not supported (C % 4 == 0, C <= 768)", id="univs_patch_merge_norm_f32"),
    pytest.param("univs_proca_attention_f32", lambda d: [d(48), d(16), d(16), 1, 1, 1, 1, 16, 0.25, d(16)],     # head_dim 16
                 "univs_proca_attention_f32: shape not covered (head_dim == 32, 1 + L <= 16384)", id="univs_proca_attention_f32"),
    pytest.param("univs_prompt_draw",                            # 40 000 keys of 4 bytes: beyond the 150 KB of LDS
                 lambda d: [d(1, U8), d(1, I32), d(40000, U8), d(2, I32), d(1), d(40000), None, 1, 1, 1, 1, 40000, 1, d(1, I64), d(1, I64),
                            d(1, U8), d(2)],
                 "univs_prompt_draw: the keys of one entity do not fit the LDS (HW = 40000)", id="univs_prompt_draw"),
    pytest.param("univs_token_mean_f32", lambda d: [d(1028), None, 1, 1, 1, 1028, d(1028)],                      # C > 1024
                 "univs_token_mean_f32: shape not covered (C <= 1024, L <= 15360)", id="univs_token_mean_f32"),
    pytest.param("univs_mask_stats_f32", lambda d: [d(MANY), MANY, 1, 1, 1, 1, 1.0, -1.0, 0.0, d(MANY * 8, I32)],
                 "univs_mask_stats_f32: planes=65536 not covered (<= 65535)", id="univs_mask_stats_f32"),
    pytest.param("univs_mask_stats_strided_f32", lambda d: [d(MANY), 256, 256, 256, 1, 1, 1, 1, 1, 1.0, -1.0, 0.0, d(MANY * 8, I32)],
                 "univs_mask_stats_f32: planes=65536 not covered (<= 65535)", id="univs_mask_stats_strided_f32"),
    pytest.param("univs_msda_prepare_f32",                       # P = 2
                 lambda d: [d(6), 6, 4, d(2), 0, d.host(ctypes.c_int64, [1, 1]), 1, 1, 1, 1, 2, d(4), d(2)],
                 "univs_msda_prepare_f32: (L=1, P=2) not instantiated (P == 4, L <= 4)", id="univs_msda_prepare_f32"),
    msda_head_major("univs_msda_forward_strips_f32", 80, 16, False), msda_head_major("univs_msda_forward_heads_f32", 160, 16, False),
    msda_head_major("univs_msda_forward_strips_f32", 80, 32, True), msda_head_major("univs_msda_forward_heads_f32", 160, 32, True),
    pytest.param("univs_image_mask_stats_f32", lambda d: [d(MANY), MANY, 1, 1, 1, 1, 1, 1, d(MANY * 8, I32)],
                 "univs_image_mask_stats_f32: not covered (Q <= 65535)", id="univs_image_mask_stats_f32"),
    pytest.param("univs_image_panoptic_ids_f32",
                 lambda d: [d(1), 1, 1, 1, 1, 1, 1, 1, d(K_KEPT, I32), d(K_KEPT), K_KEPT, d(1, I32), d(K_KEPT * 3, I32)],
                 "univs_image_panoptic_ids_f32: not covered (K <= UNIVS_IMAGE_MAX_KEPT)", id="univs_image_panoptic_ids_f32"),
    pytest.param("univs_image_panoptic_paint_i32", lambda d: [d(1, I32), 1, 1, d(K_KEPT, I32), K_KEPT, 1, 1, d(1, I32), d(K_KEPT, I32)],
                 "univs_image_panoptic_paint_i32: not covered (K <= UNIVS_IMAGE_MAX_KEPT)", id="univs_image_panoptic_paint_i32"),
    pytest.param("univs_image_semseg_f32",                       # no selected plane (Qs = 0), one class more than 65535 chunks of 160
                 lambda d: [d(1), 1, 1, 1, 1, 1, 1, 1, None, None, 0, 65535 * 160 + 1, d(65535 * 160 + 1)],
                 "univs_image_semseg_f32: not covered (C <= 65535 * 160)", id="univs_image_semseg_f32"),
    pytest.param("univs_image_instance_masks_u8",
                 lambda d: [d(1), 1, 1, 1, 1, 1, 1, 1, d(MANY, I32), MANY, 1, 1, d(MANY, U8), d(MANY * 8, I32)],
                 "univs_image_instance_masks_u8: not covered (N <= 65535)", id="univs_image_instance_masks_u8"),
    pytest.param("univs_video_mask_stats_f32", lambda d: [d(1), 1, 1, 1, 1, 1, 1, 1, 1, d(MANY, I32), MANY, 1, d(MANY * 2, I32)],
                 "univs_video_mask_stats_f32: not covered (K <= 65535, sampled frames x crop < 2^31)", id="univs_video_mask_stats_f32"),
    pytest.param("univs_video_instance_masks_u8", lambda d: [d(1), 1, 1, 1, 1, 1, 1, 1, 1, d(MANY, I32), MANY, 1, 1, d(MANY, U8)],
                 "univs_video_instance_masks_u8: not covered (N V <= 65535)", id="univs_video_instance_masks_u8"),
    pytest.param("univs_video_panoptic_counts_i32",
                 lambda d: [d(1), 1, 1, 1, 1, 1, 1, 1, 1, d(K_KEPT, I32), K_KEPT, d(1, I32), 1, 1, d(K_KEPT * 3, I32)],
                 "univs_video_panoptic_counts_i32: not covered (K <= UNIVS_IMAGE_MAX_KEPT, V H0 W0 < 2^31)", id="univs_video_panoptic_counts_i32"),
    pytest.param("univs_panoptic_pair_counts",                   # G = 1025
                 lambda d: [d(1, I32), 0, d(1, I32), 0, 1, 1, 1, d(1025, I32), 1025, d(1, I32), 1, d(1026 * 2, I32), d(2, I32)],
                 "univs_panoptic_pair_counts: not covered (G, P <= 1024, (G + 1)(P + 1) <= 16384, T <= 65535, H W < 2^31, dword-aligned maps)",
                 id="univs_panoptic_pair_counts"),
    pytest.param("univs_vss_video_counts",                       # 129^2 cells
                 lambda d: [d(4, U8), d(4, U8), 1, 1, 1, 129, d(129 * 129, I32), d(4, I32), d(1, I32)],
                 "univs_vss_video_counts: not covered (num_classes^2 <= 16384, T <= 1024, T H W < 2^31 - 4, dword-aligned maps)",
                 id="univs_vss_video_counts"),
    pytest.param("univs_davis_counts",                           # G = 33
                 lambda d: [d(4, U8), d(4, U8), 1, 1, 1, 33, 1, 1, 0, d(33 * 2, I32), d(33, I32), d(1, I32), d(33 * 2, I32)],
                 "univs_davis_counts: not covered (G, P <= 32, radius <= 36, T H W < 2^31)", id="univs_davis_counts"),
]


@pytest.mark.parametrize("name, make_args, message", CASES)
def test_uncovered_shape_is_not_implemented_with_the_recorded_message(cuda, name, make_args, message):
    from univs_amd import ops
    lib = _lib.load()
    forced = message.endswith("forced (univs_msda_set_impl(1))")
    mem = Mem(cuda)
    args = make_args(mem)
    assert len(args) + 1 == len(_lib.SIGNATURES[name][1])
    impl = ops.get_config()["msda_impl"]
    if forced:
        ops.configure(msda_impl=1)
    try:
        rc = getattr(lib, name)(*args, torch.cuda.current_stream().cuda_stream)
        text = lib.univs_last_error().decode()
    finally:
        if forced:
            ops.configure(msda_impl=impl)
    torch.cuda.synchronize()
    assert (rc, text) == (_lib.ERR_NOT_IMPLEMENTED, message)
