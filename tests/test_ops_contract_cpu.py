"""The contract of the univs_amd.ops wrappers that can be pinned without a GPU: what each wrapper does with CPU tensors, the
argument checks that run before the device check, and -- with the library replaced by a stub that returns a chosen code -- what
each wrapper makes of OK / ERR_NOT_IMPLEMENTED / ERR_LAUNCH and which arguments it hands to the library.

One table (CASES) drives all three parts: a call of valid shape per public wrapper, what it does on CPU tensors ("raise": the
RuntimeError "Not implemented on the CPU"; "none": the caller keeps ATen; "aten": the wrapper itself falls back), and what it does with
ERR_NOT_IMPLEMENTED ("none" / "strict" = NotImplementedError / "aten").

Left out of the stub part: `presplit_weights` (it records a torch.cuda.Event on the stream; the wrappers that use it get a stand-in
here, the GPU suite covers the real one).  The settings functions (`configure`, `get_config`, `msda_set_impl`, ...) launch nothing
and are not in the table."""
import pytest
import torch

from univs_amd import _lib, ops
from univs_amd.switches import SWITCHES

SH, ST = [(4, 4), (2, 2)], [0, 16]          # two levels, 20 tokens
LN = 1e-5


def z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def ln(c, eps=LN):
    return (z(c), z(c), eps)


def _prompt_pre():
    return {"sel": z(1, 2, 8, 8, dtype=torch.bool), "rowcnt": z(1, 2, 8, dtype=torch.int32),
            "feat_masks_binary": z(1, 2, 2, 2, dtype=torch.bool), "counts": z(1, 4, dtype=torch.int32)}


I64, I32, B8 = torch.int64, torch.int32, torch.bool
LOW = ((8, 8), (6, 6))                       # padded, crop of the image_* / video_* wrappers

# name -> (call, on CPU tensors, on ERR_NOT_IMPLEMENTED, the library functions a covered call reaches, in order)
CASES = {
    "ms_deform_attn_forward": (lambda: ops.ms_deform_attn_forward(z(1, 20, 2, 32), SH, ST, z(1, 5, 2, 2, 4, 2), z(1, 5, 2, 2, 4)),
                               "raise", "strict", ["univs_msda_forward_f32"]),
    "ms_deform_attn_backward": (lambda: ops.ms_deform_attn_backward(z(1, 20, 2, 32), SH, ST, z(1, 5, 2, 2, 4, 2), z(1, 5, 2, 2, 4),
                                                                    z(1, 5, 64)), "raise", "strict", ["univs_msda_backward_f32"]),
    "msda_forward_heads": (lambda: ops.msda_forward_heads(z(1, 2, 20, 32), z(1, 2, 20, 24), z(1, 20, 2), SH, ST, 2),
                           "raise", "none", ["univs_msda_forward_heads_f32"]),
    "msda_forward_strips": (lambda: ops.msda_forward_strips(z(1, 4, 20, 16), z(1, 2, 20, 24), z(1, 20, 2), SH, ST, 2),
                            "raise", "none", ["univs_msda_forward_strips_f32"]),
    "msda_prepare": (lambda: ops.msda_prepare(z(1, 20, 48), 32, z(1, 20, 2, 2), SH, 2, 2, 4), "raise", "strict", ["univs_msda_prepare_f32"]),
    "presplit_weights": (lambda: ops.presplit_weights(z(8, 32)), "raise", None, None),
    "mlp_fused": (lambda: ops.mlp_fused(z(2048, 96), z(128, 96), z(128), z(96, 128), z(96), "relu", ln=ln(96), post_ln=ln(96, 1e-6),
                                        post_add=z(1024, 96)), "none", "none", ["univs_mlp_presplit_v2_f32"]),
    "small_linear": (lambda: ops.small_linear(z(4, 32), z(256, 32), z(256), x_add=z(4, 32), relu=True, residual=z(4, 256), ln=ln(256)),
                     "none", "none", ["univs_small_linear_presplit_f32"]),
    "small_mlp": (lambda: ops.small_mlp(z(4, 256), [(z(256, 256), z(256), True), (z(256, 256), None, False)], in_ln=ln(256), want_normed=True),
                  "none", "none", ["univs_small_mlp_presplit_f32"]),
    "linear_fused": (lambda: ops.linear_fused(z(2048, 128), z(8, 128), z(8), act="relu"), "none", "none", ["univs_linear_resident_presplit_f32"]),
    "linear_split": (lambda: ops.linear_split(z(2048, 128), z(8, 128), z(8), relu=True), "none", "none", ["univs_linear_resident_presplit_f32"]),
    "linear_blocked": (lambda: ops.linear_blocked(z(2, 8, 256), z(16, 256), z(16), 8, 8), "raise", "none", ["univs_linear_blocked_presplit_f32"]),
    "conv3x3": (lambda: ops.conv3x3(z(1, 4, 4, 4), z(8, 4, 3, 3)), "none", "none", ["univs_conv3x3_presplit_f32"]),
    "conv3x3_nhwc": (lambda: ops.conv3x3_nhwc(z(1, 4, 4, 4), z(8, 4, 3, 3)), "none", "none", ["univs_conv3x3_nhwc_presplit_f32"]),
    "conv1x1": (lambda: ops.conv1x1(z(1, 96, 64, 64), z(16, 96, 1, 1), z(16)), "none", "none", ["univs_conv1x1_presplit_f32"]),
    "patch_embed4": (lambda: ops.patch_embed4(z(1, 3, 8, 8), z(96, 3, 4, 4), z(96), ln=ln(96)), "none", "none", ["univs_patch_embed4_f32"]),
    "mask_decode": (lambda: ops.mask_decode(z(2, 3, 8), z(2, 8, 4, 4)), "raise", "strict", ["univs_mask_decode_f32"]),
    "mask_decode_attn": (lambda: ops.mask_decode_attn(z(2, 3, 8), z(2, 8, 4, 4)), "raise", "strict", ["univs_mask_decode_attn_f32"]),
    "mask_decode_attn[deferred]": (lambda: ops.mask_decode_attn(z(2, 3, 8), z(2, 8, 4, 4), deferred=True), "raise", "strict",
                                   ["univs_mask_decode_attn_deferred_f32"]),
    "window_attention": (lambda: ops.window_attention(z(2, 4, 3, 2, 8), z(2, 4, 4), z(2, 4, 4), 2, 0.5), "raise", "strict",
                         ["univs_window_attention_f32"]),
    "window_attention_image": (lambda: ops.window_attention_image(z(1, 4, 3, 2, 8), z(48), z(2, 4, 4), z(1, 4, 4), 2, 2, 2, 1, 0.5),
                               "raise", "strict", ["univs_window_attention_image_mma"]),
    "cross_attention": (lambda: ops.cross_attention(z(2, 1, 32), z(32, 1, 32), z(32, 1, 32), z(1, 2, 32, dtype=B8), 1, 0.1),
                        "none", "none", ["univs_cross_attention_workspace", "univs_cross_attention_flagged_f32"]),
    "masked_softmax_": (lambda: ops.masked_softmax_(z(1, 2, 3, 4), z(1, 3, 4, dtype=B8)), "raise", "strict", ["univs_masked_softmax_f32"]),
    "proca_attention": (lambda: ops.proca_attention(z(6, 192), z(2, 5, 3, 64), z(2, 5, 3, 64), 2), "raise", "none", ["univs_proca_attention_f32"]),
    "bilinear_pyramid3": (lambda: ops.bilinear_pyramid3(z(1, 8, 8)), "raise", "none", ["univs_bilinear_pyramid3_f32"]),
    "bilinear_resample": (lambda: ops.bilinear_resample(z(1, 4, 4), (8, 8), z(1, 8, 8)), "raise", "strict", ["univs_bilinear_resample_f32"]),
    "bilinear_crop_nearest": (lambda: ops.bilinear_crop_nearest(z(2, 3, 4, 4), (8, 8), (6, 6), (5, 5)), "raise", "none",
                              ["univs_bilinear_crop_nearest_f32"]),
    "normalize_pad": (lambda: ops.normalize_pad(z(2, 3, 4, 4), z(3), z(3), 8), "none", "none", ["univs_normalize_pad_f32"]),
    "group_norm": (lambda: ops.group_norm(z(1, 4, 2, 2), 2, z(4), z(4), relu=True), "raise", "strict", ["univs_group_norm_f32"]),
    "group_norm_affine": (lambda: ops.group_norm_affine(z(1, 4, 2, 2), 2, z(4), z(4)), "raise", "strict", ["univs_group_norm_affine_f32"]),
    "upsample2x_add": (lambda: ops.upsample2x_add(z(1, 2, 2), z(1, 4, 4), z(1, 2)), "none", "none", ["univs_upsample2x_add_f32"]),
    "layer_norm": (lambda: ops.layer_norm(z(2, 3, 8), z(8), z(8)), "raise", "strict", ["univs_layer_norm_f32"]),
    "layer_norm[post_add]": (lambda: ops.layer_norm(z(2, 3, 8), z(8), z(8), residual=z(2, 3, 8), post_add=z(1, 3, 8)), "raise", "strict",
                             ["univs_layer_norm_add_f32"]),
    "patch_merge_norm": (lambda: ops.patch_merge_norm(z(1, 4, 4, 4), z(16), z(16)), "none", "none", ["univs_patch_merge_norm_f32"]),
    "decoder_memory": (lambda: ops.decoder_memory(z(2, 4, 2, 2), z(4), z(4, 4), z(2, 4)), "none", "none", ["univs_decoder_memory_f32"]),
    "transpose_last2": (lambda: ops.transpose_last2(z(2, 3, 4)), "aten", "aten", ["univs_transpose_strided_f32"]),
    "tokens_from_nchw": (lambda: ops.tokens_from_nchw([z(1, 4, 2, 2), z(1, 4, 2, 2)], [z(4, 2), None], z(1, 8, 4)), "none", "none",
                         ["univs_transpose_ex_f32", "univs_transpose_ex_f32"]),
    "prompt_prefix": (lambda: ops.prompt_prefix(z(1, 2, 8, 8), z(1, 2, 4), 4), "raise", "strict", ["univs_prompt_prefix_f32"]),
    "prompt_draw": (lambda: ops.prompt_draw(_prompt_pre(), 2, z(2, 1), z(2, 4)), "raise", "none", ["univs_prompt_draw"]),
    "prompt_point_pe": (lambda: ops.prompt_point_pe(z(4, 2), z(2), z(8), z(16), 1.0, 2), "none", "strict", ["univs_prompt_point_pe_f32"]),
    "prompt_tokens": (lambda: ops.prompt_tokens(z(1, 4, 2, 2), z(1, 4, 2, 2), z(2, 4), z(2, 4), z(2, 3, dtype=I64), z(2, dtype=B8), z(2, dtype=B8),
                                                z(1, 2, 4), z(1, dtype=I64), 2), "raise", "strict", ["univs_prompt_tokens_f32"]),
    "token_mean": (lambda: ops.token_mean(z(2, 3, 2, 4), z(4)), "none", "none", ["univs_token_mean_f32"]),
    "mask_stats": (lambda: ops.mask_stats(z(2, 4, 4)), "raise", "none", ["univs_mask_stats_strided_f32"]),
    "image_mask_stats": (lambda: ops.image_mask_stats(z(2, 4, 4), *LOW), "raise", "none", ["univs_image_mask_stats_f32"]),
    "image_panoptic_ids": (lambda: ops.image_panoptic_ids(z(2, 4, 4), *LOW, z(2, dtype=I64), z(2)), "raise", "none", ["univs_image_panoptic_ids_f32"]),
    "image_panoptic_paint": (lambda: ops.image_panoptic_paint(z(6, 6, dtype=I32), z(2, dtype=I64), (5, 5)), "raise", "none",
                             ["univs_image_panoptic_paint_i32"]),
    "image_semseg": (lambda: ops.image_semseg(z(2, 4, 4), *LOW, z(2, dtype=I64), z(2, 3)), "raise", "none", ["univs_image_semseg_f32"]),
    "image_instance_masks": (lambda: ops.image_instance_masks(z(2, 4, 4), *LOW, z(2, dtype=I64), (5, 5)), "raise", "none",
                             ["univs_image_instance_masks_u8"]),
    "minvis_accumulate": (lambda: ops.minvis_accumulate(z(2, 3, 4, 4), z(2, 2, 4, 4), z(2, dtype=I64), 0), "raise", "strict",
                          ["univs_minvis_accumulate_f32"]),
    "video_mask_stats": (lambda: ops.video_mask_stats(z(2, 3, 4, 4), *LOW, z(2, dtype=I64), 1), "raise", "none", ["univs_video_mask_stats_f32"]),
    "video_instance_masks": (lambda: ops.video_instance_masks(z(2, 3, 4, 4), *LOW, z(2, dtype=I64), (5, 5)), "raise", "none",
                             ["univs_video_instance_masks_u8"]),
    "video_panoptic_ids": (lambda: ops.video_panoptic_ids(z(2, 3, 4, 4), *LOW, z(2, dtype=I64), z(2)), "raise", "none", ["univs_video_panoptic_ids_i32"]),
    "video_panoptic_counts": (lambda: ops.video_panoptic_counts(z(2, 3, 4, 4), *LOW, z(2, dtype=I64), z(3, 6, 6, dtype=I32), (5, 5)), "raise", "none",
                              ["univs_video_panoptic_counts_i32"]),
    "video_panoptic_paint": (lambda: ops.video_panoptic_paint(z(2, 3, 4, 4), *LOW, z(2, dtype=I64), z(3, 6, 6, dtype=I32), z(2, dtype=I64), (5, 5)),
                             "raise", "none", ["univs_video_panoptic_paint_i32"]),
}
STUBBED = [n for n, c in CASES.items() if c[3] is not None]


def test_the_table_names_every_public_launching_wrapper():
    """Every public function of ops.py that reaches a `univs_*` launch is in CASES (so a new wrapper has to state its contract here)."""
    import inspect
    not_launching = {"get_config", "configure", "configured", "msda_set_impl", "msda_last_impl", "msda_last_tiled_generation",
                     "mask_decode_set_impl", "mask_decode_last_impl", "needs_grad", "msda_level_order", "msda_pack_head_major",
                     "msda_pack_heads", "presplit_generation", "invalidate_presplit", "pad4_mask"}
    public = {n for n, f in vars(ops).items() if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith("_")}
    assert public - not_launching == {n.split("[")[0] for n in CASES}
    assert len(CASES) - len(STUBBED) <= len(CASES) // 4


@pytest.mark.parametrize("name", list(CASES))
def test_cpu_tensors(name):
    call, on_cpu = CASES[name][:2]
    with torch.no_grad():
        if on_cpu == "raise":
            with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
                call()
        elif on_cpu == "none":
            assert call() is None
        else:
            assert torch.equal(call(), z(2, 4, 3))       # transpose_last2: the ATen result


def test_cpu_refusal_text():
    """The sentence itself, in its three forms."""
    with pytest.raises(RuntimeError) as e:
        ops.mask_decode(z(2, 3, 8), z(2, 8, 4, 4))
    assert str(e.value) == "mask_decode: Not implemented on the CPU (tensor on cpu); the HIP extension is the only implementation"
    for call, name in ((lambda: ops.mask_stats(z(2, 4, 4)), "mask_stats"), (lambda: ops.image_semseg(z(2, 4, 4), *LOW, z(2), z(2, 3)), "image_semseg"),
                       (lambda: ops.image_panoptic_paint(z(6, 6, dtype=I32), z(2), (5, 5)), "image_panoptic_paint"),
                       (lambda: ops.bilinear_crop_nearest(z(2, 3, 4, 4), (8, 8), (6, 6), (5, 5)), "bilinear_crop_nearest")):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == f"{name}: Not implemented on the CPU (tensor on cpu); the HIP extension is the only implementation"
    with pytest.raises(RuntimeError) as e:
        CASES["minvis_accumulate"][0]()
    assert str(e.value) == "minvis_accumulate: Not implemented on the CPU (S on cpu); the HIP extension is the only implementation"
    with pytest.raises(RuntimeError) as e:
        CASES["prompt_tokens"][0]()
    assert str(e.value) == "prompt_tokens: Not implemented on the CPU; the HIP extension is the only implementation"
    with pytest.raises(RuntimeError) as e:
        ops.layer_norm(z(4, 8).t(), z(4), z(4).expand(2, 4)[0])            # (x is made contiguous; the parameters pass as they are)
    assert "Not implemented on the CPU" in str(e.value)


def test_checks_that_run_before_the_device_check():
    """Argument checks reachable with CPU tensors keep their messages (and their choice between raising and None)."""
    def raises(msg, f, exc=RuntimeError):
        with pytest.raises(exc) as e:
            f()
        assert str(e.value) == msg, str(e.value)
    w, x = z(128, 96), z(2048, 96)
    raises("mlp_fused: residual_normed needs ln and excludes residual", lambda: ops.mlp_fused(x, w, None, w.t(), None, "relu", residual_normed=True))
    raises("mlp_fused: dual needs post_ln and excludes post_add / residual_normed", lambda: ops.mlp_fused(x, w, None, w.t(), None, "gelu", dual=True))
    assert ops.mlp_fused(x, w, None, w.t(), None, "tanh") is None
    raises("linear_fused: unknown activation 'tanh'", lambda: ops.linear_fused(x, w, None, act="tanh"))
    raises("window_attention_image: mma='bf16' (one of ['f16', 'f16x3', 'f32'])",
           lambda: ops.window_attention_image(z(1, 4, 3, 2, 8), None, z(2, 4, 4), None, 2, 2, 2, 0, 0.5, mma="bf16"), ValueError)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ops.mask_stats(z(4))                                                             # (the device check comes before the rank check)
    assert ops.linear_blocked(z(2, 8, 256), z(16, 128), None, 8, 8) is None             # K mismatch: before the device check
    assert ops.linear_blocked(z(2, 8, 256, dtype=torch.float64), z(16, 256), None, 8, 8) is None
    xg = torch.zeros(4, 8, requires_grad=True)
    for f in (lambda: ops.layer_norm(xg, z(8), z(8)), lambda: ops.linear_blocked(xg, z(16, 8), None, 4, 8), lambda: ops.bilinear_resample(xg, (8, 8)),
              lambda: ops.group_norm(xg, 2, z(8), z(8)), lambda: ops.mask_decode(xg.view(1, 4, 8), z(1, 8, 2, 2))):
        with pytest.raises(RuntimeError, match="inference-only HIP operator called with gradient recording enabled"):
            f()
    assert ops.linear_fused(xg, z(8, 8)) is None and ops.mlp_fused(xg, w, None, w.t(), None, "relu") is None


# ---- the library replaced by a stub ---------------------------------------------------------------------------------------------------
class StubLib:
    """Every `univs_*` function returns `code` and records (name, args)."""

    def __init__(self, code):
        self.code, self.calls = code, []

    def __getattr__(self, name):
        if not name.startswith("univs_"):
            raise AttributeError(name)

        def fn(*args):
            if name == "univs_last_error":
                return b"stub"
            self.calls.append((name, args))
            return 64 if name == "univs_cross_attention_workspace" else self.code
        return fn


@pytest.fixture
def stub(monkeypatch):
    """`stub(code)` -> the StubLib now behind `_lib.load()`; CPU tensors pass for GPU tensors, the stream is the string "stream"."""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    monkeypatch.setattr(ops, "_stream_ptr", lambda t: "stream")
    monkeypatch.setattr(ops, "_raw_stream", lambda index: 0)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(ops, "presplit_weights", lambda w, conv=False, mode=None: (z(4, dtype=I32), z(4)))
    monkeypatch.setattr(ops, "_MASK_FLAGS", {})
    for k, v in (("presplit_kmin", 768), ("resident_presplit", True), ("linear_kmax", 4096)):
        monkeypatch.setattr(SWITCHES, k, v)

    def install(code):
        lib = StubLib(code)
        monkeypatch.setattr(_lib, "load", lambda: lib)
        return lib
    return install


def _abstract(args):
    """Pointers (integers no size in these calls reaches) -> "p"; None, small integers, floats and the stream as they are; ctypes
    objects by their type's name."""
    out = []
    for a in args:
        if a is None or isinstance(a, (float, str)):
            out.append(a)
        elif isinstance(a, int):
            out.append("p" if a >= 1 << 32 else a)
        else:
            out.append(type(a).__name__)
    return tuple(out)


@pytest.mark.parametrize("name", STUBBED)
def test_code_ok_returns_the_outputs(name, stub):
    lib = stub(_lib.OK)
    with torch.no_grad():
        out = CASES[name][0]()
    assert out is not None
    assert [c[0] for c in lib.calls] == CASES[name][3]
    assert all(c[1][-1] == "stream" for c in lib.calls if c[0] != "univs_cross_attention_workspace")      # the stream is the last argument


@pytest.mark.parametrize("name", STUBBED)
def test_code_not_implemented(name, stub):
    lib = stub(_lib.ERR_NOT_IMPLEMENTED)
    call, _, uncovered, symbols = CASES[name]
    with torch.no_grad():
        if uncovered == "strict":
            with pytest.raises(NotImplementedError, match=f"^{name.split('[')[0]}: stub" if name != "prompt_tokens" else None):
                call()
        elif uncovered == "none":
            assert call() is None
        else:
            assert torch.equal(call(), z(2, 4, 3))
    got = [c[0] for c in lib.calls]
    if name in ("linear_fused", "linear_split"):
        assert got == ["univs_linear_resident_presplit_f32", "univs_linear_fused_f32"]      # the chain goes on to the next kernel
    else:
        assert got == symbols[:len(got)] and len(got) >= len(symbols) - 1                   # (tokens_from_nchw stops at the first level)


@pytest.mark.parametrize("name", STUBBED)
def test_code_launch_error_names_the_wrapper(name, stub):
    stub(_lib.ERR_LAUNCH)
    reported = {"linear_split": "linear_fused"}.get(name, name.split("[")[0])
    with torch.no_grad(), pytest.raises(_lib.UnivsHipError, match=rf"^{reported} failed \(code -3\): stub$"):
        CASES[name][0]()


def test_deferred_mask_materialize_is_strict(stub):
    lib = stub(_lib.OK)
    dm = CASES["mask_decode_attn[deferred]"][0]()
    assert isinstance(dm, ops.DeferredMask) and dm.gen == 1
    assert dm.materialize().dtype == torch.bool and lib.calls[-1][0] == "univs_attn_mask_rows_reset"
    assert _abstract(lib.calls[-1][1]) == ("p", "p", 1, 6, 16, "stream")
    dm2 = CASES["mask_decode_attn[deferred]"][0]()
    stub(_lib.ERR_NOT_IMPLEMENTED)
    with pytest.raises(NotImplementedError, match="^attn_mask_rows_reset: stub"):
        dm2.materialize()


def test_linear_fused_chain_order(stub):
    """streamed -> W-resident on the split image -> W-resident, each tried only when the one before does not cover the call."""
    lib = stub(_lib.ERR_NOT_IMPLEMENTED)
    assert ops.linear_fused(z(2048, 768), z(8, 768), z(8), residual=z(2048, 8)) is None
    assert [c[0] for c in lib.calls] == ["univs_linear_presplit_f32", "univs_linear_resident_presplit_f32", "univs_linear_fused_f32"]
    assert [_abstract(c[1]) for c in lib.calls] == [("p", "p", "p", "p", "p", 2048, 8, 768, 0, "p", "stream")] * 2 + \
        [("p", "p", "p", "p", 2048, 8, 768, 0, "p", "stream")]
    lib = stub(_lib.OK)
    assert tuple(ops.linear_fused(z(2, 1024, 768), z(8, 768)).shape) == (2, 1024, 8)
    assert [c[0] for c in lib.calls] == ["univs_linear_presplit_f32"]
    assert _abstract(lib.calls[0][1]) == ("p", "p", "p", None, None, 2048, 8, 768, 0, "p", "stream")
    lib = stub(_lib.OK)
    view = z(16, 128)[:8]                                    # a view of a parameter: not split per tensor, the plain W-resident kernel
    assert ops.linear_fused(z(2048, 128), view, act="gelu") is not None
    assert [(c[0], _abstract(c[1])) for c in lib.calls] == [("univs_linear_fused_f32", ("p", "p", None, None, 2048, 8, 128, 2, "p", "stream"))]
    lib = stub(_lib.OK)
    assert ops.linear_blocked(z(16, 256), view.new_zeros(16, 256)[:8], None, 8, 8) is not None
    assert [(c[0], _abstract(c[1])) for c in lib.calls] == [("univs_linear_blocked_f32", ("p", "p", None, 16, 8, 256, 8, 8, "p", "stream"))]


# recorded on the commit before the wrappers were moved onto the shared helpers: the arguments each call hands to the library
RECORDED = {
    "mlp_fused": [("p", "p", "p", "p", "p", "p", "p", None, 0, "p", "p", 1e-5, "p", "p", 1e-6, "p", 1024, "p", 2048, 96, 128, 1, "p", "stream")],
    "small_linear": [("p", "p", "p", "p", "p", 256, 0, "p", "p", "p", 1e-5, 4, 256, 32, 1, 0, 0, "p", "stream")],
    "small_mlp": [("p", 2, "c_void_p_Array_3", "c_void_p_Array_3", "c_void_p_Array_3", "c_int_Array_3", "p", "p", 1e-5, "p", 4, 0, "p", "stream")],
    "layer_norm": [("p", None, "p", "p", 6, 8, 1e-5, None, "p", "stream")],
    "layer_norm[post_add]": [("p", "p", "p", "p", "p", 3, 6, 8, 1e-5, None, "p", "p", "stream")],
    "linear_fused": [("p", "p", "p", "p", None, 2048, 8, 128, 1, "p", "stream")],
    "linear_blocked": [("p", "p", "p", "p", 16, 16, 256, 8, 8, "p", "stream")],
    "patch_embed4": [("p", "p", "p", "p", "p", 1e-5, 1, 8, 8, 96, "p", "stream")],
    "conv1x1": [("p", "p", "p", "p", 1, 96, 16, 64, 64, "p", "stream")],
    "cross_attention": [(2, 32, 1, 1), ("p", "p", "p", "p", None, 0, 2, 32, 1, 1, 32, 32, 32, 32, 0.1, "p", "p", "stream")],
    "window_attention": [("p", "p", "p", 2, 2, 4, 2, 8, 0.5, "p", "stream")],
    "window_attention_image": [("p", "p", "p", "p", 1, 2, 2, 2, 1, 2, 8, 0.5, 0, "p", "stream")],
    "bilinear_resample": [("p", "p", "p", 1, 4, 4, 8, 8, "stream")],
    "upsample2x_add": [("p", "p", "p", "p", 1, 2, 2, "stream")],
    "token_mean": [("p", "p", 2, 3, 2, 4, "p", "stream")],
    "tokens_from_nchw": [("p", 1, 4, 4, 0, "p", "p", 32, "p", "p", "stream"), ("p", 1, 4, 4, 0, None, "p", 32, "p", "p", "stream")],
    "msda_forward_heads": [("p", "c_long_Array_4", "c_long_Array_2", "p", "p", 0, 1, 20, 2, 32, 2, 20, 4, "p", "stream")],
    "msda_forward_strips": [("p", "c_long_Array_4", "c_long_Array_2", "p", "p", 0, 1, 20, 2, 32, 2, 20, 4, "p", "stream")],
    "group_norm": [("p", "p", "p", 1, 4, 4, 2, 1e-5, 1, "p", 8, "p", "stream")],
    "group_norm_affine": [("p", "p", "p", 1, 4, 4, 2, 1e-5, "p", 8, "p", "stream")],
    "conv3x3": [("p", "p", "p", 1, 4, 8, 4, 4, "p", "stream")],
    "conv3x3_nhwc": [("p", "p", "p", 1, 4, 8, 4, 4, "p", "stream")],
    "mask_decode_attn[deferred]": [("p", "p", 2, 3, 8, 16, "p", "p", 1, "stream")],
    "image_semseg": [("p", 2, 4, 4, 8, 8, 6, 6, "p", "p", 2, 3, "p", "stream")],
    "minvis_accumulate": [("p", 2, 3, 4, 4, "p", 2, 2, "p", 0, "stream")],
}


@pytest.mark.parametrize("name", list(RECORDED))
def test_arguments_handed_to_the_library(name, stub):
    lib = stub(_lib.OK)
    with torch.no_grad():
        CASES[name][0]()
    assert [_abstract(c[1]) for c in lib.calls] == RECORDED[name]


def test_optional_pointers_stay_null(stub):
    """The same wrappers without their optional operands: NULL in exactly those positions."""
    lib = stub(_lib.OK)
    with torch.no_grad():
        ops.mlp_fused(z(2048, 96), z(128, 96), None, z(96, 128), None, "gelu", residual=z(2048, 96))
        ops.mlp_fused(z(2048, 96), z(128, 96), z(128), z(96, 128), z(96), "relu", ln=ln(96), post_ln=(z(96), None, 1e-6), dual=True)
        ops.mlp_fused(z(2048, 96), z(128, 96), z(128), z(96, 128), z(96), "relu", ln=(z(96), None, LN), residual_normed=True)
        ops.small_linear(z(3, 4, 32), z(64, 32), None, rows=(16, 32), add_features=32, x_add=z(3, 4, 32), transpose01=True)
        ops.small_mlp(z(3, 4, 256), [(z(256, 256), None, False)], transpose01=True)
        ops.layer_norm(z(6, 8), z(8), z(8), residual=z(6, 8), return_sum=True)
        ops.patch_embed4(z(1, 3, 8, 8), z(96, 3, 4, 4))
        ops.window_attention(z(2, 4, 3, 2, 8), z(2, 4, 4), None, 2, 0.5)
        ops.window_attention_image(z(1, 4, 3, 2, 8), None, z(2, 4, 4), z(1, 4, 4), 2, 2, 2, 0, 0.5, mma="f16x3")
        ops.cross_attention(z(2, 1, 32), z(32, 1, 32), z(32, 1, 32), None, 1, 0.1)
        ops.token_mean(z(2, 3, 2, 4))
        ops.tokens_from_nchw([z(1, 4, 2, 2)], [None], None)
    got = [_abstract(c[1]) for c in lib.calls if c[0] != "univs_cross_attention_workspace"]
    assert got == [
        ("p", "p", "p", None, "p", "p", None, "p", 0, None, None, 0.0, None, None, 0.0, None, 0, None, 2048, 96, 128, 2, "p", "stream"),
        ("p", "p", "p", "p", "p", "p", "p", None, 2, "p", "p", 1e-5, "p", None, 1e-6, None, 0, "p", 2048, 96, 128, 1, "p", "stream"),
        ("p", "p", "p", "p", "p", "p", "p", None, 1, "p", None, 1e-5, None, None, 0.0, None, 0, None, 2048, 96, 128, 1, "p", "stream"),
        ("p", "p", "p", "p", None, 64, 16, None, None, None, 0.0, 12, 32, 32, 0, 32, 4, "p", "stream"),
        ("p", 1, "c_void_p_Array_3", "c_void_p_Array_3", "c_void_p_Array_3", "c_int_Array_3", None, None, 0.0, None, 12, 4, "p", "stream"),
        ("p", "p", "p", "p", 6, 8, 1e-5, "p", "p", "stream"),
        ("p", "p", None, None, None, 0.0, 1, 8, 8, 96, "p", "stream"),
        ("p", "p", None, 2, 2, 4, 2, 8, 0.5, "p", "stream"),
        ("p", None, "p", None, 1, 2, 2, 2, 0, 2, 8, 0.5, 2, "p", "stream"),
        ("p", "p", "p", None, None, 0, 2, 32, 1, 1, 32, 32, 32, 32, 0.1, "p", "p", "stream"),
        ("p", None, 2, 3, 2, 4, "p", "stream"),
        ("p", 1, 4, 4, 0, None, "p", 16, None, None, "stream"),
    ]


def test_layer_norm_triples(stub):
    """`ln` = (weight, bias, eps): weight mandatory, both contiguous float32 [C] on the GPU.  mlp_fused raises; small_linear and small_mlp
    hand the call back (None: the caller keeps the separate launches)."""
    lib = stub(_lib.OK)
    x, w1, w2 = z(2048, 96), z(128, 96), z(96, 128)
    bad = [(z(96, dtype=torch.float64), None, LN), (z(95), None, LN), (z(96), z(192)[::2], LN)]
    msg = "mlp_fused: LayerNorm weight / bias must be contiguous float32 \\[C\\] on the GPU"
    with torch.no_grad():
        for t in bad:
            with pytest.raises(RuntimeError, match=msg):
                ops.mlp_fused(x, w1, None, w2, None, "relu", ln=t)
            with pytest.raises(RuntimeError, match=msg):
                ops.mlp_fused(x, w1, None, w2, None, "relu", post_ln=t)
        with pytest.raises(RuntimeError, match="^mlp_fused: ln needs a weight$"):
            ops.mlp_fused(x, w1, None, w2, None, "relu", ln=(None, z(96), LN))
        with pytest.raises(RuntimeError, match="^mlp_fused: post_ln needs a weight$"):
            ops.mlp_fused(x, w1, None, w2, None, "relu", post_ln=(None, z(96), LN))
        with pytest.raises(RuntimeError, match="^mlp_fused: post_add needs post_ln$"):
            ops.mlp_fused(x, w1, None, w2, None, "relu", post_add=x)
        for t in [(z(256, dtype=torch.float64), None, LN), (z(255), None, LN), (z(256), z(512)[::2], LN), (None, z(256), LN)]:
            assert ops.small_linear(z(4, 32), z(256, 32), None, ln=t) is None
            assert ops.small_mlp(z(4, 256), [(z(256, 256), None, False)], in_ln=t) is None
    assert lib.calls == []


def test_messages_behind_the_device_check(stub):
    """The shape / dtype checks that follow the device check, reached with the device check stubbed: texts, and raise against None."""
    lib = stub(_lib.OK)
    f64 = torch.float64

    def raises(msg, f):
        with pytest.raises(RuntimeError) as e:
            f()
        assert str(e.value) == msg, str(e.value)
    with torch.no_grad():
        for name, v in (("msda_forward_heads", z(1, 2, 20, 32)), ("msda_forward_strips", z(1, 4, 20, 16))):
            f = getattr(ops, name)
            raises(f"{name}: inconsistent shapes", lambda: f(v, z(1, 2, 20, 25), z(1, 20, 2), SH, ST, 2))
            raises(f"{name}: inconsistent shapes", lambda: f(v.transpose(1, 3).contiguous(), z(1, 2, 20, 24), z(1, 20, 2), SH, ST, 2))
            raises(f"{name}: inconsistent shapes", lambda: f(v, z(1, 2, 20, 24), z(3, 20, 2), SH, ST, 2))
            raises(f"{name}: contiguous float32 operands only", lambda: f(v.double(), z(1, 2, 20, 24), z(1, 20, 2), SH, ST, 2))
            raises(f"{name}: all tensors have to be contiguous", lambda: f(v, z(1, 2, 20, 48)[..., ::2], z(1, 20, 2), SH, ST, 2))
            assert f(v, z(1, 2, 20, 48), z(1, 20, 2), SH, ST, 2, num_points=8) is None           # eight points: no kernel
        raises("ms_deform_attn_backward: float32 only",
               lambda: ops.ms_deform_attn_backward(z(1, 20, 2, 32, dtype=f64), SH, ST, z(1, 5, 2, 2, 4, 2), z(1, 5, 2, 2, 4), z(1, 5, 64)))
        raises("ms_deform_attn_backward: inconsistent shapes",
               lambda: ops.ms_deform_attn_backward(z(1, 20, 2, 32), SH, ST, z(1, 5, 2, 2, 4, 2), z(1, 5, 2, 2, 4), z(1, 5, 63)))
        raises("mask_decode: float32 only", lambda: ops.mask_decode(z(2, 3, 8, dtype=f64), z(2, 8, 4, 4)))
        raises("mask_decode_attn: shape mismatch", lambda: ops.mask_decode_attn(z(2, 3, 8), z(2, 7, 4, 4)))
        raises("layer_norm: weight / bias must be [C]", lambda: ops.layer_norm(z(2, 8), z(8), z(7)))
        raises("layer_norm: return_sum needs a residual", lambda: ops.layer_norm(z(2, 8), z(8), z(8), return_sum=True))
        raises("layer_norm: post_add needs a residual and excludes return_sum", lambda: ops.layer_norm(z(2, 8), z(8), z(8), post_add=z(2, 8)))
        raises("group_norm: bad channel / group / parameter shapes", lambda: ops.group_norm(z(1, 4, 2, 2), 3, z(4), z(4)))
        raises("group_norm_affine: bad channel / group / parameter shapes", lambda: ops.group_norm_affine(z(1, 4, 2, 2), 2, z(4), z(5)))
        raises("group_norm: float32 [N, C, ...] only", lambda: ops.group_norm(z(1, 4, 2, 2, dtype=f64), 2, z(4), z(4)))
        raises("group_norm_affine: float32 [N, C, ...] only", lambda: ops.group_norm_affine(z(4), 2, z(4), z(4)))
        raises("group_norm: all tensors have to be contiguous", lambda: ops.group_norm(z(1, 4, 2, 2), 2, z(8)[::2], z(4)))
        raises("mask_stats: float32 [..., H, W] only", lambda: ops.mask_stats(z(4)))
        raises("image_mask_stats: float32 [Q, h, w] logits only", lambda: ops.image_mask_stats(z(2, 4, 4, dtype=f64), *LOW))
        raises("video_mask_stats: float32 [Q, V, h, w] mask logits only", lambda: ops.video_mask_stats(z(2, 4, 4), *LOW, z(2), 1))
        raises("image_panoptic_paint: int32 [hi, wi] ids only", lambda: ops.image_panoptic_paint(z(6, 6), z(2), (5, 5)))
        raises("linear_fused: bias must be float32 [N] on the GPU", lambda: ops.linear_fused(z(2048, 128), z(8, 128), z(9)))
        raises("mlp_fused: biases must be contiguous float32 [Hd] / [C] on the GPU",
               lambda: ops.mlp_fused(z(2048, 96), z(128, 96), z(127), z(96, 128), None, "relu"))
        raises("patch_merge_norm: weight / bias must be [4 C]", lambda: ops.patch_merge_norm(z(1, 4, 4, 4), z(16), z(15)))
    assert lib.calls == []
