"""GPU: the seams folded into their consumers (include/univs_fused_hip.h, univs_amd/fused_ops.py) against the separate launches they
replace.  Every seam is an exact refactoring -- the same operations on the same values in the same order -- so every comparison is
`torch.equal`.

  A  GroupNorm + ReLU of the FPN output applied by the mask-feature 1 x 1 convolution while it loads its operand
  B  the attention core's merge of its key segments inside the out-projection (few-rows Linear, residual + LayerNorm) behind it
  C  Swin stage outputs as channels-last views of the token tensors, read in place by the pixel decoder's 1 x 1 convolutions

Shapes: H x W = 41 x 51 (HW = 2091 is no multiple of the 32-row tile, so a tile straddles the frame seam, the workgroup whose 256 rows
cross it stages the pairs of two frames, and the last tile is partial), T = 2 (M = 4182 >= 4096, the kernel's lower bound)."""
import pytest
import torch

from tests import cases, helpers
from univs_amd import fused_ops, ops
from univs_amd.switches import override

pytestmark = pytest.mark.gpu

T, H, W = 2, 41, 51


def _randn(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _conv_params(seed, cin, cout, cuda):
    return (_randn(seed, cout, cin, 1, 1) / cin ** 0.5).to(cuda), _randn(seed + 1, cout).to(cuda)


# ---- A, operator

def _gn_params(seed, c, cuda):
    return (1.0 + 0.2 * _randn(seed, c)).to(cuda), (0.1 * _randn(seed + 1, c)).to(cuda)


def _x_plain(cin):
    return _randn(3, T, cin, H, W)


def _x_constant_group(cin):
    x = _randn(4, T, cin, H, W)
    cg = cin // 32
    x[1, 2 * cg:3 * cg] = 0.75                      # every value of one group of frame 1 is the same: variance 0
    return x


def _x_mostly_negative(cin):
    x = _randn(5, T, cin, H, W) - 2.0               # ~98 % of the raw values are negative; after the normalisation about half are
    x[:, ::3] *= 0.01                               # every third plane: a narrow spread around a large offset
    return x


@pytest.mark.parametrize("cin,cout,make_x", [(256, 256, _x_plain), (128, 48, _x_plain), (256, 256, _x_constant_group),
                                             (256, 256, _x_mostly_negative)],
                         ids=["256to256", "128to48_short_last_pass", "constant_group", "mostly_negative"])
def test_norm_relu_folded_into_the_conv_operand_is_the_materialised_path(cuda, cin, cout, make_x):
    x = make_x(cin).to(cuda)
    w, b = _conv_params(11, cin, cout, cuda)
    gamma, beta = _gn_params(21, cin, cuda)
    if make_x is _x_mostly_negative:
        beta = beta - 1.0                           # most normalised values below zero: the ReLU decides most of the operand
    normed = ops.group_norm(x, 32, gamma, beta, 1e-5, relu=True)
    ref = ops.conv1x1(normed, w, b)
    assert ref is not None
    affine = ops.group_norm_affine(x, 32, gamma, beta, 1e-5)
    got = fused_ops.conv1x1_fused(x, w, b, affine)
    assert got is not None and got.is_contiguous() and tuple(got.shape) == (T, cout, H, W)
    assert torch.equal(got, ref)
    if make_x is _x_mostly_negative:
        assert (normed == 0).float().mean().item() > 0.6
    # the same on the channels-last operand (the pairs are those of the NCHW tensor)
    x_cl = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not x_cl.is_contiguous()
    got_cl = fused_ops.conv1x1_fused(x_cl, w, b, affine)
    assert got_cl is not None and torch.equal(got_cl, ref)


# ---- B, operator.  (Fully masked rows are NaN on both sides: compared as bits, which is torch.equal and stricter.)

def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _attention_case(L, S, N, Hh, mask2d, cuda):
    E = 32 * Hh
    q, k, v = (_randn(50 + i, n, N, E).to(cuda) for i, n in enumerate((L, S, S)))
    if mask2d:
        m = _randn(53, 1, L, S) > 0.25                           # 60 % masked
        m[:, 3::7] = True                                        # fully masked rows
        m[:, 1::5, : S // 2] = True                              # whole key segments masked for some queries
    else:
        m = _randn(53, N, L, S) > 0.25
        m[:, 1::5, : S // 2] = True
    w = (_randn(54, E, E) / E ** 0.5).to(cuda)
    b = _randn(55, E).to(cuda)
    res = _randn(56, L, N, E).to(cuda)
    ln = ((1.0 + 0.2 * _randn(57, E)).to(cuda), (0.1 * _randn(58, E)).to(cuda), 1e-5)
    return q, k, v, m.to(cuda), w, b, res, ln


@pytest.mark.parametrize("L,S,N,mask2d,forced", [(100, 920, 5, False, 0), (100, 920, 5, False, 8 + 65536 * 7), (500, 500, 1, True, 0)],
                         ids=["100x920x5_own_plan", "100x920x5_8seg_7qb_Lp112", "500x500x1_mask2d_last_workgroup_of_4"])
def test_merge_inside_the_out_projection_is_merge_then_projection(cuda, L, S, N, mask2d, forced):
    Hh = 8
    q, k, v, m, w, b, res, ln = _attention_case(L, S, N, Hh, mask2d, cuda)
    scale = 32 ** -0.5
    with ops.configured(xattn_segments=forced):
        out = ops.cross_attention(q, k, v, m, Hh, scale)
        assert out is not None
        ref_plain = ops.small_linear(out, w, b)
        ref_tail = ops.small_linear(out, w, b, residual=res, ln=ln)
        got_plain = fused_ops.attention_out_proj(q, k, v, m, Hh, scale, w, b)
        got_tail = fused_ops.attention_out_proj(q, k, v, m, Hh, scale, w, b, residual=res, ln=ln)
    assert ref_plain is not None and ref_tail is not None and got_plain is not None and got_tail is not None
    assert _same_bits(got_plain, ref_plain)
    assert _same_bits(got_tail, ref_tail)
    if mask2d:
        assert torch.isnan(out[3]).all() and not torch.isnan(out[0]).any()      # the fully masked rows are there


def test_attention_layers_with_the_merge_folded_are_the_switch_off_layers(cuda):
    """One CrossAttentionLayer + SelfAttentionLayer on Q' = 20 queries, T = 2 frames, 23 x 40 keys."""
    from univs_amd.modeling.transformer_decoder.transformer_layers import CrossAttentionLayer, SelfAttentionLayer
    torch.manual_seed(0)
    ca = CrossAttentionLayer(d_model=256, nhead=8, dropout=0.0, normalize_before=False).to(cuda).eval()
    sa = SelfAttentionLayer(d_model=256, nhead=8, dropout=0.0, normalize_before=False).to(cuda).eval()
    Q, Tn, S = 20, 2, 23 * 40
    tgt, qpos = _randn(60, Q, Tn, 256).to(cuda), _randn(61, Q, Tn, 256).to(cuda)
    mem, mpos = _randn(62, S, Tn, 256).to(cuda), _randn(63, S, Tn, 256).to(cuda)
    mask = (_randn(64, Tn, Q, S) > 0.25).to(cuda)

    def run():
        with torch.no_grad():
            x = ca(tgt, mem, memory_mask=mask, memory_key_padding_mask=None, pos=mpos, query_pos=qpos)
            y = sa(x.reshape(Q * Tn, 1, 256), tgt_mask=None, tgt_key_padding_mask=None, query_pos=qpos.reshape(Q * Tn, 1, 256))
        return x, y
    with override(fold_attn_merge=False):
        ref = run()
    with override(fold_attn_merge=True):
        got = run()
    assert _same_bits(got[0], ref[0]) and _same_bits(got[1], ref[1])


# ---- C, operator

@pytest.mark.parametrize("cin", [96, 192, 768])
def test_channels_last_conv1x1_is_the_nchw_conv1x1(cuda, cin):
    tokens = _randn(7, T, H * W, cin).to(cuda)                     # what a Swin stage hands on
    view = tokens.view(T, H, W, cin).permute(0, 3, 1, 2)
    w, b = _conv_params(13, cin, 256, cuda)
    ref = ops.conv1x1(view.contiguous(), w, b)
    assert ref is not None
    got = fused_ops.conv1x1_fused(view, w, b)
    assert got is not None and got.is_contiguous() and torch.equal(got, ref)
    assert torch.equal(fused_ops.conv1x1_fused(view.contiguous(), w, None), ops.conv1x1(view.contiguous(), w, None))


def test_uncovered_and_strided_operands_answer_none(cuda):
    w, b = _conv_params(13, 96, 256, cuda)
    small = _randn(8, 2, 96, 8, 8).to(cuda)                        # 128 pixels < 4096
    assert fused_ops.conv1x1_fused(small, w, b) is None
    x = _randn(9, T, 96, H, 2 * W).to(cuda)[..., ::2]              # neither layout: never copied behind the caller's back
    assert fused_ops.conv1x1_fused(x, w, b) is None
    tiny_hw = _randn(10, 32, 256, 12, 12).to(cuda)                 # H W = 144 < 256 with the affine: three frames in one round
    w2, b2 = _conv_params(13, 256, 256, cuda)
    gamma, beta = _gn_params(21, 256, cuda)
    assert fused_ops.conv1x1_fused(tiny_hw, w2, b2, ops.group_norm_affine(tiny_hw, 32, gamma, beta)) is None
    assert fused_ops.conv1x1_fused(tiny_hw, w2, b2) is not None


# ---- modules.  Feature sizes: res2 96 x 128 and res3 48 x 64 are covered by the kernels (>= 4096 pixels at T = 2), res4 24 x 32 and
# res5 12 x 16 are not and take the LDS tile transpose + the library convolution: both routes in one pass.

@pytest.fixture(scope="module")
def pixel_decoder(cuda):
    return helpers.build_pixel_decoder(cases.SWINT_SHAPES, cuda)


@pytest.fixture(scope="module")
def swin_features(cuda):
    """(NCHW-contiguous features, the same values as channels-last views of token tensors)"""
    nchw, views = {}, {}
    for i, (k, (c, s)) in enumerate(cases.SWINT_SHAPES.items()):
        h, w = 384 // s, 512 // s
        tokens = _randn(30 + i, 2, h * w, c).to(cuda)
        views[k] = tokens.view(2, h, w, c).permute(0, 3, 1, 2)
        nchw[k] = views[k].contiguous()
    return nchw, views


def _flat(res):
    mf, bfe, enc0, ms = res
    return [mf, bfe, enc0, *ms]


@pytest.fixture(scope="module")
def pixel_decoder_reference(pixel_decoder, swin_features):
    with torch.no_grad(), override(fold_fpn_norm=False, swin_channels_last=False):
        return _flat(pixel_decoder.forward_features(swin_features[0]))


def test_pixel_decoder_with_the_norm_folded_is_the_switch_off_result(pixel_decoder, swin_features, pixel_decoder_reference):
    ref = pixel_decoder_reference
    with torch.no_grad():
        with override(fold_fpn_norm=True):
            plain = _flat(pixel_decoder.forward_features(swin_features[0]))       # called as ever: the materialised tensor is there
            with pixel_decoder.normed_optional():
                lean = _flat(pixel_decoder.forward_features(swin_features[0]))
        with override(fold_fpn_norm=False), pixel_decoder.normed_optional():
            off = _flat(pixel_decoder.forward_features(swin_features[0]))
    assert lean[1] is None and plain[1] is not None and off[1] is not None
    assert torch.equal(plain[1], ref[1]) and torch.equal(off[1], ref[1])
    for k in (0, 2, 3, 4, 5):
        assert torch.equal(lean[k], ref[k]), k
        assert torch.equal(plain[k], ref[k]) and torch.equal(off[k], ref[k]), k


def test_pixel_decoder_on_channels_last_views_is_the_nchw_result(pixel_decoder, swin_features, pixel_decoder_reference):
    ref = pixel_decoder_reference
    with torch.no_grad():
        got = _flat(pixel_decoder.forward_features(swin_features[1]))
    for k in range(6):
        assert got[k].is_contiguous() and torch.equal(got[k], ref[k]), k


def test_swin_stage_outputs_are_views_of_the_tokens(cuda):
    swin = helpers.build_swin(cuda)
    x = _randn(40, 2, 3, 128, 160).to(cuda)
    with torch.no_grad():
        with override(swin_channels_last=False):
            ref = swin(x)
        with override(swin_channels_last=True):
            got = swin(x)
    assert sorted(got) == sorted(ref) == ["res2", "res3", "res4", "res5"]
    for k in ref:
        assert ref[k].is_contiguous()
        assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k]), k
        base = got[k]._base
        assert base is not None and got[k].untyped_storage().data_ptr() == base.untyped_storage().data_ptr(), k   # a view: no copy
        assert got[k].permute(0, 2, 3, 1).is_contiguous(), k
