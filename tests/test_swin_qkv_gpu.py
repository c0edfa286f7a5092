"""GPU: Swin window attention that computes q, k, v from the tokens itself (swin_ops.window_attention_qkv, csrc/window_attn_qkv.hip) against
the two launches it replaces.

identity   torch.equal with `ops.window_attention_image(ops.linear_fused(x, W, b).view(B, L, 3, nH, 32), b, bias, mask, H, W, 7, shift,
           scale, mma="f16x3")` -- the existing path, never the code under test -- at (B, H, W, shift, C, nH), all >= 2048 tokens (below
           that `ops.linear_fused` declines):
             (2, 30, 45, 0, 96, 3)    (3, 30, 45, 3, 192, 6)    (1, 46, 47, 3, 96, 3): padding on both axes, windows that wrap
             (3, 23, 40, 3, 192, 6)   (1, 189, 189, 3, 96, 3): 729 windows, more than one round of the persistent loop at 256 CUs
           each with and without a qkv bias.  The inputs (made once per shape, left unchanged) hold ordinary normal rows, a row whose first
           k-step is ~1e-3 and whose last is ~1e3 (the running row scale is lowered inside the row), an all-zero row, a window scaled so
           that k reaches 2^15 and beyond, and a window in which every |k| and |v| stays below 2^-4 (both range-scale paths of the
           attention; asserted on the reference's qkv tensor).
fp64       below 2048 tokens, (1, 7, 7, 0, 96, 3) and (2, 14, 21, 3, 96, 3): err < max(2 err32, 2e-6 scale) against an fp64 Linear plus
           oracle.cpu_path.window_attention_image, err32 the error of F.linear in fp32 followed by ops.window_attention_image(mma="f16x3").
refusals   C = 128, 12 x 12 windows, a misaligned x, a view of the weight: None.
module     SwinTransformer at Swin-T widths, switch on == switch off under torch.equal on all four outputs: 2 frames of 64 x 96 (768
           and 192 tokens in stages 1 and 2: below the three-product Linear's 2048 rows both sides take the two launches -- the routing
           keeps the parent's bits there), and 2 frames of 256 x 320 (10 240 and 2 560 tokens), where stages 1-2 make four fused calls and no
           `ops.linear_fused` call with N = 3 C.
Every line printed is `SQ <shape> <bias> err err32 scale`."""
import pytest
import torch

from oracle import cpu_path
from univs_amd import ops, swin_ops, synth
from univs_amd.modeling.backbone.swin import BasicLayer, SwinTransformer
from univs_amd.switches import override

pytestmark = pytest.mark.gpu
F = torch.nn.functional
WS, HD = 7, 32
SHAPES = [(2, 30, 45, 0, 96, 3), (3, 30, 45, 3, 192, 6), (1, 46, 47, 3, 96, 3), (3, 23, 40, 3, 192, 6), (1, 189, 189, 3, 96, 3)]
SMALL = [(1, 7, 7, 0, 96, 3), (2, 14, 21, 3, 96, 3)]
_CACHE = {}


def _window_tokens(H, W, shift, wy, wx):
    """token indices (within one image) of window (wy, wx): pixel ((7 wy + py + shift) mod Hp, (7 wx + px + shift) mod Wp) where it is real"""
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    toks = []
    for py in range(WS):
        for px in range(WS):
            y, x = (wy * WS + py + shift) % Hp, (wx * WS + px + shift) % Wp
            if y < H and x < W:
                toks.append(y * W + x)
    return toks


def _inputs(shape, cuda, special):
    """x [B, L, C], (w [3C, C], b [3C]) of the qkv Linear, bias [nH, 49, 49], mask [nW, 49, 49] or None; (big, small) token lists"""
    key = (shape, special)
    if key not in _CACHE:
        B, H, W, shift, C, nH = shape
        tag = "swinqkv/" + "x".join(str(v) for v in shape)
        x = synth.normal(tag + "/x", (B, H * W, C))
        big = small = None
        if special:
            x[0, 5, :32] *= 1e-3                                 # the running scale is set for 1e-3 and lowered for the last k-step
            x[0, 5, C - 32:] *= 1e3
            x[0, 11] = 0.0                                       # a zero row
            big, small = _window_tokens(H, W, shift, 0, 0), _window_tokens(H, W, shift, 1, 1)
            assert len(small) == WS * WS                         # (an interior window: no padded pixel, whose k and v would be the bias)
            x[B - 1, big] *= 3.0e5
            x[B - 1, small] *= 1.0e-4
        w = synth.normal(tag + "/w", (3 * C, C), std=C ** -0.5)
        b = synth.normal(tag + "/b", (3 * C,), std=0.004)
        bias = synth.normal(tag + "/bias", (nH, WS * WS, WS * WS), std=0.5)
        mask = BasicLayer(C, 2, nH)._shift_mask(H, W, "cpu") if shift else None
        _CACHE[key] = tuple(None if t is None else t.to(cuda) for t in (x, w, b, bias, mask)) + (big, small)
    return _CACHE[key]


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_fused_equals_the_two_launches_bit_for_bit(cuda, shape, with_bias):
    B, H, W, shift, C, nH = shape
    x, w, b, bias, mask, big, small = _inputs(shape, cuda, True)
    b = b if with_bias else None
    scale = HD ** -0.5
    qkv = ops.linear_fused(x, w, b)
    assert qkv is not None, "ops.linear_fused declined: the yardstick is not the three-product Linear"
    qkv = qkv.view(B, H * W, 3, nH, HD)
    # the inputs reach what they are for: k beyond 2^15 in one window, every |k|, |v| of another below 2^-4
    assert qkv[B - 1, big, 1].abs().max().item() >= 2.0 ** 15
    assert qkv[B - 1, small, 1:].abs().max().item() < 2.0 ** -4
    ref = ops.window_attention_image(qkv, b, bias, mask, H, W, WS, shift, scale, mma="f16x3")
    assert torch.isfinite(ref).all()
    x0 = x.clone()
    out = swin_ops.window_attention_qkv(x, w, b, bias, mask, H, W, WS, shift, scale)
    assert out is not None, "the entry answered None: the case is not covered"
    assert tuple(out.shape) == (B, H * W, C) and torch.equal(x, x0)
    diff = (out != ref)
    print(f"SQ {shape} {'bias' if with_bias else 'nobias'} differing elements {int(diff.sum())} of {out.numel()}, "
          f"max |diff| {(out - ref).abs().max().item():.3e}")
    assert torch.equal(out, ref)


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(str(v) for v in s))
def test_small_shapes_against_fp64(cuda, shape):
    B, H, W, shift, C, nH = shape
    x, w, b, bias, mask, _, _ = _inputs(shape, cuda, False)
    scale = HD ** -0.5
    out = swin_ops.window_attention_qkv(x, w, b, bias, mask, H, W, WS, shift, scale)
    assert out is not None and tuple(out.shape) == (B, H * W, C)
    x64, w64, b64, bias64 = (t.double().cpu() for t in (x, w, b, bias))
    qkv64 = F.linear(x64, w64, b64).view(B, H * W, 3, nH, HD)
    ref = cpu_path.window_attention_image(qkv64, b64, bias64, None if mask is None else mask.double().cpu(), H, W, WS, shift, scale)
    y32 = ops.window_attention_image(F.linear(x, w, b).view(B, H * W, 3, nH, HD).contiguous(), b, bias, mask, H, W, WS, shift, scale, mma="f16x3")
    err, err32 = (out.double().cpu() - ref).abs().max().item(), (y32.double().cpu() - ref).abs().max().item()
    sc = ref.abs().max().item()
    print(f"SQ {shape} bias {err:.3e} {err32:.3e} {sc:.3e}")
    assert err < max(2.0 * err32, 2e-6 * sc), (err, err32, sc)


def test_what_is_not_covered_answers_none(cuda):
    scale = HD ** -0.5
    H, W = 14, 21

    def args(C, nH, ws):
        n = ws * ws
        return (torch.zeros(1, H * W, C, device=cuda), torch.zeros(3 * C, C, device=cuda), torch.zeros(3 * C, device=cuda),
                torch.zeros(nH, n, n, device=cuda))

    x, w, b, bias = args(128, 4, WS)
    assert swin_ops.window_attention_qkv(x, w, b, bias, None, H, W, WS, 0, scale) is None            # C = 128
    x, w, b, bias = args(96, 3, 12)
    assert swin_ops.window_attention_qkv(x, w, b, bias, None, H, W, 12, 0, scale) is None            # 12 x 12 windows
    x, w, b, bias = args(96, 3, WS)
    assert swin_ops.window_attention_qkv(x, w, b, bias, None, H, W, WS, 0, scale) is not None
    xm = torch.zeros(H * W * 96 + 1, device=cuda)[1:].view(1, H * W, 96)                             # 4 bytes off a 16-byte boundary
    assert xm.data_ptr() % 16 == 4 and swin_ops.window_attention_qkv(xm, w, b, bias, None, H, W, WS, 0, scale) is None
    wv = torch.zeros(3 * 96 + 1, 96, device=cuda)[1:]                                                # a view: no cached split image
    assert wv.is_contiguous() and swin_ops.window_attention_qkv(x, wv, b, bias, None, H, W, WS, 0, scale) is None


@pytest.mark.parametrize("hw,fused_calls", [((64, 96), 0), ((256, 320), 4)], ids=["64x96", "256x320"])
def test_swin_backbone_switch_on_equals_switch_off(cuda, monkeypatch, hw, fused_calls):
    model = synth.load_synthetic(SwinTransformer(), "swinqkv/model").to(cuda).eval()
    frames = synth.synthetic_frames(2, hw[0], hw[1]).to(cuda)
    with torch.no_grad(), override(swin_fused_qkv=False):
        off = model(frames)
    linears, fused = [], []
    real_linear, real_fused = ops.linear_fused, swin_ops.window_attention_qkv

    def counted_linear(x, weight, *a, **k):
        linears.append((int(weight.shape[0]), int(weight.shape[1])))
        return real_linear(x, weight, *a, **k)

    def counted_fused(x, *a, **k):
        y = real_fused(x, *a, **k)
        fused.append((int(x.shape[-1]), y is not None))
        return y

    monkeypatch.setattr(ops, "linear_fused", counted_linear)
    monkeypatch.setattr(swin_ops, "window_attention_qkv", counted_fused)
    with torch.no_grad(), override(swin_fused_qkv=True):
        on = model(frames)
    assert sorted(on) == sorted(off) == ["res2", "res3", "res4", "res5"]
    for k in on:
        assert torch.equal(on[k], off[k]), k
    assert len(fused) == fused_calls and all(ok for _, ok in fused)
    if fused_calls:
        assert sorted(c for c, _ in fused) == [96, 96, 192, 192]
        assert not [nk for nk in linears if nk in ((288, 96), (576, 192))], "stages 1-2 still ran a qkv Linear"
