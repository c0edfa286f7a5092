"""GPU: the seams of a post-norm decoder layer (include/univs_seam_hip.h, univs_amd/seam_ops.py, SWITCHES.decoder_seams) against the
launches they replace.  A seam changes no arithmetic -- the second kernel's operand tile is built from the first one's rows in LDS
instead of from memory -- so every comparison is `torch.equal`, never a tolerance.

  kernel   ops.small_seam == ops.small_linear(residual, ln) followed by ops.small_linear on its result, both outputs
  chain    ops.small_mlp(pre_ln=, side=) == ops.layer_norm(residual) + ops.small_mlp + ops.small_linear, all outputs
  module   a small head with SWITCHES.decoder_seams on and off: every tensor of the output dict; with prompt queries (the ProCA layers
           rewrite the prompt queries between a head and the next cross-attention: that hand-over must not happen) and frame-sharded
           under a one-rank group (no seam applies: the in-projection runs on the gathered tensor)
  count    the launches of one decoder layer with the switch on: 9, so that a silent fallback cannot pass for success

Rows: M in {1, 15, 16, 17, 33} -- the edges of the 16-row tile; a workgroup never sees another tile, so more rows add nothing."""
import os

import pytest
import torch

from univs_amd import ops, synth
from univs_amd import workloads as cases
from univs_amd.switches import SWITCHES, override

pytestmark = pytest.mark.gpu

MS = (1, 15, 16, 17, 33)
LN_EPS = 1e-5
# special rows (where the tile has them): all zero | 1e4 | 1e-30 | t + add cancels exactly
R_ZERO, R_BIG, R_TINY, R_CANCEL = 1, 3, 5, 7


def _n(tag, *shape, std=1.0):
    return synth.normal(f"decoder_seams/{tag}", tuple(shape), std=std)


# (name, rows of W_b, range (f_off, N_b) | None, add, add_features, relu)
SEAM_CASES = [
    ("n256_add", 256, None, True, 0, False),
    ("n768_add512", 768, None, True, 512, False),                # the self-attention's packed in-projection: q, k from t + add, v from t
    ("n512_of_768_at_256_add256", 768, (256, 512), True, 256, False),   # a range of a packed image at a non-zero f_off, both tiles
    ("n768_of_1024_at_256_add512", 1024, (256, 768), True, 512, False),
    ("n2048_relu", 2048, None, False, 0, True),                 # the FFN's linear1 + ReLU
]


@pytest.mark.parametrize("biases", [True, False], ids=["biases", "no_biases"])
@pytest.mark.parametrize("case", SEAM_CASES, ids=[c[0] for c in SEAM_CASES])
@pytest.mark.parametrize("M", MS)
def test_seam_kernel_is_the_two_launches(cuda, M, case, biases):
    name, nwb, rows, with_add, add_features, relu = case
    x, res = _n(f"x/{M}", M, 256), _n(f"res/{M}", M, 256)
    if M > R_CANCEL:
        x[R_ZERO], res[R_ZERO] = 0.0, 0.0                       # row maximum 0 in stage A's tile (and, without biases, t = 0 at the hand-over)
        x[R_BIG] *= 1e4
        x[R_TINY] *= 1e-30                                      # 1e4 and 1e-30 in ONE tile: per-row scales
        res[R_TINY] *= 1e-30                                    # (without the LayerNorm bias this row of t is ~1e-28: the hand-over's scale too)
    wa, wb = _n("wa", 256, 256, std=1 / 16), _n(f"wb/{nwb}", nwb, 256, std=1 / 16)
    ba, bb = (_n("ba", 256, std=0.1), _n(f"bb/{nwb}", nwb, std=0.1)) if biases else (None, None)
    ln = (1.0 + _n("ln_g", 256, std=0.2), _n("ln_b", 256, std=0.1) if biases else None, LN_EPS)
    x, res, wa, wb = (v.to(cuda) for v in (x, res, wa, wb))
    ba, bb = (None if v is None else v.to(cuda) for v in (ba, bb))
    ln = (ln[0].to(cuda), None if ln[1] is None else ln[1].to(cuda), ln[2])

    t_ref = ops.small_linear(x, wa, ba, residual=res, ln=ln)
    assert t_ref is not None
    add = None
    if with_add:
        add = _n(f"add/{M}", M, 256).to(cuda)
        if M > R_CANCEL:
            add[R_BIG] *= 1e4                                   # a row of t + add at 1e4 beside rows of order 1
            add[R_CANCEL] = -t_ref[R_CANCEL]                    # t + add exactly zero: the zero row maximum at the hand-over
    y_ref = ops.small_linear(t_ref, wb, bb, rows=rows, x_add=add, relu=relu, add_features=add_features)
    assert y_ref is not None
    got = ops.small_seam(x, wa, ba, res, ln, wb, bb, rows=rows, add=add, relu=relu, add_features=add_features)
    assert got is not None, "the seam kernel does not cover the call"
    t, y = got
    assert t.shape == t_ref.shape and y.shape == y_ref.shape
    assert torch.isfinite(t_ref).all() and torch.isfinite(y_ref).all()
    assert torch.equal(t, t_ref), f"t differs in {(t != t_ref).sum().item()} values, max {(t - t_ref).abs().max().item():.3e}"
    assert torch.equal(y, y_ref), f"y differs in {(y != y_ref).sum().item()} values, max {(y - y_ref).abs().max().item():.3e}"
    if M > R_CANCEL and with_add:
        assert (t_ref[R_CANCEL] + add[R_CANCEL]).abs().max().item() == 0.0
    if M > R_CANCEL and not biases:
        assert t_ref[R_ZERO].abs().max().item() == 0.0 and 0.0 < t_ref[R_TINY].abs().max().item() < 1e-20


def test_seam_kernel_answers_none_where_it_does_not_apply(cuda):
    x, res = _n("x/16", 16, 256).to(cuda), _n("res/16", 16, 256).to(cuda)
    wa, wb = _n("wa", 256, 256, std=1 / 16).to(cuda), _n("wb/768", 768, 256, std=1 / 16).to(cuda)
    ln = (torch.ones(256, device=cuda), None, LN_EPS)
    assert ops.small_seam(x, wa, None, res, ln, wb) is not None
    assert ops.small_seam(x, wa, None, res, ln, wb, rows=(0, 128)) is None                      # N_b no multiple of 256
    assert ops.small_seam(x, wa, None, res, ln, wb[:512]) is None                              # a view: no cached split of its own
    assert ops.small_seam(x[:, :128].contiguous(), wa[:, :128].contiguous(), None, res, ln, wb) is None     # K != 256
    assert ops.small_seam(x, wa, None, res, None, wb) is None                                  # no LayerNorm: not a layer's tail
    assert ops.small_seam(x.cpu(), wa.cpu(), None, res.cpu(), (ln[0].cpu(), None, LN_EPS), wb.cpu()) is None
    assert ops.small_seam(torch.zeros(5000, 256, device=cuda), wa, None, torch.zeros(5000, 256, device=cuda), ln, wb) is None


# ---- the chain with the end of the layer in front of it

def _chain_operands(cuda, shape):
    M = 1
    for s in shape[:-1]:
        M *= s
    x, res = _n(f"chain/x/{shape}", M, 256), _n(f"chain/res/{shape}", M, 256)
    if M > 4:
        x[2] = x[2] + 1000.0                                    # mean >> spread (tests/test_norm_conditioning_gpu.py: big_mean)
        x[3], res[3] = 3.25, 0.5                                # a constant row: variance 0
        x[4] = x[4] * 1e-3 + 5.0                                # eps matters
        res[4] = 0.0
    lay = [(_n(f"chain/w{i}", 256, 256, std=1 / 16).to(cuda), _n(f"chain/b{i}", 256, std=0.1).to(cuda), i < 2) for i in range(3)]
    pre = ((1.0 + _n("chain/pre_g", 256, std=0.2)).to(cuda), _n("chain/pre_b", 256, std=0.1).to(cuda))
    inn = ((1.0 + _n("chain/in_g", 256, std=0.2)).to(cuda), _n("chain/in_b", 256, std=0.1).to(cuda), LN_EPS)
    wq, bq = _n("chain/wq", 768, 256, std=1 / 16).to(cuda), _n("chain/bq", 768, std=0.1).to(cuda)    # a packed in-projection: q = its rows [0, 256)
    qpos = _n(f"chain/qpos/{shape}", *shape).to(cuda)
    return x.view(shape).to(cuda), res.view(shape).to(cuda), lay, pre, inn, wq, bq, qpos


@pytest.mark.parametrize("shape", [(m, 256) for m in MS] + [(6, 1, 256), (3, 2, 256)], ids=[f"M{m}" for m in MS] + ["M6_outT0", "M6_outT2"])
def test_chain_with_layer_end_is_the_separate_launches(cuda, shape):
    x, res, lay, pre, inn, wq, bq, qpos = _chain_operands(cuda, shape)
    t01 = len(shape) == 3 and shape[1] == 2
    if len(shape) == 3 and not t01:
        x, res, qpos = x.view(6, 256), res.view(6, 256), qpos.view(6, 256)
    xr_ref = ops.layer_norm(x, pre[0], pre[1], LN_EPS, residual=res)
    y_ref, xn_ref = ops.small_mlp(xr_ref, lay, in_ln=inn, want_normed=True, transpose01=t01)
    q_ref = ops.small_linear(xr_ref, wq, bq, rows=(0, 256), x_add=qpos)
    assert q_ref is not None
    got = ops.small_mlp(x, lay, in_ln=inn, want_normed=True, transpose01=t01, pre_ln=(res, pre[0], pre[1], LN_EPS), side=(wq, bq, (0, 256), qpos))
    assert got is not None, "the chain does not cover the call"
    y, xn, xr, q = got
    for name, a, b in (("x'", xr, xr_ref), ("y", y, y_ref), ("q", q, q_ref), ("x_normed", xn, xn_ref)):
        assert a.shape == b.shape and torch.isfinite(b).all(), name
        assert torch.equal(a, b), f"{name} differs in {(a != b).sum().item()} values, max {(a - b).abs().max().item():.3e}"
    # each front stage alone, and the side Linear of another range without its add and bias
    y2, xr2 = ops.small_mlp(x, lay, in_ln=inn, transpose01=t01, pre_ln=(res, pre[0], pre[1], LN_EPS))
    assert torch.equal(y2, y_ref) and torch.equal(xr2, xr_ref)
    y3, q3 = ops.small_mlp(xr_ref, lay, in_ln=inn, transpose01=t01, side=(wq, None, (512, 256), None))
    assert torch.equal(y3, y_ref) and torch.equal(q3, ops.small_linear(xr_ref, wq, None, rows=(512, 256)))
    assert ops.small_mlp(x, lay, side=(wq, bq, (0, 128), qpos)) is None and ops.small_mlp(x, lay, pre_ln=(res, pre[0], None, LN_EPS)) is None


# ---- modules

def _build_head(case, device, layers):
    """workloads.build_head with `layers` decoder layers"""
    from univs_amd.modeling.meta_arch.mask_former_head import MaskFormerHead
    from univs_amd.modeling.prompt_encoder import VisualPromptSampler
    from univs_amd.modeling.transformer_decoder.univs_decoder import VideoMultiScaleMaskedTransformerDecoderUniVS
    from univs_amd.registry import ShapeSpec
    kw = dict(cases.decoder_kwargs(case), dec_layers=layers)
    dec = VideoMultiScaleMaskedTransformerDecoderUniVS(
        clip_class_embed_path=cases.clip_table(), visual_prompt_sampler=VisualPromptSampler(**cases.sampler_kwargs(case)),
        return_aux_outputs=True, **kw).eval()
    synth.load_synthetic(dec, prefix="sem_seg_head.predictor.")
    ish = {k: ShapeSpec(channels=c, stride=s) for k, (c, s) in case["shapes"].items()}
    head = MaskFormerHead(ish, num_classes=133, pixel_decoder=cases.build_pixel_decoder(case["shapes"]),
                          pixel_decoder_name="MSDeformAttnPixelDecoder", transformer_predictor=dec,
                          transformer_in_feature="multi_scale_pixel_decoder").eval()
    return head.to(device)


SMALL = dict(cases.HEAD_CASE, name="head_seams", Q=6)            # two frames, six queries, levels of 2 x 3, 4 x 6 and 8 x 12 pixels
WIDE = dict(cases.HEAD_CASE, name="head_seams_wide", Q=32, H=256, W=384)   # every attention on the fused core, as the flagship clip's


def _warm_head(case, cuda):
    """(head, the pixel decoder's outputs), computed ONCE: the seams live in the transformer decoder (`head.predictor`), and the runs that
    are compared must see the same inputs bit for bit.  The pixel decoder itself does not give them twice on feature maps of a few
    pixels -- its mask features differ in the last bits from call to call (a library convolution; with the seams off too, measured),
    while the decoder on fixed inputs is reproducible."""
    head, feats = _build_head(case, cuda, 3), {k: v.to(cuda) for k, v in cases.backbone_features(case).items()}
    with torch.no_grad():
        mask_features, bfe_conv, _, multi_scale = head.pixel_decoder.forward_features(feats)
    return head, (multi_scale, mask_features, bfe_conv)


def _decode(head, inputs, targets):
    return head.predictor(*inputs, None, targets)


@pytest.fixture(scope="module")
def small_head(cuda):
    return _warm_head(SMALL, cuda)


@pytest.fixture(scope="module")
def wide_head(cuda):
    return _warm_head(WIDE, cuda)


def _flatten(out, prefix=""):
    """every tensor of an output dict, by path"""
    if isinstance(out, torch.Tensor):
        return {prefix: out}
    if isinstance(out, dict):
        return {k2: v2 for k, v in out.items() for k2, v2 in _flatten(v, f"{prefix}/{k}").items()}
    if isinstance(out, (list, tuple)):
        return {k2: v2 for i, v in enumerate(out) for k2, v2 in _flatten(v, f"{prefix}[{i}]").items()}
    return {}


def _on_off(head, feats, targets, cuda):
    def to_dev(tv):
        return [{k: (v.to(cuda) if isinstance(v, torch.Tensor) else v) for k, v in t_.items()} for t_ in tv]
    with torch.no_grad():
        with override(decoder_seams=False):
            ref = _flatten(_decode(head, feats, to_dev(targets())))
        with override(decoder_seams=True):
            got = _flatten(_decode(head, feats, to_dev(targets())))
    assert sorted(got) == sorted(ref) and len(ref) >= 3 + 3 * 3          # the last head's three tensors and those of three aux heads
    for k in ref:
        assert got[k].shape == ref[k].shape, k
        assert torch.equal(got[k], ref[k]), f"{k}: {(got[k] != ref[k]).sum().item()} values differ"
    return ref


def _count_seams(fn):
    """the names of all wrapper calls of fn(), in order"""
    names, orig = [], ops._call

    def call(name, *a, **k):
        names.append(name)
        return orig(name, *a, **k)
    ops._call = call
    try:
        fn()
    finally:
        ops._call = orig
    return names


@pytest.mark.parametrize("which", ["small", "wide"])
def test_head_with_seams_is_the_head_without(cuda, small_head, wide_head, which):
    head, feats = small_head if which == "small" else wide_head
    case = SMALL if which == "small" else WIDE
    _on_off(head, feats, lambda: cases.targets_first_clip(case), cuda)
    with torch.no_grad(), override(decoder_seams=True):
        names = _count_seams(lambda: _decode(head, feats, cases.targets_first_clip(case)))
    assert names.count("small_seam") == 2 * 3, names              # (the equality above is not that of a silent fallback)


def test_head_with_prompt_queries_falls_back_around_proca(cuda, small_head):
    """The second clip of a video: entity prompts are appended to the queries and ProCA layers rewrite them between a prediction head and
    the next cross-attention -- the query projection made beside the head must not be used there."""
    head, feats = small_head
    prev = SWITCHES.sampler
    SWITCHES.sampler = "reference"                                # (host draws: the same prompts in both runs)
    try:
        def targets():
            torch.manual_seed(0)                                  # (read by the sampler's draws behind this call)
            return cases.targets_with_entities(SMALL)
        ref = _on_off(head, feats, targets, cuda)
    finally:
        SWITCHES.sampler = prev
    assert any(v.shape[1] > SMALL["Q"] for k, v in ref.items() if k.endswith("pred_logits")), "no prompt queries were appended"


def test_frame_sharded_head_is_untouched(cuda, small_head):
    import tempfile

    import torch.distributed as dist
    from univs_amd.distributed import FrameShard
    head, feats = small_head
    own = not dist.is_initialized()
    if own:
        store = dist.FileStore(os.path.join(tempfile.mkdtemp(), "store"), 1)
        dist.init_process_group("gloo", store=store, rank=0, world_size=1)
    try:
        head.predictor.frame_shard = FrameShard()
        _on_off(head, feats, lambda: cases.targets_first_clip(SMALL), cuda)
        with torch.no_grad(), override(decoder_seams=True):
            names = _count_seams(lambda: _decode(head, feats, cases.targets_first_clip(SMALL)))
        assert "small_seam" not in names
    finally:
        head.predictor.frame_shard = None
        if own:
            dist.destroy_process_group()


def test_a_decoder_layer_is_nine_launches(cuda, wide_head):
    """One decoder layer of the flagship structure (every attention on the fused core, K / V projections made ahead, no class logits for
    an intermediate layer) with the seams: partial, merge | seam | partial, merge | seam | library GEMM | head chain | mask-decode-attn.
    `ops.cross_attention` is the two launches partial + merge (include/univs_fused_hip.h); the library GEMM is counted where
    layers.linear hands it over."""
    from univs_amd import layers
    head, feats = wide_head
    dec = head.predictor
    aux, dec.return_aux_outputs = dec.return_aux_outputs, False
    try:
        with torch.no_grad(), override(decoder_seams=True):
            _decode(head, feats, cases.targets_first_clip(WIDE))                       # (warm: weight splits, padded masks)
            layers.reset_library_linear_counts()
            names = _count_seams(lambda: _decode(head, feats, cases.targets_first_clip(WIDE)))
            gemms = dict(layers.LIBRARY_LINEAR_COUNTS)
    finally:
        dec.return_aux_outputs = aux
    ends = [i for i, n in enumerate(names) if n == "mask_decode_attn"]
    assert len(ends) == 4                                                              # head 0 and the heads behind the three layers
    ffn2 = sum(v for (what, k, n), v in gemms.items() if (k, n) == (2048, 256))
    assert ffn2 == 3, gemms
    # behind head 0, once per clip: the cross-attention K / V projections of all layers, one Linear per level and kind (few rows at this
    # size, so they show up as small_linear; tall GEMMs in the flagship clip) -- not part of a layer
    kv = names[ends[0] + 1:ends[0] + 7]
    assert kv == ["small_linear"] * 6, names[ends[0] + 1:ends[1] + 1]
    for a, b in ((ends[0] + 6, ends[1]), (ends[1], ends[2])):                          # the layers in front of an intermediate head
        layer = names[a + 1:b + 1]
        assert layer == ["cross_attention", "small_seam", "cross_attention", "small_seam", "small_mlp", "mask_decode_attn"], layer
        launches = sum(2 if n == "cross_attention" else 1 for n in layer) + ffn2 // 3
        assert launches == 9
