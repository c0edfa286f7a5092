"""Measures the semantic-feature decoder (univs_amd/inference/semantic_to_mask.py) on one GPU against the reference's formulation in
ATen on the same GPU, at T = 300 frames, N = 200 tokens, C = 256, temporal stride 10, for 22 x 40 and 90 x 160 pixels:

  selection   the two counts per row: semantic_ops.semantic_quality_counts (the kernel, its wrapper and the output allocation) against
              the logit stack, its strided view, two boolean stacks and two reductions (semantic_feature_to_mask.py:9-12, :101-109);
              the counts must equal those of the logits the exact-f32 mask decode stores (`counts_equal`); how many rows the ATen
              GEMM's other summation order counts differently is reported beside it
  convert     `ConvertSemanticFeatureToMask.convert` end to end against the reference's `convert` restated on the same parameters;
              the indices must be equal.  The thresholds sit in the widest gap near the median of each score, so a minority of the rows survives both.

Per side: `--samples` alternating samples after `--warmup` untimed calls, median with min-max, and the allocator's peak above the inputs
and the outputs of one call.  One JSON line; `--out profiles/semantic_decode_bench_v1.json` keeps it.

    python tools/semantic_decode_bench.py --out profiles/semantic_decode_bench_v1.json
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import eval_bench_common as common                                                  # noqa: E402
from univs_amd import ops, semantic_ops                                               # noqa: E402
from univs_amd.inference.semantic_to_mask import ConvertSemanticFeatureToMask      # noqa: E402

T, N, C, STRIDE, K, E = 300, 200, 256, 10, 1203, 640
SIZES = {"22x40": (22, 40), "90x160": (90, 160)}


def reference_counts(me, feats, s):
    L = torch.einsum("tnc,tchw->tnhw", me, feats).transpose(0, 1)
    W = L[:, ::s]
    return torch.stack([(W > 1).flatten(1).sum(-1), (W > -1).flatten(1).sum(-1)], dim=1).to(torch.int32)


@torch.no_grad()
def reference_convert(conv, mask_feats, obj_tokens):
    """semantic_feature_to_mask.py:90-114 on the converter's parameters, in ATen."""
    x = conv.decoder_norm(obj_tokens.transpose(1, 2))
    cls_logits = F.linear(x, conv.vis2text_projection.weight, conv.vis2text_projection.bias)
    clip = F.normalize(conv.clip_cls_text_emb, p=2, dim=-1)
    cls_logits = torch.einsum("tnc,kc->tnk", F.normalize(cls_logits, p=2, dim=-1), clip) * conv.cls_temp.weight.exp()
    cls_logits = cls_logits.transpose(0, 1)
    me = x
    for i, layer in enumerate(conv.mask_embed.layers):
        me = F.linear(me, layer.weight, layer.bias)
        me = F.relu(me) if i < 2 else me
    mask_logits = torch.einsum("tnc,tchw->tnhw", me, mask_feats).transpose(0, 1)
    conf = cls_logits.sigmoid()[..., 1000:].flatten(1).max(1)[0] > conv.apply_cls_thres
    W = mask_logits[:, ::conv.temporal_stride]
    quality = (W > 1).flatten(1).sum(-1) / (W > -1).flatten(1).sum(-1).clamp(min=1)
    idx = torch.nonzero(conf & (quality > conv.apply_mask_quality_thres)).reshape(-1)
    return cls_logits[idx], mask_logits[idx], idx


def counts_check(me, feats):
    """(the kernel's counts equal those of the logits ops.mask_decode STORES under the exact-f32 setting -- the tensor the kept rows are
    taken from --, the rows whose ATen counts differ from the kernel's, the largest such difference).  The ATen contraction is a library
    GEMM with another summation order: a logit within rounding of a threshold can fall on its other side there."""
    got = semantic_ops.semantic_quality_counts(me, feats, STRIDE).long()
    with ops.configured(mask_decode_impl=1):
        W = ops.mask_decode(me, feats)[:, ::STRIDE]
    exact = torch.stack([(W > 1).flatten(1).sum(-1), (W > -1).flatten(1).sum(-1)], dim=1)
    del W
    off = (reference_counts(me, feats, STRIDE).long() - got).abs()
    return bool(torch.equal(got, exact)), int((off.sum(1) > 0).sum()), int(off.max())


def peak_above(fn, out_bytes):
    """The allocator's peak during one call of fn, above what was allocated before it and above its outputs, in MB."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return round(max(0, peak - out_bytes) / 1e6, 1)


def widest_gap(scores):
    """A threshold in the widest gap between neighbours of the middle half of the sorted scores: about half of the rows pass, and none
    sits where the last bits of the two formulations' arithmetic decide."""
    v = torch.sort(scores.double().cpu())[0]
    mid = v[len(v) // 4:3 * len(v) // 4]
    i = int(torch.argmax(mid[1:] - mid[:-1]))
    return float(mid[i] + mid[i + 1]) / 2


def nbytes(r):
    return sum(x.numel() * x.element_size() for x in (r if isinstance(r, (tuple, list)) else (r,)))


def converter(dev):
    rs = np.random.RandomState(0)
    sd = {"decoder_norm.weight": np.ones(C), "decoder_norm.bias": np.zeros(C), "cls_temp.weight": [[np.log(4.0)]],
          "vis2text_projection.weight": rs.normal(0, 1, (E, C)) / np.sqrt(C), "vis2text_projection.bias": np.zeros(E)}
    for i in range(3):
        sd[f"mask_embed.layers.{i}.weight"] = rs.normal(0, 1, (C, C)) * np.sqrt((2.0 if i < 2 else 1.0) / C)
        sd[f"mask_embed.layers.{i}.bias"] = 0.1 * rs.normal(0, 1, C)
    sd = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in sd.items()}
    clip = torch.from_numpy(rs.normal(0, 1, (K, E)).astype(np.float32))
    return ConvertSemanticFeatureToMask(hidden_dim=C, mask_dim=C, text_emb_dim=E, temporal_stride=STRIDE, clip_class_embed_path=clip,
                                        pretrained_ckpt=sd, device=dev)


def main():
    args = common.arg_parser(reps=5).parse_args()
    dev = common.gpu_or_exit("semantic_decode_bench")
    conv = converter(dev)
    out = {"tool": "semantic_decode_bench", "T": T, "N": N, "C": C, "stride": STRIDE, "K": K, "samples": args.samples, "warmup": args.warmup,
           "reps_fused_selection": args.reps, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for name, (h, w) in SIZES.items():
        g = torch.Generator().manual_seed(h)
        tokens = (torch.randn(1, C, N, generator=g) + 0.5 * torch.randn(T, C, N, generator=g)).to(dev)
        with torch.no_grad():
            _, me = conv.heads(tokens)
        # a shared direction at one of two levels per pixel plus noise, scaled to logits of deviation 2: rows differ in quality
        feats = torch.randn(1, C, 1, 1, generator=g) * (torch.randint(0, 2, (T, 1, h, w), generator=g) * 2.0 - 1.0) + torch.randn(T, C, h, w, generator=g)
        feats = feats.to(dev)
        feats = (feats * (2.0 / float(torch.einsum("nc,chw->nhw", me[0], feats[0]).std()))).contiguous()
        o = {"logit_stack_MB": round(T * N * h * w * 4 / 1e6, 1)}

        sel = {}
        fused_sel = lambda: (semantic_ops.semantic_quality_counts(me, feats, STRIDE),)        # noqa: E731
        aten_sel = lambda: (reference_counts(me, feats, STRIDE),)                                # noqa: E731
        common.kernel_vs_aten(sel, args, fused_sel, aten_sel, "counts_equal_to_aten")
        sel["counts_equal"], sel["aten_rows_off"], sel["aten_max_off"] = counts_check(me, feats)
        sel["fused_peak_MB"] = peak_above(fused_sel, N * 2 * 4)
        sel["aten_peak_MB"] = peak_above(aten_sel, N * 2 * 4)
        o["selection"] = sel

        with torch.no_grad():
            cls_all, _ = conv.heads(tokens)
            conf, quality, _ = conv.scores(cls_all, me, feats)
        conv.apply_cls_thres, conv.apply_mask_quality_thres = widest_gap(conf), widest_gap(quality)
        del cls_all
        cv = {}
        fused_cv = lambda: conv.convert(feats, tokens)                                          # noqa: E731
        aten_cv = lambda: reference_convert(conv, feats, tokens)                                # noqa: E731
        a, b = fused_cv(), aten_cv()
        cv["kept_rows"] = int(a[2].numel())
        if torch.equal(a[2], b[2]) and a[2].numel():
            cv["max_abs_diff_mask_logits"] = float((a[1] - b[1]).abs().max())
            cv["max_abs_diff_cls_logits"] = float((a[0] - b[0]).abs().max())
        ob = nbytes(a)
        del a, b
        reps, args.reps = args.reps, 1
        common.kernel_vs_aten(cv, args, lambda: (fused_cv()[2],), lambda: (aten_cv()[2],), "indices_equal")
        args.reps = reps
        cv["fused_peak_MB"] = peak_above(fused_cv, ob)
        cv["aten_peak_MB"] = peak_above(aten_cv, ob)
        o["convert"] = cv
        out["sizes"][name] = o
        del feats, tokens, me
        torch.cuda.empty_cache()
    common.emit(out, args.out)


if __name__ == "__main__":
    main()
