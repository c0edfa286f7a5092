"""Synthetic workloads of the BASELINE.json configurations: network geometries, closed-form inputs and builders of the
product modules with the closed-form weights (univs_amd/synth.py).  One definition shared by bench.py, tools/ and the
tests (tests/cases.py and tests/helpers.py import these names), and -- through oracle/gen_golden.py, which feeds the very
same tensors to the real reference -- by the golden fixtures.
"""
import numpy as np
import torch

from . import synth
from .registry import ShapeSpec

# ---------------------------------------------------------------------------------------------------
# network geometries
# ---------------------------------------------------------------------------------------------------
SWIN_T = dict(pretrain_img_size=224, patch_size=4, in_chans=3, embed_dim=96, depths=[2, 2, 6, 2],
              num_heads=[3, 6, 12, 24], window_size=7, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
              ape=False, patch_norm=True)

R50_SHAPES = {"res2": (256, 4), "res3": (512, 8), "res4": (1024, 16), "res5": (2048, 32)}   # cfg 1
SWINT_SHAPES = {"res2": (96, 4), "res3": (192, 8), "res4": (384, 16), "res5": (768, 32)}

PIXDEC = dict(transformer_dropout=0.0, transformer_nheads=8, transformer_dim_feedforward=1024,
              transformer_enc_layers=6, conv_dim=256, mask_dim=256, norm="GN",
              transformer_in_features=["res3", "res4", "res5"], common_stride=4)
SWIN_B = dict(pretrain_img_size=384, patch_size=4, in_chans=3, embed_dim=128, depths=[2, 2, 18, 2],
              num_heads=[4, 8, 16, 32], window_size=12, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
              ape=False, patch_norm=True)
SWIN_L = dict(pretrain_img_size=384, patch_size=4, in_chans=3, embed_dim=192, depths=[2, 2, 18, 2],
              num_heads=[6, 12, 24, 48], window_size=12, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
              ape=False, patch_norm=True)
SWINL_SHAPES = {"res2": (192, 4), "res3": (384, 8), "res4": (768, 16), "res5": (1536, 32)}

# a small head case: features of a 64x96 padded input with R50 channel counts
HEAD_CASE = dict(name="head", T=2, H=64, W=96, Q=20, shapes=R50_SHAPES)
# BASELINE config 5's decoder length (T = 10 frames, 200 queries: a 2 000-token spatio-temporal self-attention, class / re-id
# means over 10 frames) on reduced-resolution features -- the decoder does not care about H x W, the reference's own 1080p run
# at T = 10 needs > 100 GB on the CPU (golden g6c)
HEAD_CASE_T10 = dict(name="head_t10", T=10, H=64, W=96, Q=200, shapes=R50_SHAPES)


def backbone_features(case=HEAD_CASE):
    """Synthetic res2..res5 (unit-variance, like LayerNorm'ed Swin outputs)."""
    feats = {}
    for k, (c, s) in case["shapes"].items():
        feats[k] = synth.normal(f"{case['name']}/feat/{k}", (case["T"], c, case["H"] // s, case["W"] // s))
    return feats


def clip_table():
    return synth.uniform("clip_cls_emb", (3938, 640))


def decoder_kwargs(case=HEAD_CASE, text_to_image=False, sa_mask="sep", num_dense_points=32, num_prev=5):
    return dict(in_channels=256, mask_classification=True, num_classes=133, hidden_dim=256,
                num_queries=case["Q"], nheads=8, dim_feedforward=2048, dec_layers=9, pre_norm=False,
                mask_dim=256, enforce_input_project=False, prompt_self_attn_layers=-1, num_frames=case["T"],
                num_dense_points=num_dense_points, text_prompt_enable=True, prompt_as_queries=True,
                text_prompt_to_image_enable=text_to_image, maskdec_self_attn_mask_type=sa_mask,
                position_embedding_sin3d_type="ArbitraryT", num_prev_frames_memory=num_prev,
                enabled_prev_frames_memory=True, enabled_prev_visual_prompts_for_grounding=False)


def sampler_kwargs(case=HEAD_CASE, num_dense_points=32, num_prev=5):
    return dict(pretrain_img_size=1024, hidden_dim=256, num_heads=8, num_frames=case["T"],
                num_prev_frames_memory=num_prev, num_dense_points=num_dense_points,
                position_embedding_sin3d_type="ArbitraryT", clip_stride=1)


def targets_first_clip(case=HEAD_CASE, task="detection", prompt_type="visual", dataset="ytvis_2021_dev"):
    return [{"task": task, "dataset_name": dataset, "prompt_type": prompt_type, "num_frames": case["T"],
             "first_frame_idx": 0, "frame_indices": torch.arange(0, case["T"])}]


def targets_with_entities(case=HEAD_CASE, first_frame_idx=1, n_ent=3):
    """Second clip of a video (stride 1): rectangular entity masks carried over from previous frames.
    masks/boxes cover the frames seen so far plus the (zero-padded) newest frame, as the clip loop leaves
    them (inference_video_entity.py:878-912)."""
    T, H, W = case["T"], case["H"], case["W"]
    t_hist = first_frame_idx + T          # frames 0 .. first_frame_idx+T-1
    masks = torch.zeros(n_ent, t_hist, H, W)
    boxes = torch.zeros(n_ent, t_hist, 4)
    for e in range(n_ent):
        for t in range(t_hist - 1):       # newest frame has no annotation yet
            y0, x0 = 4 + 9 * e + t, 6 + 17 * e + 2 * t
            hh, ww = 14 + 3 * e, 20 + 5 * e
            masks[e, t, y0:y0 + hh, x0:x0 + ww] = 1.0
            boxes[e, t] = torch.tensor([x0 / W, y0 / H, (x0 + ww) / W, (y0 + hh) / H])
    tv = targets_first_clip(case)[0]
    tv.update({"first_frame_idx": first_frame_idx,
               "frame_indices": torch.arange(first_frame_idx, first_frame_idx + T),
               "masks": masks, "boxes": boxes, "ids": torch.arange(n_ent)[:, None].repeat(1, t_hist),
               "first_appear_frame_idxs": torch.zeros(n_ent, dtype=torch.long)})
    return [tv]


# ---------------------------------------------------------------------------------------------------
# BASELINE config 2: Swin-T, T=5 @ 720p (padded 736x1280), 100 queries, first clip
# ---------------------------------------------------------------------------------------------------
CFG2 = dict(name="cfg2", T=5, H=720, W=1280, Q=100, shapes=SWINT_SHAPES)


def cfg2_frames(case=CFG2):
    return synth.synthetic_frames(case["T"], case["H"], case["W"], "frames/seed0")


# Swin-L (configs/univs_inf/vids/vis/univs_swinl_yt21_c1+univs.yaml:5-13) -- BASELINE config 5: T=10 @ 1080p (padded to
# 1088x1920), 200 queries.  The reference's CPU run of the full clip needs > 100 GB, so the golden (g19) is the same
# network on the first TWO frames; the T=10 run is checked through size-independent properties on the GPU.
# BASELINE config 4: Swin-B (window 12), T=5 @ 720p, 200 learnable queries + 4 referring expressions (grounding, 'sep-blocked'
# self-attention mask, text prompts fused into the image features: configs/univs_inf/vids/refvos/univs_swinb_refvos_davis_c1+univs.yaml)
SWINB_SHAPES = {"res2": (128, 4), "res3": (256, 8), "res4": (512, 16), "res5": (1024, 32)}
CFG4 = dict(name="cfg4", T=5, H=720, W=1280, Q=200, shapes=SWINB_SHAPES, n_exp=4)
CFG4_DECODER = dict(text_to_image=True, sa_mask="sep-blocked")


def targets_grounding(case=HEAD_CASE, n_exp=3):
    T = case["T"]
    tv = targets_first_clip(case, task="grounding", prompt_type="text")[0]
    tv["exp_word_feats"] = synth.normal("grounding/word", (n_exp, 77, T, 640))
    tv["exp_sentence_feats"] = synth.normal("grounding/sent", (n_exp, T, 640))
    tv["exp_word_len"] = [7] * n_exp
    return [tv]


def cfg4_targets(case=CFG4):
    return [targets_grounding(case, n_exp=case["n_exp"])[0]]


CFG5 = dict(name="cfg5", T=10, H=1080, W=1920, Q=200, shapes=SWINL_SHAPES)
CFG5_GOLDEN_T = 2


def cfg5_frames(T):
    return synth.synthetic_frames(T, CFG5["H"], CFG5["W"], "cfg5/frames")


def preprocess(frames, divisibility=32):
    """normalise + zero-pad to a multiple of 32 (univs/inference/inference_video_entity.py:251-260)."""
    mean = torch.tensor(synth.PIXEL_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(synth.PIXEL_STD).view(1, 3, 1, 1)
    x = (frames - mean) / std
    H, W = x.shape[-2:]
    Hp, Wp = (H + divisibility - 1) // divisibility * divisibility, (W + divisibility - 1) // divisibility * divisibility
    return torch.nn.functional.pad(x, (0, Wp - W, 0, Hp - H))


# ---------------------------------------------------------------------------------------------------
# product modules with the closed-form weights
# ---------------------------------------------------------------------------------------------------
def build_swin(device="cpu", variant=None, attn_mma="f16x3"):
    from .modeling.backbone.swin import SwinTransformer
    k = dict(variant or SWIN_T)
    m = SwinTransformer(k["pretrain_img_size"], k["patch_size"], k["in_chans"], k["embed_dim"], k["depths"],
                        k["num_heads"], k["window_size"], k["mlp_ratio"], k["qkv_bias"], k["qk_scale"], k["ape"],
                        k["patch_norm"]).eval()
    synth.load_synthetic(m, prefix="backbone.")
    return m.set_attention_mma(attn_mma).to(device)


def build_pixel_decoder(shapes, device="cpu"):
    from .modeling.pixel_decoder.msdeformattn import MSDeformAttnPixelDecoder
    ish = {k: ShapeSpec(channels=c, stride=s) for k, (c, s) in shapes.items()}
    m = MSDeformAttnPixelDecoder(ish, **PIXDEC).eval()
    synth.load_synthetic(m, prefix="sem_seg_head.pixel_decoder.")
    return m.to(device)


def build_head(case, device="cpu", return_aux=True, **dec_over):
    from .modeling.meta_arch.mask_former_head import MaskFormerHead
    from .modeling.prompt_encoder import VisualPromptSampler
    from .modeling.transformer_decoder.univs_decoder import VideoMultiScaleMaskedTransformerDecoderUniVS
    pd = build_pixel_decoder(case["shapes"])
    ish = {k: ShapeSpec(channels=c, stride=s) for k, (c, s) in case["shapes"].items()}
    dec = VideoMultiScaleMaskedTransformerDecoderUniVS(
        clip_class_embed_path=clip_table(), visual_prompt_sampler=VisualPromptSampler(**sampler_kwargs(case)),
        return_aux_outputs=return_aux, **decoder_kwargs(case, **dec_over)).eval()
    synth.load_synthetic(dec, prefix="sem_seg_head.predictor.")
    head = MaskFormerHead(ish, num_classes=133, pixel_decoder=pd, pixel_decoder_name="MSDeformAttnPixelDecoder",
                          transformer_predictor=dec, transformer_in_feature="multi_scale_pixel_decoder").eval()
    return head.to(device)


def build_model(device, case=None, variant=None, return_aux=False, **dec_over):
    """(backbone, head) of a workload on `device` with the closed-form weights: config 2 (Swin-T, 100 queries) by default."""
    case = CFG2 if case is None else case
    return build_swin(device, variant), build_head(case, device, return_aux=return_aux, **dec_over)


# ---------------------------------------------------------------------------------------------------
# per-image post-processing (inference/image_generic_seg.py): closed-form decoder outputs
# ---------------------------------------------------------------------------------------------------
def image_blob_logits(seed, Q, h, w, C, crop_lowres=None):
    """Smooth mask logits L [Q, h, w] and class logits [Q, C] of one image from a seeded recipe (numpy's RandomState, so every machine
    makes the same values): each query is -6 plus one to three Gaussian blobs (centres inside the low-resolution extent of the crop,
    widths 1.5-8 cells, heights 4-12), so that masks overlap, win and lose pixels to each other and stuff classes repeat; class logits
    are N(-2, 1.5^2) with a peak of 3-7 at one class per query (classes drawn from a third of the vocabulary, so that classes recur)."""
    rs = np.random.RandomState(seed)
    ch, cw = crop_lowres if crop_lowres is not None else (h, w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    L = np.full((Q, h, w), -6.0)
    for q in range(Q):
        for _ in range(rs.randint(1, 4)):
            cy, cx = rs.uniform(0, ch), rs.uniform(0, cw)
            s = rs.uniform(1.5, 8.0)
            L[q] += rs.uniform(4.0, 12.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    cls = rs.normal(-2.0, 1.5, size=(Q, C))
    peak = rs.randint(0, max(1, C // 3), size=Q) * 3 % C
    cls[np.arange(Q), peak] += rs.uniform(3.0, 7.0, size=Q)
    return torch.from_numpy(L.astype(np.float32)), torch.from_numpy(cls.astype(np.float32))


class MinVISClipHead:
    """Seeded closed-form stand-in for `sem_seg_head(features, targets=targets)` of the MinVIS-style clip loops: reads the clip's frames
    from targets[0]["frame_indices"] and returns {"pred_logits" [1, Q, C_all], "pred_masks" [1, Q, T, h, w], "pred_embds" [1, Q, T, E],
    "aux_outputs": []} (numpy's RandomState, so every machine makes the same values).

    `n_obj` objects move through the video, each alive in a span of frames (objects enter and leave), with one class, one embedding and
    a Gaussian blob per frame.  Per clip the query order is shuffled (the matching has to undo it), queries of dead objects report a
    faint blob, and in every other clip one object is reported by two queries (its rows repeat in the VIS top-k).  `Q` queries of
    which the first `Q - extra` are learnable; the last `extra` (prompt / text queries) only count in the first clip's top-k.
    `classes`: the class of each object (indices into the dataset's slice [start, start + C) of the C_all columns)."""

    def __init__(self, seed, V, Q, h, w, C_all, start, C, n_obj, extra=0, classes=None, E=32):
        rs = np.random.RandomState(seed)
        self.V, self.Q, self.h, self.w, self.C_all, self.start, self.C = V, Q, h, w, C_all, start, C
        self.n_obj, self.extra, self.E = n_obj, extra, E
        self.seed = seed
        self.cls = np.asarray(classes if classes is not None else rs.randint(0, C, size=n_obj))
        self.emb = rs.normal(0, 1, size=(n_obj, E))
        self.life = []
        for j in range(n_obj):
            f0 = int(rs.randint(0, max(1, V // 3))) if j % 3 == 1 else 0
            f1 = int(rs.randint(2 * V // 3, V)) if j % 3 == 2 else V - 1
            self.life.append((f0, f1))
        self.c0 = rs.uniform(0.2, 0.8, size=(n_obj, 2)) * (h, w)
        self.vel = rs.uniform(-0.6, 0.6, size=(n_obj, 2))
        self.size = rs.uniform(1.5, 4.0, size=n_obj)
        self.peak = rs.uniform(3.0, 7.0, size=n_obj)
        self.bg_emb = rs.normal(0, 1, size=(Q, E))

    def blob(self, j, f, rs):
        yy, xx = np.mgrid[0:self.h, 0:self.w].astype(np.float64)
        cy, cx = self.c0[j] + self.vel[j] * f
        alive = self.life[j][0] <= f <= self.life[j][1]
        amp = (8.0 + self.peak[j]) if alive else 2.0
        s = self.size[j]
        return -5.0 + amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) + rs.normal(0, 0.05, size=(self.h, self.w))

    def __call__(self, features, targets=None):
        frames = [int(v) for v in targets[0]["frame_indices"]]
        i = frames[0]
        T = len(frames)
        rs = np.random.RandomState(self.seed * 1000 + i)
        Ql = self.Q - self.extra
        # query slot -> object (or -1: background); one object twice in every other clip
        slots = list(range(self.n_obj)) + [-1] * (Ql - self.n_obj)
        if i % 2 == 1 and Ql > self.n_obj:
            slots[self.n_obj] = int(rs.randint(0, self.n_obj))
        slots = list(rs.permutation(slots)) + [int(rs.randint(0, self.n_obj)) for _ in range(self.extra)]
        masks = np.empty((self.Q, T, self.h, self.w))
        logits = rs.normal(-4.0, 1.0, size=(self.Q, self.C_all))
        embds = np.empty((self.Q, T, self.E))
        for q, j in enumerate(slots):
            for t, f in enumerate(frames):
                if j >= 0:
                    masks[q, t] = self.blob(j, f, rs)
                    embds[q, t] = self.emb[j] + rs.normal(0, 0.1, size=self.E)
                else:
                    masks[q, t] = -6.0 + rs.normal(0, 0.5, size=(self.h, self.w))
                    embds[q, t] = self.bg_emb[q] + rs.normal(0, 0.3, size=self.E)
            if j >= 0:
                alive = any(self.life[j][0] <= f <= self.life[j][1] for f in frames)
                logits[q, self.start:self.start + self.C] = rs.normal(-3.0, 1.0, size=self.C)
                logits[q, self.start + self.cls[j]] = rs.uniform(1.0, 4.0) if alive else rs.uniform(-2.0, 0.0)
            else:
                logits[q, self.start:self.start + self.C] = rs.normal(-3.5, 1.0, size=self.C)
        f32 = lambda a: torch.from_numpy(a.astype(np.float32))[None]
        return {"pred_logits": f32(logits), "pred_masks": f32(masks), "pred_embds": f32(embds), "aux_outputs": []}


class SemanticClipHead:
    """Seeded closed-form stand-in for `sem_seg_head(features, targets=targets)` under semantic extraction
    (inference/video_semantic_extraction.py): returns {"pred_embds" [T, C, N], "mask_features" [T, C, h, w]} as functions of
    targets[0]["frame_indices"] only (numpy's RandomState per frame, so every machine makes the same values and a frame has the same
    values whichever clip it falls in): smooth planes (a plane wave per channel, drifting with the frame) plus noise, so that both the
    bilinear weights and the choice of the nearest pixel show.  `calls` records what each call received: (first_frame_idx,
    frame_indices, the number of frames of the features handed in)."""

    def __init__(self, seed, C, N, h, w):
        self.seed, self.C, self.N, self.h, self.w = seed, C, N, h, w
        self.calls = []

    def frame(self, f):
        rs = np.random.RandomState(self.seed * 1000 + f)
        yy, xx = np.mgrid[0:self.h, 0:self.w].astype(np.float64)
        ky, kx = rs.uniform(-0.8, 0.8, size=(2, self.C, 1, 1))
        ph = rs.uniform(0, 2 * np.pi, size=(self.C, 1, 1))
        feat = 2.0 * np.sin(ky * yy + kx * xx + ph + 0.3 * f) + rs.normal(0, 0.25, size=(self.C, self.h, self.w))
        tok = rs.normal(0, 1, size=(self.C, self.N))
        return tok.astype(np.float32), feat.astype(np.float32)

    def __call__(self, features, targets=None):
        frames = [int(v) for v in targets[0]["frame_indices"]]
        handed = int(next(iter(features.values())).shape[0])
        self.calls.append((int(targets[0]["first_frame_idx"]), frames, handed))
        toks, feats = zip(*(self.frame(f) for f in frames))
        return {"pred_embds": torch.from_numpy(np.stack(toks)), "mask_features": torch.from_numpy(np.stack(feats))}
