"""MSDeformAttn pixel decoder for the MI355X hot path.

Interface / state-dict layout: the reference's `MSDeformAttnPixelDecoder`
(mask2former/modeling/pixel_decoder/msdeformattn.py:166-360), `MSDeformAttn`
(ops/modules/ms_deform_attn.py:34-121) and the encoder classes (:23-163).  Differences in how the
work is organised (results are the same):

  * the deformable-attention core is the HIP operator (`ops.ms_deform_attn_forward`, LDS-tiled for the
    encoder geometry) fed with the Python-side level table, so there is no device read-back and no
    per-call int64 tensors;
  * quantities that depend only on the feature-map shapes -- sine position embeddings + level embed,
    reference points, the offset normaliser -- are cached per (shape, device) instead of being rebuilt
    per call (msdeformattn.py:61-89, :143-158; position_encoding.py:29-52);
  * the all-False padding mask and the `masked_fill` pass it triggers (ms_deform_attn.py:99-100,
    msdeformattn.py:62) are dropped: valid_ratio is identically 1;
  * everything stays fp32 regardless of autocast (msdeformattn.py:316,322).
"""
import contextlib
from typing import Callable, Dict, List, Optional, Union

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from ... import encoder_ops, fused_ops, ops
from ...layers import Conv2d, get_activation_fn, get_norm, layer_norm, linear, linear_act
from ...registry import SEM_SEG_HEADS_REGISTRY, ShapeSpec, configurable
from ..position_encoding import PositionEmbeddingSine


from ...switches import SWITCHES   # msda_strips (default True): the encoder's MSDeformAttn core on head-major operands
# (csrc/msda_strips.hip): value_proj and the merged offset / logit projection store their outputs in the sampling kernel's
# layouts (blocked Linear epilogue), the kernel handles half a head per workgroup with two workgroups per CU.  False: the
# standard-layout operators (msda_prepare + ms_deform_attn_forward).  msda_heads (default True): generation 6 first
# (csrc/msda_heads.hip: value in blocks of a full head, one workgroup per CU).


def _shape_list(spatial_shapes):
    return spatial_shapes.tolist() if isinstance(spatial_shapes, torch.Tensor) else list(spatial_shapes)


class MSDeformAttn(nn.Module):
    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4):
        super().__init__()
        if d_model % n_heads != 0:
            raise ValueError(f"d_model must be divisible by n_heads, but got {d_model} and {n_heads}")
        self.im2col_step = 128
        self.d_model, self.n_levels, self.n_heads, self.n_points = d_model, n_levels, n_heads, n_points
        self.sampling_offsets = nn.Linear(d_model, n_heads * n_levels * n_points * 2)
        self.attention_weights = nn.Linear(d_model, n_heads * n_levels * n_points)
        self.value_proj = nn.Linear(d_model, d_model)
        self.output_proj = nn.Linear(d_model, d_model)

    def _merged_query_proj(self):
        so, aw = self.sampling_offsets, self.attention_weights
        key = (so.weight.data_ptr(), so.weight._version, aw.weight.data_ptr(), aw.weight._version,
               so.bias._version, aw.bias._version, so.weight.device)
        c = getattr(self, "_qproj_cache", None)
        if c is None or c[0] != key:
            with torch.no_grad():
                c = (key, torch.cat([so.weight, aw.weight]).contiguous(), torch.cat([so.bias, aw.bias]).contiguous())
            self._qproj_cache = c
        return c[1], c[2], so.weight.shape[0]

    def _head_major_query_proj(self, order):
        """The merged projection with its rows permuted to [head][point][L offset pairs, L logits], levels in `order`
        (ops.msda_level_order): its blocked output is the strips kernel's projection operand."""
        so, aw = self.sampling_offsets, self.attention_weights
        key = (so.weight.data_ptr(), so.weight._version, aw.weight.data_ptr(), aw.weight._version,
               so.bias._version, aw.bias._version, so.weight.device, order)
        c = getattr(self, "_qproj_hm_cache", None)
        if c is None or c[0] != key:
            M, L, P = self.n_heads, self.n_levels, self.n_points
            n_off = M * L * P * 2
            idx = []
            for m in range(M):
                for p in range(P):
                    idx += [((m * L + l) * P + p) * 2 + xy for l in order for xy in (0, 1)]
                    idx += [n_off + (m * L + l) * P + p for l in order]
            with torch.no_grad():
                ix = torch.tensor(idx, dtype=torch.long, device=so.weight.device)
                w = torch.cat([so.weight, aw.weight])[ix].contiguous()
                b = torch.cat([so.bias, aw.bias])[ix].contiguous()
            c = (key, w, b)
            self._qproj_hm_cache = c
        return c[1], c[2]

    def pair_applies(self, src, pos, ref_per_query, padding_mask=None):
        """True where `forward(None, ..., query_pos=pos)` projects `src` and `src + pos` in one launch (SWITCHES.encoder_pair;
        encoder_ops.linear_pair_blocked): where the generation-6 head-major path applies today -- its two `ops.linear_blocked` cover the
        rows -- and `pos` is one frame's table.  The caller then has no use for `src + pos` as a tensor.  (`src`: any tensor of the
        input's device and dtype with the frames in front, the NCHW maps included.)"""
        return (SWITCHES.encoder_pair and SWITCHES.msda_strips and SWITCHES.msda_heads and ref_per_query is not None and pos is not None
                and pos.dim() == 3 and int(src.shape[0]) * int(pos.shape[1]) >= encoder_ops.HEAD_MAJOR_MIN_ROWS
                and src.is_cuda and src.dtype == torch.float32 and pos.dtype == torch.float32 and pos.dim() == 3 and pos.shape[0] == 1
                and self.n_points == 4 and self.n_levels <= 4 and padding_mask is None and self.d_model == 32 * self.n_heads == 256
                and ops._resident_presplit(self.value_proj.weight, 256)
                and not ops.needs_grad(src, pos, self.value_proj.weight, self.sampling_offsets.weight, self.attention_weights.weight))

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes,
                input_level_start_index, input_padding_mask=None, ref_per_query=None, residual=None, query_pos=None):
        """query [N,Lq,C]; reference_points [N|1,Lq,L,2]; input_flatten [N,S,C];
        input_spatial_shapes / input_level_start_index: python lists (or tensors).
        `query` None with `query_pos` [1, Lq, C]: the query is `input_flatten + query_pos` (self-attention of the encoder), formed
        inside the projection where `pair_applies`, as a tensor otherwise.
        `ref_per_query` [N|1, Lq, 2] (optional): the caller's promise that every level shares one reference point per query
        (the encoder's pixel centres, msdeformattn.py:143-158 with valid_ratio == 1) -- enables the head-major kernel.
        `residual` [N, Lq, C] (optional): added to the result in `output_proj`'s epilogue (the layer's `src + self_attn(...)`)."""
        pair = query is None and self.pair_applies(input_flatten, query_pos, ref_per_query, input_padding_mask)
        if query is None and not pair:
            query = input_flatten + query_pos
        N, Len_q, _ = input_flatten.shape if query is None else query.shape
        _, Len_in, _ = input_flatten.shape
        M, L, P = self.n_heads, self.n_levels, self.n_points
        like = input_flatten if query is None else query
        if (SWITCHES.msda_strips and ref_per_query is not None and like.is_cuda and P == 4 and L <= 4 and Len_q == Len_in
                and input_padding_mask is None and self.d_model == 32 * M and like.dtype == torch.float32):
            shapes = _shape_list(input_spatial_shapes)
            order = tuple(ops.msda_level_order(shapes))
            w_hm, b_hm = self._head_major_query_proj(order)
            qp_hm = value_hm = None
            if pair:
                # both projections from one read of the input, `input_flatten + query_pos` summed in registers (csrc/linear_pair_f16x3.hip)
                both = encoder_ops.linear_pair_blocked(input_flatten, query_pos, self.value_proj.weight, self.value_proj.bias, 32,
                                                       w_hm, b_hm, 3 * L * P)
                if both is not None:
                    value_hm, qp_hm = both
                else:
                    query = input_flatten + query_pos
            if qp_hm is None:
                qp_hm = ops.linear_blocked(query, w_hm, b_hm, Len_q, 3 * L * P)
            if qp_hm is not None and SWITCHES.msda_heads:
                # generation 6 (csrc/msda_heads.hip): value in blocks of one head, a lane owns a sample of a full head
                if value_hm is None:
                    value_hm = ops.linear_blocked(input_flatten, self.value_proj.weight, self.value_proj.bias, Len_in, 32)
                if value_hm is not None:
                    output = ops.msda_forward_heads(value_hm, qp_hm, ref_per_query, shapes, input_level_start_index, M, P)
                    if output is not None:
                        return self._project(output, residual)
            if qp_hm is not None:
                value_hm = ops.linear_blocked(input_flatten, self.value_proj.weight, self.value_proj.bias, Len_in, 16)
                if value_hm is not None:
                    output = ops.msda_forward_strips(value_hm, qp_hm, ref_per_query, shapes, input_level_start_index, M, P)
                    if output is not None:
                        return self._project(output, residual)
        if query is None:
            query = input_flatten + query_pos
        value = linear(input_flatten, self.value_proj.weight, self.value_proj.bias)
        if input_padding_mask is not None:
            value = value.masked_fill(input_padding_mask[..., None], float(0))
        value = value.view(N, Len_in, M, self.d_model // M)
        # one GEMM for the two Linears that read `query` (their weights concatenated once): 288 output columns
        # instead of 192 + 96, `query` is read once
        w, b, n_off = self._merged_query_proj()
        qp = linear(query, w, b)
        if reference_points.shape[-1] == 2 and P == 4 and L <= 4:
            # softmax over the L*P logits + reference point + offset / (W_l, H_l): one pass (HIP operator)
            sampling_locations, attention_weights = ops.msda_prepare(qp, n_off, reference_points, input_spatial_shapes,
                                                                     M, L, P)
        else:
            sampling_offsets = qp[..., :n_off].view(N, Len_q, M, L, P, 2)
            attention_weights = F.softmax(qp[..., n_off:].reshape(N, Len_q, M, L * P), -1).view(N, Len_q, M, L, P)
            if reference_points.shape[-1] == 2:
                normalizer = torch.tensor([[w_, h_] for (h_, w_) in _shape_list(input_spatial_shapes)], dtype=query.dtype,
                                          device=query.device)
                sampling_locations = reference_points[:, :, None, :, None, :] \
                    + sampling_offsets / normalizer[None, None, None, :, None, :]
            elif reference_points.shape[-1] == 4:
                sampling_locations = reference_points[:, :, None, :, None, :2] \
                    + sampling_offsets / P * reference_points[:, :, None, :, None, 2:] * 0.5
            else:
                raise ValueError(f"Last dim of reference_points must be 2 or 4, but get {reference_points.shape[-1]} instead.")
        output = ops.ms_deform_attn_forward(value.contiguous(), input_spatial_shapes, input_level_start_index,
                                            sampling_locations.contiguous(), attention_weights.contiguous(),
                                            self.im2col_step)
        return self._project(output, residual)

    def _project(self, output, residual):
        w, b = self.output_proj.weight, self.output_proj.bias
        if residual is None:
            return linear(output, w, b)
        y = ops.linear_fused(output, w, b, residual=residual) if (SWITCHES.split_linear and output.is_cuda) else None
        return y if y is not None else residual + linear(output, w, b)


class MSDeformAttnTransformerEncoderLayer(nn.Module):
    def __init__(self, d_model=256, d_ffn=1024, dropout=0.1, activation="relu", n_levels=4, n_heads=8, n_points=4):
        super().__init__()
        self.self_attn = MSDeformAttn(d_model, n_levels, n_heads, n_points)
        self.norm1 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.activation = get_activation_fn(activation)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.norm2 = nn.LayerNorm(d_model)

    def forward(self, src, pos, reference_points, spatial_shapes, level_start_index, padding_mask=None, query=None,
                want_next_query=False, ref_per_query=None):
        """`query` = `src + pos` when the caller already has it (the previous layer's norm2 pass made it);
        `want_next_query`: also return `out + pos` for the next layer (same pass as norm2); `ref_per_query`: see
        MSDeformAttn.forward."""
        # the attention forms `src + pos` inside its projections: no query tensor here, none asked of the FFN kernel for the next layer
        pair = self.self_attn.pair_applies(src, pos, ref_per_query, padding_mask)
        query_pos = None
        if pair:
            query, query_pos, want_pos = None, pos, False
        else:
            want_pos = want_next_query and pos is not None
            if query is None:
                query = src if pos is None else src + pos
        fused = SWITCHES.fused_mlp and SWITCHES.split_linear and src.is_cuda and self.activation is F.relu
        if fused and SWITCHES.fused_norm1 and not torch.is_grad_enabled() and src.dtype == torch.float32:
            # `src + self_attn(...)` from output_proj's epilogue, then norm1 + linear1 + ReLU + linear2 + residual + norm2 (+ the next
            # layer's `src + pos`) in ONE kernel: norm1 is evaluated on the x tile in registers and is also the FFN's residual
            # (csrc/mlp_f16x3.hip: res_normed)
            sum1 = self.self_attn(query, reference_points, src, spatial_shapes, level_start_index, padding_mask,
                                  ref_per_query=ref_per_query, residual=src, query_pos=query_pos)
            n1, n2 = (self.norm1.weight, self.norm1.bias, self.norm1.eps), (self.norm2.weight, self.norm2.bias, self.norm2.eps)
            with_next = want_pos
            res = ops.mlp_fused(sum1, self.linear1.weight, self.linear1.bias, self.linear2.weight, self.linear2.bias, "relu",
                                ln=n1, residual_normed=True, post_ln=n2, post_add=pos if with_next else None)
            if res is not None:
                if with_next:
                    return res
                return (res, None) if want_next_query else res
            src = layer_norm(self.norm1, sum1)
        else:
            src2 = self.self_attn(query, reference_points, src, spatial_shapes, level_start_index, padding_mask,
                                  ref_per_query=ref_per_query, query_pos=query_pos)
            src = layer_norm(self.norm1, src2, residual=src)
        ffn = None
        if fused:
            # linear1 + ReLU + linear2 + residual + norm2 (+ the next layer's `src + pos`) in ONE kernel: the [tokens, d_ffn]
            # activations stay in registers and the finished row is normalised before it is stored (csrc/mlp_f16x3.hip)
            n2 = (self.norm2.weight, self.norm2.bias, self.norm2.eps)
            with_next = want_pos
            res = ops.mlp_fused(src, self.linear1.weight, self.linear1.bias, self.linear2.weight, self.linear2.bias, "relu",
                                residual=src, post_ln=n2, post_add=pos if with_next else None)
            if res is not None:
                if with_next:
                    return res
                return (res, None) if want_next_query else res
        if ffn is None:
            ffn = linear(linear_act(src, self.linear1, self.activation), self.linear2.weight, self.linear2.bias)
        if want_pos and src.is_cuda:
            return layer_norm(self.norm2, ffn, residual=src, post_add=pos)
        src = layer_norm(self.norm2, ffn, residual=src)
        return (src, None) if want_next_query else src


class MSDeformAttnTransformerEncoder(nn.Module):
    def __init__(self, d_model, d_ffn, dropout, activation, n_levels, n_heads, n_points, num_layers):
        super().__init__()
        self.layers = nn.ModuleList([
            MSDeformAttnTransformerEncoderLayer(d_model, d_ffn, dropout, activation, n_levels, n_heads, n_points)
            for _ in range(num_layers)])
        self.num_layers = num_layers

    @staticmethod
    def get_reference_points(spatial_shapes, device):
        """Pixel centres normalised per level, valid_ratio == 1 (msdeformattn.py:143-158): [1, S, L, 2]."""
        refs = []
        for (H_, W_) in spatial_shapes:
            ref_y, ref_x = torch.meshgrid(
                torch.linspace(0.5, H_ - 0.5, H_, dtype=torch.float32, device=device),
                torch.linspace(0.5, W_ - 0.5, W_, dtype=torch.float32, device=device), indexing="ij")
            ref_y = ref_y.reshape(-1)[None] / H_
            ref_x = ref_x.reshape(-1)[None] / W_
            refs.append(torch.stack((ref_x, ref_y), -1))
        reference_points = torch.cat(refs, 1)
        return reference_points[:, :, None].expand(-1, -1, len(spatial_shapes), -1).contiguous()

    def forward(self, src, spatial_shapes, level_start_index, reference_points, pos=None, ref_per_query=None, query=None):
        """`query`: `src + pos` for the first layer when the caller already has it"""
        output = src
        for i, layer in enumerate(self.layers):
            if i + 1 < self.num_layers:
                output, query = layer(output, pos, reference_points, spatial_shapes, level_start_index, None, query=query,
                                      want_next_query=True, ref_per_query=ref_per_query)
            else:
                output = layer(output, pos, reference_points, spatial_shapes, level_start_index, None, query=query,
                               ref_per_query=ref_per_query)
        return output


class MSDeformAttnTransformerEncoderOnly(nn.Module):
    def __init__(self, d_model=256, nhead=8, num_encoder_layers=6, dim_feedforward=1024, dropout=0.1,
                 activation="relu", num_feature_levels=4, enc_n_points=4):
        super().__init__()
        self.d_model, self.nhead = d_model, nhead
        self.encoder = MSDeformAttnTransformerEncoder(d_model, dim_feedforward, dropout, activation,
                                                      num_feature_levels, nhead, enc_n_points, num_encoder_layers)
        self.level_embed = nn.Parameter(torch.Tensor(num_feature_levels, d_model))
        nn.init.normal_(self.level_embed)
        self._ref_cache = {}

    def forward(self, srcs, pos_embeds, affines=None):
        """`affines` (optional, GPU inference): srcs are the RAW input-projection convolutions and affines[l] the per-plane (scale, bias)
        of their GroupNorm (ops.group_norm_affine) -- applied while the level is written into the encoder input."""
        spatial_shapes = [(int(s.shape[2]), int(s.shape[3])) for s in srcs]
        level_start_index, acc = [], 0
        for (h, w) in spatial_shapes:
            level_start_index.append(acc)
            acc += h * w
        # position embedding + level embedding: a function of the shapes and of one parameter (cached with its version)
        le = self.level_embed
        pkey = (tuple(spatial_shapes), tuple(int(p.shape[0]) for p in pos_embeds), str(srcs[0].device), le._version, le.data_ptr(),
                tuple(p.data_ptr() for p in pos_embeds))
        pc = self.__dict__.get("_lvl_pos_cache")
        if pc is not None and pc[0] == pkey and not torch.is_grad_enabled():
            lvl_pos = pc[1]
        else:
            lvl_pos = torch.cat([p.flatten(2).transpose(1, 2) + le[lvl].view(1, 1, -1) for lvl, p in enumerate(pos_embeds)], 1)
            if not torch.is_grad_enabled():
                self.__dict__["_lvl_pos_cache"] = (pkey, lvl_pos, list(pos_embeds))     # (the embeddings are kept alive with their addresses)
        query0 = None
        fast = None
        # (where the first layer forms `src + pos` inside its projections, the second output is not asked for)
        pair0 = srcs[0].is_cuda and lvl_pos.shape[0] == 1 and self.encoder.layers[0].self_attn.pair_applies(srcs[0], lvl_pos, True)
        if srcs[0].is_cuda and not torch.is_grad_enabled() and lvl_pos.shape[0] == 1:
            # NCHW -> tokens per level by the LDS tile transpose, written straight into the concatenated tensor, GroupNorm applied on
            # the way in, `src + pos` for the first layer as a second output: one launch per level (a concatenation of transposed views
            # runs at 0.6 TB/s: 175 us for the 99 MB of a 720p clip)
            fast = ops.tokens_from_nchw(srcs, affines if affines is not None else [None] * len(srcs), None if pair0 else lvl_pos.contiguous())
        if fast is not None:
            src_flatten, query0 = fast
        else:
            if affines is not None:
                srcs = [s if a is None else s * a[:, 0].view(s.shape[0], s.shape[1], 1, 1) + a[:, 1].view(s.shape[0], s.shape[1], 1, 1)
                        for s, a in zip(srcs, affines)]
            if srcs[0].is_cuda and not torch.is_grad_enabled():
                src_flatten = torch.cat([ops.transpose_last2(s.flatten(2).contiguous()) for s in srcs], 1)
            else:
                src_flatten = torch.cat([s.flatten(2).transpose(1, 2) for s in srcs], 1)
        key = (tuple(spatial_shapes), str(src_flatten.device))
        ref = self._ref_cache.get(key)
        if ref is None:
            if len(self._ref_cache) > 8:
                self._ref_cache.clear()
            r = MSDeformAttnTransformerEncoder.get_reference_points(spatial_shapes, src_flatten.device)
            # get_reference_points expands ONE point per query over the levels (valid_ratio == 1): keep that point too
            ref = (r, r[:, :, 0].contiguous())
            self._ref_cache[key] = ref
        memory = self.encoder(src_flatten, spatial_shapes, level_start_index, ref[0], lvl_pos, ref_per_query=ref[1], query=query0)
        return memory, spatial_shapes, level_start_index


@SEM_SEG_HEADS_REGISTRY.register()
class MSDeformAttnPixelDecoder(nn.Module):
    @configurable
    def __init__(self, input_shape: Dict[str, ShapeSpec], *, transformer_dropout: float, transformer_nheads: int,
                 transformer_dim_feedforward: int, transformer_enc_layers: int, conv_dim: int, mask_dim: int,
                 norm: Optional[Union[str, Callable]] = None, transformer_in_features: List[str],
                 common_stride: int):
        super().__init__()
        transformer_input_shape = {k: v for k, v in input_shape.items() if k in transformer_in_features}
        input_shape = sorted(input_shape.items(), key=lambda x: x[1].stride)
        self.in_features = [k for k, v in input_shape]
        self.feature_strides = [v.stride for k, v in input_shape]
        self.feature_channels = [v.channels for k, v in input_shape]
        transformer_input_shape = sorted(transformer_input_shape.items(), key=lambda x: x[1].stride)
        self.transformer_in_features = [k for k, v in transformer_input_shape]
        transformer_in_channels = [v.channels for k, v in transformer_input_shape]
        self.transformer_feature_strides = [v.stride for k, v in transformer_input_shape]
        self.transformer_num_feature_levels = len(self.transformer_in_features)
        chans = transformer_in_channels[::-1] if self.transformer_num_feature_levels > 1 else [transformer_in_channels[-1]]
        self.input_proj = nn.ModuleList([
            nn.Sequential(nn.Conv2d(c, conv_dim, kernel_size=1), nn.GroupNorm(32, conv_dim)) for c in chans])
        self.transformer = MSDeformAttnTransformerEncoderOnly(
            d_model=conv_dim, dropout=transformer_dropout, nhead=transformer_nheads,
            dim_feedforward=transformer_dim_feedforward, num_encoder_layers=transformer_enc_layers,
            num_feature_levels=self.transformer_num_feature_levels)
        self.pe_layer = PositionEmbeddingSine(conv_dim // 2, normalize=True)
        self.mask_dim = mask_dim
        self.mask_features = Conv2d(conv_dim, mask_dim, kernel_size=1, stride=1, padding=0)
        self.maskformer_num_feature_levels = 3
        self.common_stride = common_stride
        stride = min(self.transformer_feature_strides)
        self.num_fpn_levels = int(np.log2(stride) - np.log2(self.common_stride))
        lateral_convs, output_convs = [], []
        use_bias = norm == ""
        for idx, in_channels in enumerate(self.feature_channels[:self.num_fpn_levels]):
            lateral_conv = Conv2d(in_channels, conv_dim, kernel_size=1, bias=use_bias, norm=get_norm(norm, conv_dim))
            output_conv = Conv2d(conv_dim, conv_dim, kernel_size=3, stride=1, padding=1, bias=use_bias,
                                 norm=get_norm(norm, conv_dim), activation=F.relu)
            self.add_module(f"adapter_{idx + 1}", lateral_conv)
            self.add_module(f"layer_{idx + 1}", output_conv)
            lateral_convs.append(lateral_conv)
            output_convs.append(output_conv)
        self.lateral_convs = lateral_convs[::-1]
        self.output_convs = output_convs[::-1]
        self._pe_cache = {}

    @classmethod
    def from_config(cls, cfg, input_shape: Dict[str, ShapeSpec]):
        ret = {}
        ret["input_shape"] = {k: v for k, v in input_shape.items() if k in cfg.MODEL.SEM_SEG_HEAD.IN_FEATURES}
        ret["conv_dim"] = cfg.MODEL.SEM_SEG_HEAD.CONVS_DIM
        ret["mask_dim"] = cfg.MODEL.SEM_SEG_HEAD.MASK_DIM
        ret["norm"] = cfg.MODEL.SEM_SEG_HEAD.NORM
        ret["transformer_dropout"] = cfg.MODEL.MASK_FORMER.DROPOUT
        ret["transformer_nheads"] = cfg.MODEL.MASK_FORMER.NHEADS
        ret["transformer_dim_feedforward"] = 1024  # fixed for the deformable encoder (msdeformattn.py:307)
        ret["transformer_enc_layers"] = cfg.MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS
        ret["transformer_in_features"] = cfg.MODEL.SEM_SEG_HEAD.DEFORMABLE_TRANSFORMER_ENCODER_IN_FEATURES
        ret["common_stride"] = cfg.MODEL.SEM_SEG_HEAD.COMMON_STRIDE
        return ret

    def _pos(self, x):
        key = (tuple(x.shape[-2:]), str(x.device))
        p = self._pe_cache.get(key)
        if p is None:
            if len(self._pe_cache) > 16:
                self._pe_cache.clear()
            p = self.pe_layer(x[:1])  # [1, C, H, W]; identical for every frame
            self._pe_cache[key] = p
        return p

    @contextlib.contextmanager
    def normed_optional(self):
        """Inside the block `forward_features(features)` may return None as its second element: for the callers that hand it to a
        predictor which ignores it (MaskFormerHead.layers, inference/video_entity.py).  The mask-feature convolution then normalises
        its operand while loading it (SWITCHES.fold_fpn_norm) and the normalised tensor is never written.  The call itself keeps its
        one-argument form: drop-in callers and wrappers of it are not concerned."""
        old = self.__dict__.get("_normed_optional", False)
        self.__dict__["_normed_optional"] = True
        try:
            yield self
        finally:
            self.__dict__["_normed_optional"] = old

    def forward_features(self, features):
        """(mask_features, the normalised FPN output they are computed from, the coarsest encoder level, multi_scale_features); the
        second is the correct tensor, or None inside `normed_optional()` -- never anything else."""
        want_normed = not self.__dict__.get("_normed_optional", False)
        with torch.autocast(device_type=next(iter(features.values())).device.type, enabled=False):
            if SWITCHES.graphs and not self.training and all(f.is_cuda for f in features.values()):
                # hipGraph replay per input signature (univs_amd/graphs.py): one launch instead of ~200
                g = self.__dict__.get("_graphed")
                if g is None:
                    from ...graphs import GraphedCallable
                    g = self.__dict__["_graphed"] = GraphedCallable(self._forward_features)
                return g({k: features[k] for k in self.in_features}, bool(want_normed))
            return self._forward_features(features, want_normed)

    @staticmethod
    def _conv1x1_in_place(conv, x):
        """The 1 x 1 convolution `conv` (no norm, no activation) of a backbone feature that is a channels-last VIEW of its token tensor
        (SwinTransformer, SWITCHES.swin_channels_last), read where it lies -> (y NCHW or None, x).  Where the kernel does not cover the
        call, x comes back as the contiguous NCHW tensor the other paths take, made by the LDS tile transpose: handed on as the view it
        would be copied by ATen's generic strided kernel at the first `.contiguous()` (0.6 TB/s)."""
        if not x.is_cuda or x.is_contiguous() or not x.is_contiguous(memory_format=torch.channels_last):
            return None, x
        y = None
        if SWITCHES.split_conv and x.dtype == torch.float32 and not ops.needs_grad(x, conv.weight, conv.bias):
            y = fused_ops.conv1x1_fused(x, conv.weight, conv.bias)
        if y is None:
            T, C, H, W = x.shape
            tokens = x.permute(0, 2, 3, 1).reshape(T, H * W, C)       # (a view: x is channels last)
            x = ops.transpose_last2(tokens).view(T, C, H, W) if not ops.needs_grad(x) else x.contiguous()
        return y, x

    def _input_proj(self, idx, x):
        """input_proj[idx] = Sequential(Conv2d 1 x 1, GroupNorm(32)) (msdeformattn.py:205-212) through the HIP operators (the
        modules only hold the parameters; plain nn.Conv2d / nn.GroupNorm would take MIOpen + ATen)."""
        conv, gn = self.input_proj[idx][0], self.input_proj[idx][1]
        if x.is_cuda and x.dtype == torch.float32 and not ops.needs_grad(x, conv.weight):
            y = ops.conv1x1(x, conv.weight, conv.bias) if SWITCHES.split_conv else None
            if y is None:
                y = conv(x)
            return ops.group_norm(y, gn.num_groups, gn.weight, gn.bias, gn.eps)
        return self.input_proj[idx](x)

    def _forward_features(self, features, want_normed=True):
        srcs, pos, affines = [], [], []
        for idx, f in enumerate(self.transformer_in_features[::-1]):
            x = features[f].float()
            conv, gn = self.input_proj[idx][0], self.input_proj[idx][1]
            raw, x = self._conv1x1_in_place(conv, x)
            if x.is_cuda and not torch.is_grad_enabled() and not ops.needs_grad(x, conv.weight):
                # the convolution alone + its GroupNorm in affine form: the normalisation is applied where the level is written into
                # the encoder input (ops.tokens_from_nchw), not by a pass of its own
                if raw is None:
                    raw = ops.conv1x1(x, conv.weight, conv.bias) if SWITCHES.split_conv else None
                raw = conv(x) if raw is None else raw
                srcs.append(raw)
                affines.append(ops.group_norm_affine(raw, gn.num_groups, gn.weight, gn.bias, gn.eps))
            else:
                srcs.append(self._input_proj(idx, x))
                affines.append(None)
            pos.append(self._pos(x))
        if all(a is None for a in affines):
            y, spatial_shapes, level_start_index = self.transformer(srcs, pos)
        else:
            y, spatial_shapes, level_start_index = self.transformer(srcs, pos, affines)
        bs = y.shape[0]
        sizes = [h * w for (h, w) in spatial_shapes]
        y = torch.split(y, sizes, dim=1)
        # tokens [T, S_l, C] -> NCHW, contiguous: an LDS tile transpose per level on the GPU (a strided view would be copied
        # by ATen's generic kernel at the first consumer: 110 us for the 1/8 level instead of 22)
        if y[0].is_cuda:
            out = [ops.transpose_last2(z).view(bs, -1, spatial_shapes[i][0], spatial_shapes[i][1]) for i, z in enumerate(y)]   # (a row range: no copy)
        else:
            out = [z.transpose(1, 2).reshape(bs, -1, spatial_shapes[i][0], spatial_shapes[i][1]) for i, z in enumerate(y)]
        normed, folded = None, None
        for idx, f in enumerate(self.in_features[:self.num_fpn_levels][::-1]):
            x = features[f].float()
            lat = self.lateral_convs[idx]
            y_ = None
            raw_in_place, x = self._conv1x1_in_place(lat, x)
            if (x.is_cuda and isinstance(lat.norm, nn.GroupNorm) and lat.activation is None and not torch.is_grad_enabled()
                    and x.shape[-2] == 2 * out[-1].shape[-2] and x.shape[-1] == 2 * out[-1].shape[-1]):
                # lateral 1 x 1 convolution, GroupNorm statistics, then `GroupNorm(lateral) + upsample(coarser)` in one pass that
                # normalises the convolution output while reading it (csrc/resample.hip: upsample2x_add_kernel)
                raw = raw_in_place if raw_in_place is not None else lat.convolve(x)
                y_ = ops.upsample2x_add(out[-1], raw, ops.group_norm_affine(raw, lat.norm.num_groups, lat.norm.weight, lat.norm.bias,
                                                                          lat.norm.eps))
                if y_ is None:
                    cur_fpn = ops.group_norm(raw, lat.norm.num_groups, lat.norm.weight, lat.norm.bias, lat.norm.eps)
                    y_ = ops.bilinear_resample(out[-1], cur_fpn.shape[-2:], addend=cur_fpn)
            if y_ is None:
                cur_fpn = lat(x)
                y_ = ops.bilinear_resample(out[-1], cur_fpn.shape[-2:], addend=cur_fpn)
            oc = self.output_convs[idx]
            if (idx + 1 == self.num_fpn_levels and not want_normed and SWITCHES.fold_fpn_norm and SWITCHES.split_conv and y_.is_cuda
                    and y_.dtype == torch.float32 and len(out) >= self.maskformer_num_feature_levels
                    and isinstance(oc.norm, nn.GroupNorm) and oc.activation is F.relu and not torch.is_grad_enabled()
                    and self.mask_features.norm is None and self.mask_features.activation is None):
                # the last FPN level, whose normalised output only the mask-feature convolution reads: the 3 x 3 convolution alone, its
                # GroupNorm as per-plane (scale, bias), and the 1 x 1 applies relu(fma(x, scale, bias)) while it loads x
                raw = oc.convolve(y_)
                affine = ops.group_norm_affine(raw, oc.norm.num_groups, oc.norm.weight, oc.norm.bias, oc.norm.eps)
                folded = fused_ops.conv1x1_fused(raw, self.mask_features.weight, self.mask_features.bias, affine)
                if folded is None:                         # (not covered: the pass of its own)
                    normed = ops.group_norm(raw, oc.norm.num_groups, oc.norm.weight, oc.norm.bias, oc.norm.eps, relu=True)
                out.append(normed)                         # (None when folded: nothing below reads out[-1])
                continue
            out.append(oc(y_))
        multi_scale_features = out[:self.maskformer_num_feature_levels]
        if folded is not None:
            return folded, None, out[0], multi_scale_features
        return self.mask_features(out[-1]), out[-1], out[0], multi_scale_features
