"""GPU: csrc/semantic_decode.hip against the logits that the exact-f32 `ops.mask_decode` STORES (the counts must be that tensor's counts,
exactly), its strict comparisons, its zeroing and its order-independence; then the module (inference/semantic_to_mask.py) on the device
against what the reference returned (golden g31_semantic_decode_*), fused against ATen, and the round trip through the two files of the
extraction driver.  Nothing here reads the reference."""
import itertools

import numpy as np
import pytest
import torch

from tests import semantic_decode_cases as sc
from tests.test_semantic_extraction_cpu import driver
from univs_amd import _lib, ops, semantic_ops
from univs_amd.inference import semantic_to_mask as stm
from univs_amd.workloads import SemanticClipHead

pytestmark = pytest.mark.gpu

NS, HWS, CS, FRAMES = (1, 33, 37, 65), (30, 255, 257, 880), (64, 256), ((7, 3), (6, 3), (4, 1), (2, 10))


def operands(T, N, C, HW, seed, cuda):
    """mask_embed [T, N, C] ~ N(0, 1) and features [T, C, HW] ~ N(0, 4 / C): logits of deviation 2, which both +1 and -1 split."""
    g = torch.Generator().manual_seed(seed)
    me = torch.randn(T, N, C, generator=g)
    feats = torch.randn(T, C, HW, generator=g) * (2.0 / np.sqrt(C))
    return me.to(cuda), feats.to(cuda)


def stored_counts(me, feats, s, t_hi=1.0, t_lo=-1.0):
    """The counts of the logits that ops.mask_decode stores under the exact-f32 setting: (int64 [N, 2], the walked logits)."""
    with ops.configured(mask_decode_impl=1):
        L = ops.mask_decode(me, feats.unsqueeze(-1))                 # [N, T, HW, 1]
        assert ops.mask_decode_last_impl() == 1
    W = L[:, ::s]
    return torch.stack([(W > t_hi).flatten(1).sum(-1), (W > t_lo).flatten(1).sum(-1)], dim=1), W


@pytest.mark.parametrize("N,HW,C,frames", list(itertools.product(NS, HWS, CS, FRAMES)))
def test_counts_are_the_stored_logits_counts(cuda, N, HW, C, frames):
    T, s = frames
    me, feats = operands(T, N, C, HW, 7 * N + HW + C + T, cuda)
    got = semantic_ops.semantic_quality_counts(me, feats, s)
    assert got is not None and got.dtype == torch.int32 and tuple(got.shape) == (N, 2)
    want, W = stored_counts(me, feats, s)
    per_row = W[0].numel()
    print(f"walked logits per row {per_row}; > 1: {int(want[:, 0].sum())}, > -1: {int(want[:, 1].sum())} of {W.numel()}; "
          f"max |kernel - stored| = {int((got.long() - want).abs().max())}")
    assert torch.equal(got.long(), want)
    assert 0 < int(want[:, 0].sum()) < int(want[:, 1].sum()) < W.numel()       # both thresholds split the logits
    assert per_row == len(range(0, T, s)) * HW


@pytest.mark.parametrize("N,T,HW,C", [(40, 12, 4096, 64), (70, 12, 4096, 64), (129, 12, 2048, 64)])
def test_counts_with_two_three_and_four_row_blocks_per_workgroup(cuda, N, T, HW, C):
    """Beyond the small shapes: the launcher gives a workgroup 64, 96 or 128 rows only when at least 192 workgroups remain, so the three
    wider instantiations of the kernel need 12 frames of 2048-4096 pixels to run at all (a 13 MB logit tensor for the comparison)."""
    me, feats = operands(T, N, C, HW, N, cuda)
    got = semantic_ops.semantic_quality_counts(me, feats, 1)
    want, W = stored_counts(me, feats, 1)
    assert got is not None and torch.equal(got.long(), want)
    assert 0 < int(want[:, 0].sum()) < int(want[:, 1].sum()) < W.numel()
    got3 = semantic_ops.semantic_quality_counts(me, feats, 5)       # frames 0, 5, 10: fewer workgroups, a narrower tile
    assert torch.equal(got3.long(), stored_counts(me, feats, 5)[0])


@pytest.mark.parametrize("C,HW", [(64, 257), (256, 257), (256, 30)])
def test_comparisons_are_strict(cuda, C, HW):
    """One-hot rows of mask_embed pick one channel each; the features hold exactly +-1.0 and +-1.5: the logits ARE those values (every
    other term of the chain is an exact zero), and the ones equal to a threshold are not counted."""
    T, N, s = 4, 37, 3
    rs = np.random.RandomState(C + HW)
    values = np.array([-1.5, -1.0, 1.0, 1.5], dtype=np.float32)
    feats = values[rs.randint(0, 4, (T, C, HW))]
    chan = rs.randint(0, C, (T, N))
    me = np.zeros((T, N, C), dtype=np.float32)
    for t in range(T):
        me[t, np.arange(N), chan[t]] = 1.0
    picked = np.stack([feats[t, chan[t]] for t in range(0, T, s)], axis=1)          # [N, frames, HW]: the logits
    want = np.stack([(picked == 1.5).reshape(N, -1).sum(-1), (picked >= 1.0).reshape(N, -1).sum(-1)], axis=1)
    assert (picked == 1.0).any() and (picked == -1.0).any()
    got = semantic_ops.semantic_quality_counts(torch.from_numpy(me).to(cuda), torch.from_numpy(feats).to(cuda), s)
    assert got.cpu().tolist() == want.tolist()
    got = semantic_ops.semantic_quality_counts(torch.from_numpy(me).to(cuda), torch.from_numpy(feats).to(cuda), s, t_hi=-1.0, t_lo=-1.5)
    want = np.stack([(picked >= 1.0).reshape(N, -1).sum(-1), (picked >= -1.0).reshape(N, -1).sum(-1)], axis=1)
    assert got.cpu().tolist() == want.tolist()


@pytest.mark.parametrize("N,HW,C,frames", [(65, 880, 256, (7, 3)), (37, 257, 64, (6, 3))])
def test_two_calls_agree_and_the_entry_zeroes_its_output(cuda, N, HW, C, frames):
    T, s = frames
    me, feats = operands(T, N, C, HW, 11, cuda)
    first = semantic_ops.semantic_quality_counts(me, feats, s)
    second = semantic_ops.semantic_quality_counts(me, feats, s)
    assert torch.equal(first, second)
    stale = torch.full((N, 2), 12345, dtype=torch.int32, device=cuda)
    assert ops._call("test", _lib.load().univs_semantic_quality_counts_f32, me, ops._ptr(me), ops._ptr(feats), T, N, C, HW, s, 1.0, -1.0,
                     ops._ptr(stale))
    assert torch.equal(stale, first) and int(first.sum()) > 0


@pytest.mark.parametrize("case", sc.CASES)
def test_convert_gpu_matches_reference(cuda, case, monkeypatch):
    fx = sc.load(case)
    r = fx["recipe"]
    conv = sc.converter(r, cuda)
    fused = []
    real = semantic_ops.semantic_quality_counts
    monkeypatch.setattr(semantic_ops, "semantic_quality_counts", lambda *a, **k: fused.append(real(*a, **k)) or fused[-1])
    cls_logits, mask_logits, indices = sc.check_against_fixture(conv, fx)
    assert fused and all(c is not None for c in fused)              # the counts came from the kernel
    assert ops.get_config()["mask_decode_impl"] == 0                # the exact-f32 setting was restored
    # the logits returned are the very values that were counted: the exact-f32 decode of the kept rows, bit for bit, which is the
    # exact-f32 decode of ALL rows at those rows
    feats, tokens = sc.inputs(r)
    feats = feats.to(cuda)
    _, mask_embed = conv.heads(tokens.to(cuda))
    with ops.configured(mask_decode_impl=1):
        kept = ops.mask_decode(mask_embed[:, indices].contiguous(), feats)
        every = ops.mask_decode(mask_embed, feats)
    assert torch.equal(mask_logits, kept) and torch.equal(mask_logits, every[indices])
    W = every[:, ::r["stride"]]
    assert torch.stack([(W > 1).flatten(1).sum(-1), (W > -1).flatten(1).sum(-1)], dim=1).cpu().tolist() == fx["counts"].tolist()


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_fused_selection_equals_aten_selection(cuda, case, monkeypatch):
    fx = sc.load(case)
    r = fx["recipe"]
    conv = sc.converter(r, cuda)
    feats, tokens = (x.to(cuda) for x in sc.inputs(r))
    cls_all, mask_embed = conv.heads(tokens)
    _, q_fused, c_fused = conv.scores(cls_all, mask_embed, feats)
    fused = conv.convert(feats, tokens)
    monkeypatch.setattr(semantic_ops, "semantic_quality_counts", lambda *a, **k: None)
    _, q_aten, c_aten = conv.scores(cls_all, mask_embed, feats)
    aten = conv.convert(feats, tokens)
    assert torch.equal(c_fused, c_aten) and torch.equal(q_fused, q_aten) and c_aten.dtype == torch.int32
    assert torch.equal(fused[2], aten[2]) and fused[2].cpu().tolist() == fx["indices"].tolist()
    assert torch.equal(fused[0], aten[0]) and torch.equal(fused[1], aten[1])


def test_round_trip_through_the_extraction_drivers_files(cuda, tmp_path):
    """`InferenceVideoSemanticExtraction.save` writes the two files of a small SemanticClipHead video; the CLI's function reads them back;
    the result equals `convert` on the tensors in memory."""
    r = dict(seed=77, C=256, N=5, h=6, w=8, T=4, text_emb_dim=16, K=1007, cls_scale=4.0, cls_thres=0.5, quality_thres=0.2, stride=3,
             ratio=8, t_itv=1, default_dir=False)
    head = SemanticClipHead(r["seed"], r["C"], r["N"], r["h"], r["w"])
    out = head({"res2": torch.zeros(r["T"], 1)}, targets=[{"first_frame_idx": 0, "frame_indices": torch.arange(r["T"])}])
    tokens, feats = out["pred_embds"].to(cuda), (out["mask_features"] * 0.1).to(cuda)
    d = driver(r, str(tmp_path / "out"), cuda)
    tok_path, feat_path = d.save("vid", ["raw/set/vid/0.jpg"], tokens, feats)
    assert tok_path.endswith("vid._obj_tokens_8_1.pt") and feat_path.endswith("vid._compression_mask_features_8_1.pt")
    ckpt, clip = str(tmp_path / "ckpt.pth"), str(tmp_path / "clip.pth")
    torch.save({"model": sc.checkpoint(r)}, ckpt)
    torch.save(sc.clip_table(r), clip)
    for all_rows in (False, True):
        res = stm.decode_files(tok_path, feat_path, ckpt, clip, out=str(tmp_path / "result.pt"), all_rows=all_rows, device="cuda",
                               **sc.keywords(r))
        want = sc.converter(r, cuda).convert(feats, tokens, only_high_conf_masks=not all_rows)
        saved = torch.load(str(tmp_path / "result.pt"))
        for name, w in zip(("cls_logits", "mask_logits", "indices"), want):
            assert res[name].device.type == "cpu" and res[name].is_contiguous()
            assert torch.equal(res[name], w.cpu()) and torch.equal(saved[name], w.cpu()), name
        assert tuple(res["mask_logits"].shape)[1:] == (r["T"], r["h"], r["w"]) and tuple(res["cls_logits"].shape)[1:] == (r["T"], r["K"])
    assert res["indices"].tolist() == list(range(r["N"]))
