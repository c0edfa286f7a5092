"""CPU: the semantic-feature decoder (univs_amd/inference/semantic_to_mask.py) -- the ATen path of `convert` against what the
reference's own `ConvertSemanticFeatureToMask.convert` returned (golden g31_semantic_decode_*, tools/gen_golden_semantic_decode.py), its
checkpoint rule, the K <= 1000 error, `from_predictor`, the CLI's function, and the ATen counts against the plain expression."""
import logging
import types

import pytest
import torch

from tests import semantic_decode_cases as sc
from univs_amd import semantic_ops
from univs_amd.inference import semantic_to_mask as stm


@pytest.mark.parametrize("case", sc.CASES)
def test_convert_cpu_matches_reference(case):
    fx = sc.load(case)
    conv = sc.converter(fx["recipe"], "cpu")
    cls_logits, mask_logits, indices = sc.check_against_fixture(conv, fx)
    if case == "e":
        r = fx["recipe"]
        assert tuple(cls_logits.shape) == (0, r["T"], r["K"]) and tuple(mask_logits.shape) == (0, r["T"], r["h"], r["w"])
    if case == "d":
        assert indices.tolist() == list(range(fx["recipe"]["N"]))


def test_fixtures_reach_what_they_are_for():
    """Each filter keeps and drops rows in a and c (b has one row, kept by both), d returns all rows, e none; the walked frames."""
    for case in ("a", "c"):
        fx = sc.load(case)
        r = fx["recipe"]
        hc, hq = fx["confidence"] > r["cls_thres"], fx["quality"] > r["quality_thres"]
        assert 0 < hc.sum() < r["N"] and 0 < hq.sum() < r["N"] and 0 < len(fx["indices"]) < r["N"]
    b, d, e = (sc.load(c) for c in "bde")
    assert b["recipe"]["N"] == 1 and b["indices"].tolist() == [0] and b["recipe"]["C"] == 64 and b["recipe"]["h"] * b["recipe"]["w"] == 257
    assert d["indices"].tolist() == list(range(37)) and not d["recipe"]["only_high"]
    assert len(e["indices"]) == 0
    assert [list(range(0, sc.load(c)["recipe"]["T"], sc.load(c)["recipe"]["stride"])) for c in "abc"] == [[0, 3, 6], [0, 3], [0]]


@pytest.mark.parametrize("wrapped", [True, False])
def test_checkpoint_rule(wrapped, caplog):
    """A bare state dict and a {"model": ...} dict both load; the names matched and skipped are the ones the reference printed; the
    skipped parameter (wrong size) keeps its initial value and the unrelated key is ignored; one log record, nothing printed."""
    fx = sc.load("a")
    r = fx["recipe"]
    with caplog.at_level(logging.INFO, logger=stm.__name__):
        conv = sc.converter(r, "cpu", wrapped=wrapped)
    assert conv.matched == fx["matched"] and conv.skipped == fx["skipped"] == ["decoder_norm.bias"]
    assert len([rec for rec in caplog.records if rec.name == stm.__name__]) == 1
    sd, ck = conv.state_dict(), sc.checkpoint(r)
    assert sorted(sd) == sorted(fx["matched"] + fx["skipped"])
    for name in fx["matched"]:
        assert torch.equal(sd[name], ck[stm.PREDICTOR_PREFIX + name]), name
    assert torch.equal(sd["decoder_norm.bias"], torch.zeros(r["C"]))
    matched, skipped = conv.load_pretrained_checkpoint({"decoder_norm.weight": torch.full((r["C"],), 2.0)})
    assert matched == ["decoder_norm.weight"] and len(skipped) == len(sd) - 1 and float(conv.decoder_norm.weight.detach()[0]) == 2.0
    with pytest.raises(ValueError):
        conv.load_pretrained_checkpoint([1, 2])


def test_first_matching_key_wins(tmp_path):
    C = 8
    first, second = torch.full((C,), 3.0), torch.full((C,), 5.0)
    path = tmp_path / "ckpt.pth"
    torch.save({"model": {"sem_seg_head.predictor.decoder_norm.weight": first, "decoder_norm.weight": second}}, path)
    conv = stm.ConvertSemanticFeatureToMask(hidden_dim=C, mask_dim=C, text_emb_dim=4, clip_class_embed_path=torch.randn(1001, 4),
                                            pretrained_ckpt=str(path), device="cpu")
    assert torch.equal(conv.decoder_norm.weight.detach(), first) and conv.matched == ["decoder_norm.weight"]


def test_too_few_classes_raise():
    C = 8
    conv = stm.ConvertSemanticFeatureToMask(hidden_dim=C, mask_dim=C, text_emb_dim=4, clip_class_embed_path=torch.randn(1000, 4),
                                            pretrained_ckpt=None, device="cpu")
    feats, tokens = torch.randn(2, C, 3, 4), torch.randn(2, C, 5)
    with pytest.raises(ValueError, match="K = 1000"):
        conv.convert(feats, tokens)
    cls_logits, mask_logits, indices = conv.convert(feats, tokens, only_high_conf_masks=False)        # (the all-rows branch reads no class)
    assert tuple(cls_logits.shape) == (5, 2, 1000) and tuple(mask_logits.shape) == (5, 2, 3, 4) and indices.tolist() == list(range(5))


def test_from_predictor_shares_the_parameters():
    fx = sc.load("a")
    r = fx["recipe"]
    src = sc.converter(r, "cpu")
    predictor = types.SimpleNamespace(decoder_norm=src.decoder_norm, mask_embed=src.mask_embed, vis2text_projection=src.vis2text_projection,
                                      cls_temp=src.cls_temp, clip_cls_text_emb=src.clip_cls_text_emb)
    conv = stm.ConvertSemanticFeatureToMask.from_predictor(predictor, apply_cls_thres=r["cls_thres"],
                                                           apply_mask_quality_thres=r["quality_thres"], temporal_stride=r["stride"])
    assert conv.mask_embed is src.mask_embed and conv.cls_temp.weight is src.cls_temp.weight
    sc.check_against_fixture(conv, fx)
    with pytest.raises(TypeError):
        stm.ConvertSemanticFeatureToMask.from_predictor(predictor, threshold=1)


@pytest.mark.parametrize("all_rows", [False, True])
def test_cli_function_round_trip(tmp_path, all_rows):
    fx = sc.load("a")
    r = fx["recipe"]
    feats, tokens = sc.inputs(r)
    paths = {k: str(tmp_path / f"{k}.pt") for k in ("tokens", "feats", "ckpt", "clip", "out")}
    torch.save(tokens, paths["tokens"])
    torch.save(feats, paths["feats"])
    torch.save({"model": sc.checkpoint(r)}, paths["ckpt"])
    torch.save(sc.clip_table(r), paths["clip"])
    argv = ["--obj_tokens", paths["tokens"], "--mask_features", paths["feats"], "--ckpt", paths["ckpt"], "--clip_emb", paths["clip"], "--out",
            paths["out"], "--device", "cpu", "--hidden_dim", str(r["C"]), "--mask_dim", str(r["C"]), "--text_emb_dim", str(r["text_emb_dim"]),
            "--cls_thres", str(r["cls_thres"]), "--mask_quality_thres", str(r["quality_thres"]), "--temporal_stride", str(r["stride"])]
    stm.main(argv + (["--all"] if all_rows else []))
    saved = torch.load(paths["out"])
    want = sc.converter(r, "cpu").convert(feats, tokens, only_high_conf_masks=not all_rows)
    assert sorted(saved) == ["cls_logits", "indices", "mask_logits"]
    for name, w in zip(("cls_logits", "mask_logits", "indices"), want):
        assert saved[name].device.type == "cpu" and saved[name].is_contiguous() and torch.equal(saved[name], w), name


def test_aten_counts_are_the_plain_expression():
    g = torch.Generator().manual_seed(5)
    me, feats = torch.randn(7, 5, 16, generator=g), torch.randn(7, 16, 3, 4, generator=g) * 0.4
    L = torch.einsum("tnc,tchw->nthw", me, feats)[:, ::3]
    want = torch.stack([(L > 0.5).flatten(1).sum(-1), (L > -0.25).flatten(1).sum(-1)], dim=1)
    got = semantic_ops.semantic_quality_counts_aten(me, feats, 3, 0.5, -0.25)
    assert got.dtype == torch.int32 and got.tolist() == want.tolist() and 0 < int(want[:, 0].sum()) < int(want[:, 1].sum()) < L.numel()
    assert semantic_ops.semantic_quality_counts_aten(me, feats.flatten(2), 3, 0.5, -0.25).tolist() == want.tolist()
    for bad in (0, -1, 1.5):
        with pytest.raises(RuntimeError):
            semantic_ops.semantic_quality_counts_aten(me, feats, bad)
    with pytest.raises(RuntimeError):
        semantic_ops.semantic_quality_counts_aten(me, feats[:, :8], 1)
