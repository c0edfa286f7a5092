"""GPU: the ragged CLIP text tower (CLIPLangEncoder.encode_text_ragged, SWITCHES.text_ragged) against the reference's outputs
(g16b / g16c, at the GPU tolerances of tests/test_modules_gpu.py) and against the dense tower run on the CPU."""
import os

import numpy as np
import pytest
import torch

from oracle.cpu_path import cpu_ops
from tests import cases
from tests.test_language_cpu import check_text_encoder
from univs_amd import switches, text_ops

pytestmark = pytest.mark.gpu


def _g(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


@pytest.mark.parametrize("name,cfg,tol,stride", [("g16b_text_encoder_small", cases.TEXT_SMALL, 1e-4, 1),
                                                 ("g16c_text_encoder_full", cases.TEXT_FULL, 5e-4, 4)], ids=["small", "rn50x4"])
def test_expression_prompts_through_the_ragged_tower_match_reference(cuda, golden_dir, monkeypatch, name, cfg, tol, stride):
    calls = []
    real = text_ops.varlen_causal_attention
    monkeypatch.setattr(text_ops, "varlen_causal_attention", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    with switches.override(text_ragged=True):
        err = check_text_encoder(_g(golden_dir, name), cfg, cuda, tol, stride)
    print(f"ragged text encoder {name}: max abs err {err:.2e}")
    assert calls, "get_expression_prompt did not take the ragged tower"


def test_sample_matches_the_golden_features(cuda, golden_dir):
    g = _g(golden_dir, "g16b_text_encoder_small")
    enc = cases.build_text_encoder(cases.TEXT_SMALL, cuda)
    sample = torch.from_numpy(g["sample"]).long()
    N = sample.shape[0]
    x_word, x_eot = enc.encode_text_ragged(sample, only_eot=False, word_rows=range(N))       # tokens on the host
    assert tuple(x_word.shape) == tuple(g["x_word"].shape) and x_eot.is_cuda
    assert (x_eot.cpu() - torch.from_numpy(g["x_eot"])).abs().max().item() < 1e-4
    assert (x_word.cpu() - torch.from_numpy(g["x_word"])).abs().max().item() < 1e-4
    only = enc.encode_text_ragged(sample.to(cuda))                                             # tokens on the device, every text cut
    assert (only.cpu() - torch.from_numpy(g["x_eot"])).abs().max().item() < 1e-4
    w, e = enc.encode_text_ragged(sample, only_eot=False, word_rows=[3, 0])
    assert (w.cpu() - torch.from_numpy(g["x_word"])[[3, 0]]).abs().max().item() < 1e-4
    assert (e.cpu() - torch.from_numpy(g["x_eot"])).abs().max().item() < 1e-4


def test_cut_short_and_long_texts_match_the_dense_tower_on_the_cpu(cuda):
    """77 tokens without an end-of-text token (the largest id sits at position 40: that is where both towers read), 2 tokens, 65 tokens."""
    gen = torch.Generator().manual_seed(7)
    text = torch.zeros((3, 77), dtype=torch.int64)
    text[0] = torch.randint(1, 40000, (77,), generator=gen)
    text[0, 40] = 45000
    text[1, :2] = torch.tensor([49406, 49407])
    text[2, :65] = torch.randint(1, 40000, (65,), generator=gen)
    text[2, 0], text[2, 64] = 49406, 49407
    with cpu_ops():
        dense = cases.build_text_encoder(cases.TEXT_SMALL, "cpu").encode_text(text)
    enc = cases.build_text_encoder(cases.TEXT_SMALL, cuda)
    assert enc.kept_lengths(text) == [41, 2, 65]
    got = enc.encode_text_ragged(text)
    assert (got.cpu() - dense).abs().max().item() < 1e-4
    w, e = enc.encode_text_ragged(text, only_eot=False, word_rows=[0])
    with cpu_ops():
        dw, _ = cases.build_text_encoder(cases.TEXT_SMALL, "cpu").encode_text(text[:1], only_eot=False)
    assert (w.cpu() - dw).abs().max().item() < 1e-4 and (e.cpu() - dense).abs().max().item() < 1e-4


def test_chunks_without_word_rows(cuda, golden_dir):
    from tests.test_text_ragged_cpu import check_small_chunks
    check_small_chunks(golden_dir, cuda, 1e-4)


def test_no_dense_score_tensor_is_allocated(cuda):
    """2000 templated texts: the allocator's peak above what was live stays below the [N, h, 77, 77] floats of the dense attention."""
    cfg = cases.TEXT_SMALL
    enc = cases.build_text_encoder(cfg, cuda)
    gen = torch.Generator().manual_seed(11)
    N = 2000
    lengths = torch.randint(4, 14, (N,), generator=gen)
    text = torch.zeros((N, 77), dtype=torch.int64)
    for i, n in enumerate(lengths.tolist()):
        text[i, :n] = torch.randint(1, 40000, (n,), generator=gen)
        text[i, 0], text[i, n - 1] = 49406, 49407
    enc.encode_text_ragged(text[:8])                                   # (lazy initialisation outside the measurement)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = enc.encode_text_ragged(text)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    dense_scores = N * cfg["transformer_heads"] * 77 * 77 * 4
    print(f"ragged peak {peak / 2 ** 20:.1f} MiB, dense score tensor {dense_scores / 2 ** 20:.1f} MiB")
    assert tuple(out.shape) == (N, cfg["embed_dim"]) and peak < dense_scores
