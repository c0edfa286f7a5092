"""CPU: the ragged text tower (CLIPLangEncoder.encode_text_ragged, SWITCHES.text_ragged) on the oracle's CPU operators, with the ATen
formulation of the varlen attention: the chunking of `get_expression_prompt` by kept tokens, and the calls with no word rows."""
import os

import numpy as np
import torch

from oracle.cpu_path import cpu_ops
from tests import cases
from univs_amd import switches
from univs_amd.modeling.prompt_encoder import TextPromptEncoder


def check_small_chunks(golden_dir, device, tol):
    """`max_batch` of 1, 2 and 7 under text_ragged: chunks of at most 77, 154 and 539 kept tokens -- most hold no bare-expression row,
    some hold nothing else -- against the reference's prompts (g16b).  Shared with tests/test_text_ragged_gpu.py."""
    g = np.load(os.path.join(golden_dir, "g16b_text_encoder_small.npz"))
    enc = cases.build_text_encoder(cases.TEXT_SMALL, device)
    tokens = torch.from_numpy(g["tokens"]).long()
    E, P, L = tokens.shape
    lengths = enc.kept_lengths(tokens.reshape(E * P, L), range(0, E * P, P))
    assert max(lengths) == 77 and sum(lengths) > 7 * 77 * 4            # every max_batch below splits the texts into many chunks
    tpe = TextPromptEncoder(enc, num_frames=1, device=device)
    exprs = [("w " * (int(n) - 5)).strip() for n in g["exp_word_len"]]
    calls = []
    real = enc.encode_text_ragged

    def counted(text, **kw):
        calls.append((text.shape[0], len(kw["word_rows"])))
        return real(text, **kw)
    enc.encode_text_ragged = counted
    for max_batch in (1, 2, 7):
        calls.clear()
        with switches.override(text_ragged=True):
            w, s, _ = tpe.get_expression_prompt(exprs, device, tokens=tokens, max_batch=max_batch)
        assert sum(n for n, _ in calls) == E * P and sum(k for _, k in calls) == E
        assert any(k == 0 for _, k in calls), "no chunk without a bare-expression row: the case under test did not occur"
        assert tuple(w.shape) == (E, 77, 1, cases.TEXT_SMALL["embed_dim"])
        e_w = (w[:, :, 0].cpu() - torch.from_numpy(g["exp_word_feats"])).abs().max().item()
        e_s = (s[:, 0].cpu() - torch.from_numpy(g["exp_sentence_feats"])).abs().max().item()
        assert e_w < tol and e_s < tol, (max_batch, e_w, e_s)
    del enc.encode_text_ragged


def test_chunks_without_word_rows(golden_dir):
    with cpu_ops():
        check_small_chunks(golden_dir, "cpu", 2e-5)


def test_no_word_rows_give_an_empty_word_tensor(golden_dir):
    g = np.load(os.path.join(golden_dir, "g16b_text_encoder_small.npz"))
    sample = torch.from_numpy(g["sample"]).long()
    with cpu_ops():
        enc = cases.build_text_encoder(cases.TEXT_SMALL, "cpu")
        w, e = enc.encode_text_ragged(sample, only_eot=False, word_rows=[])
        assert tuple(w.shape) == (0, 77, 48) and (e - torch.from_numpy(g["x_eot"])).abs().max().item() < 2e-5
        assert torch.equal(e, enc.encode_text_ragged(sample))
