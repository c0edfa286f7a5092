"""CPU: a class vocabulary from names (univs_amd/vocabulary.py) against the reference's own table for the same names
(tests/golden/g39_vocabulary_small.npz, tools/gen_golden_vocabulary.py: its clean_strings, pre_tokenize and encode_text by the rule of
its extract_concept_emb.py).  2e-5: the CPU tolerance of tests/test_language_cpu.py for this geometry."""
import json
import os

import numpy as np
import pytest
import torch

from oracle.cpu_path import cpu_ops
from tests import cases
from tests.test_language_cpu import BPE
from univs_amd import vocabulary
from univs_amd.modeling.language import SimpleTokenizer


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g39_vocabulary_small.npz"))


def names_of(golden):
    return [str(n) for n in golden["names"]]


def check_vocabulary(golden, device, tol, tmp_path):
    """Shared with tests/test_vocabulary_gpu.py: ids, table, round trip, and the two file formats."""
    tok = SimpleTokenizer(BPE)
    names = names_of(golden)
    assert torch.equal(vocabulary.vocabulary_tokens(names, tok), torch.from_numpy(golden["ids"]).long())
    enc = cases.build_text_encoder(cases.TEXT_SMALL, device)
    table = vocabulary.class_embeddings(names, enc, tok)
    assert tuple(table.shape) == (len(names), cases.TEXT_SMALL["embed_dim"]) and table.dtype == torch.float32
    assert table.device.type == torch.device(device).type
    err = (table.cpu() - torch.from_numpy(golden["mean"])).abs().max().item()
    print(f"class_embeddings on {device}: max abs err {err:.2e}")
    assert err < tol, err
    one = vocabulary.class_embeddings(names[1:2], enc, tok)                      # [1, D], not the reference's squeezed [D]
    assert tuple(one.shape) == (1, table.shape[1]) and (one - table[1:2]).abs().max().item() < tol
    chunked = vocabulary.class_embeddings(names, enc, tok, max_tokens=300)       # chunks straddle names
    assert (chunked - table).abs().max().item() < tol

    txt, js = tmp_path / "names.txt", tmp_path / "categories.json"
    txt.write_text("\n".join(names[:3]) + "\n\n" + "\n".join(names[3:]) + "\n")
    js.write_text(json.dumps({"categories": [{"id": 10 + 3 * i, "name": n, "isthing": int(i % 2 == 0)} for i, n in enumerate(names)]}))
    a, b = vocabulary.Vocabulary.from_file(str(txt), enc, tok), vocabulary.Vocabulary.from_file(str(js), enc, tok)
    assert a.names == b.names == names and torch.equal(a.table, b.table) and torch.equal(a.table, table)
    assert a.things is None and a.isthing is None and b.things == [0, 2, 4]

    for v in (a, b):
        path = str(tmp_path / "table.pth")
        v.save(path)
        bare = torch.load(path, map_location="cpu")
        assert isinstance(bare, torch.Tensor) and torch.equal(bare, table.cpu())     # the bare tensor, as the reference's file
        assert json.load(open(tmp_path / "table.json")) == {"names": names, "isthing": v.isthing}
        back = vocabulary.Vocabulary.load(path)
        assert back.names == v.names and back.things == v.things and torch.equal(back.table, table.cpu())


def test_vocabulary_matches_the_reference_table(golden, tmp_path):
    with cpu_ops():
        check_vocabulary(golden, "cpu", 2e-5, tmp_path)


def test_golden_holds_what_the_rule_says(golden):
    assert [str(c) for c in golden["cleaned"]] == ["person", "traffic light", "dog", "giraffe", "red jacket", "cats dogs"]
    assert tuple(golden["ids"].shape) == (6, 81, 77) and tuple(golden["x_eot"].shape) == (6, 81, 48)
    # the recorded mean is torch's fp32 one: within the summation bound n u max|x| of the exact mean of the recorded features
    x = golden["x_eot"].astype(np.float64)
    assert np.abs(x.mean(1) - golden["mean"]).max() < 81 * 2.0 ** -24 * np.abs(x).max()
    kept = golden["ids"].argmax(-1) + 1
    assert kept.min() >= 4 and kept.max() <= 13                           # what the ragged tower computes of the 77


def test_vocabulary_refuses_mismatched_parts():
    t = torch.zeros((2, 4))
    for names, table, things in ((["a"], t, None), (["a", "b"], t[0], None), (["a", "b"], t, [2]), (["a", "b"], t, [0, 0]), ([], t[:0], None)):
        with pytest.raises(ValueError):
            vocabulary.Vocabulary(names, table, things)
    with pytest.raises(ValueError):
        vocabulary.class_embeddings([], None)


def test_command_line_writes_table_and_sidecar(golden, tmp_path, monkeypatch):
    names = names_of(golden)
    (tmp_path / "names.txt").write_text("\n".join(names))
    out = tmp_path / "t.pth"
    args = vocabulary.parse_args(["--names", str(tmp_path / "names.txt"), "--clip-weights", "w.pkl", "--bpe", BPE, "--out", str(out)])
    assert (args.names, args.clip_weights, args.bpe, args.out, args.clip_depth) == (str(tmp_path / "names.txt"), "w.pkl", BPE, str(out), 200)
    monkeypatch.setattr(vocabulary, "build_lang_encoder", lambda w, depth: cases.build_text_encoder(cases.TEXT_SMALL, "cpu"))
    with cpu_ops():
        vocabulary.main(["--names", str(tmp_path / "names.txt"), "--clip-weights", "w.pkl", "--bpe", BPE, "--out", str(out)])
    back = vocabulary.Vocabulary.load(str(out))
    assert back.names == names and (back.table - torch.from_numpy(golden["mean"])).abs().max().item() < 2e-5
