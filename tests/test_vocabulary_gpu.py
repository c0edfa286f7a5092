"""GPU: a class vocabulary from names through the ragged text tower (univs_amd/vocabulary.py, csrc/text_attn.hip) against the reference's
table (tests/golden/g39_vocabulary_small.npz).  1e-4: the GPU tolerance of tests/test_modules_gpu.py for this geometry."""
import pytest

from tests.test_vocabulary_cpu import check_vocabulary, golden  # noqa: F401  (the fixture)
from univs_amd import text_ops

pytestmark = pytest.mark.gpu


def test_vocabulary_matches_the_reference_table(cuda, golden, tmp_path, monkeypatch):  # noqa: F811
    calls = []
    real = text_ops.varlen_causal_attention

    def counted(*a, **kw):
        out = real(*a, **kw)
        calls.append(out is not None)
        return out
    monkeypatch.setattr(text_ops, "varlen_causal_attention", counted)
    check_vocabulary(golden, cuda, 1e-4, tmp_path)
    assert calls and all(calls), "the vocabulary did not run on the varlen attention kernel"
