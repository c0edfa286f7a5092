"""Writes tests/golden/g39_vocabulary_small.npz: a class-embedding table of the REFERENCE, made by its own `clean_strings`,
`pre_tokenize` and `CLIPLangEncoder.encode_text` (through oracle.ref_harness) by the rule of its
tools/clip_concept_extraction/extract_concept_emb/extract_concept_emb.py, on the synthetic weights of `cases.TEXT_SMALL`.

    python tools/gen_golden_vocabulary.py

The names are built from words that tests/golden/bpe_merges_subset.txt.gz covers ("person", "traffic light", words of g16a's
expressions); the tool checks that: this project's tokenizer on the subset table has to give the ids the reference gives on the
full one.  Recorded: the names, the cleaned names, the ids [N, 81, 77], the per-template x_eot [N, 81, D] and their mean [N, D]."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness as rh  # noqa: E402
from tests import cases  # noqa: E402
from univs_amd import synth  # noqa: E402

NAMES = ["person", "traffic light", "dog", "giraffe", "Red_jacket(2)", "cats/dogs"]
OUT = os.path.join(ROOT, "tests", "golden", "g39_vocabulary_small.npz")
SUBSET = os.path.join(ROOT, "tests", "golden", "bpe_merges_subset.txt.gz")


def main():
    L = rh.ref_language()
    U = L.clip_prompt_utils
    enc = synth.load_synthetic(L.TextEncoder.CLIPLangEncoder(out_features=["res5"], freeze_at=0, **cases.TEXT_SMALL), "lang_encoder.").eval()
    ids, feats, cleaned = [], [], []
    for name in NAMES:                                                  # extract_concept_embeddings, one name per call
        with torch.no_grad():
            concept = [U.clean_strings(name)]
            tokens = U.pre_tokenize([concept])[0]                       # 81 x 77
            x = enc.encode_text(tokens)                                 # 81 x D
        cleaned.append(concept[0])
        ids.append(tokens)
        feats.append(x)
    ids, feats = torch.stack(ids), torch.stack(feats)
    from univs_amd.modeling.language import SimpleTokenizer
    from univs_amd.vocabulary import vocabulary_tokens
    ours = vocabulary_tokens(NAMES, SimpleTokenizer(SUBSET))
    assert torch.equal(ours, ids), "a name uses a word the subset merge table does not cover"
    np.savez_compressed(OUT, names=np.array(NAMES), cleaned=np.array(cleaned), ids=ids.to(torch.int32).numpy(), x_eot=feats.numpy(),
                        mean=feats.mean(1).numpy())
    kept = (ids.argmax(-1) + 1).float()
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB): {len(NAMES)} names {cleaned}, kept tokens per text "
          f"{kept.mean():.1f} ({int(kept.min())} to {int(kept.max())})")


if __name__ == "__main__":
    main()
