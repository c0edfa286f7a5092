"""The CLIP text tower, dense against ragged, on the RN50x4 geometry (cases.TEXT_FULL, synthetic weights):

  vocab133 / vocab1203   a class vocabulary of 133 / 1203 names (81 templated texts each) -> table [N, 640]
  expressions4           TextPromptEncoder.get_expression_prompt for 4 referring expressions

    python tools/text_tower_bench.py [--cases vocab133,vocab1203,expressions4] [--samples 5] [--out profiles/text_tower_bench_v1.json]

Yardstick: the dense `encode_text`, chunked as `max_batch` = 4096 texts chunks it (for the expressions: get_expression_prompt with
SWITCHES.text_ragged off).  Each case is timed dense and ragged in the same run, `--samples` alternating samples after one warm-up of
each; min and max are reported, with the allocator's peak above what was live before the call, and the token counts.  The names are
drawn from the words tests/golden/bpe_merges_subset.txt.gz covers, one to three words each, so that the tool needs no other table."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import cases  # noqa: E402
from univs_amd import switches, vocabulary  # noqa: E402
from univs_amd.modeling.language import SimpleTokenizer, pre_tokenize_expression  # noqa: E402
from univs_amd.modeling.prompt_encoder import TextPromptEncoder  # noqa: E402

WORDS = ["person", "traffic", "light", "dog", "giraffe", "red", "jacket", "cats", "dogs", "zebras", "heads", "left", "running", "white",
         "skiing", "downhill", "eating", "leaves"]
EXPRESSIONS = ["a dog running", "The person in a red-and-white jacket, skiing downhill!", "two zebras' heads (left)",
               "it's the giraffe that's eating leaves"]
BPE = os.environ.get("UNIVS_BPE_VOCAB") or os.path.join(ROOT, "tests", "golden", "bpe_merges_subset.txt.gz")
MAX_BATCH = 4096


def names_of(n):
    gen = torch.Generator().manual_seed(n)
    out = []
    for _ in range(n):
        k = int(torch.randint(1, 4, (1,), generator=gen))
        out.append(" ".join(WORDS[int(i)] for i in torch.randint(0, len(WORDS), (k,), generator=gen)))
    return out


def measure(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, torch.cuda.max_memory_allocated() - before, out


def compare(dense, ragged, samples):
    """One warm-up of each, then `samples` alternating samples -> the two records and the results of the last sample."""
    dense(), ragged()
    rec = {"dense": {"ms": [], "peak": 0}, "ragged": {"ms": [], "peak": 0}}
    outs = {}
    for _ in range(samples):
        for key, fn in (("dense", dense), ("ragged", ragged)):
            ms, peak, outs[key] = measure(fn)
            rec[key]["ms"].append(ms)
            rec[key]["peak"] = max(rec[key]["peak"], peak)
    return ({k: {"ms_min": round(min(v["ms"]), 3), "ms_max": round(max(v["ms"]), 3), "peak_MiB": round(v["peak"] / 2 ** 20, 1)}
             for k, v in rec.items()}, outs)


def vocab_case(n, enc, tok, samples):
    tokens = vocabulary.vocabulary_tokens(names_of(n), tok)
    N, P, L = tokens.shape
    flat = tokens.reshape(N * P, L)
    kept = sum(enc.kept_lengths(flat))

    def dense():
        dev = flat.to(enc.device)
        return torch.cat([enc.encode_text(dev[lo:lo + MAX_BATCH]) for lo in range(0, N * P, MAX_BATCH)]).view(N, P, -1).mean(1)

    def ragged():
        return vocabulary.embeddings_of_tokens(tokens, enc)            # (both from the host ids: tokenizing is outside either)
    rec, outs = compare(dense, ragged, samples)
    rec.update(names=n, texts=N * P, dense_tokens=N * P * L, kept_tokens=kept,
               max_abs_diff=float((outs["dense"] - outs["ragged"]).abs().max()))
    return rec


def expression_case(enc, tok, samples):
    tokens = pre_tokenize_expression(EXPRESSIONS, tok)
    tpe = TextPromptEncoder(enc, num_frames=1, device=enc.device)
    E, P, L = tokens.shape
    kept = sum(enc.kept_lengths(tokens.reshape(E * P, L), range(0, E * P, P)))

    def run(flag):
        def fn():
            with switches.override(text_ragged=flag):
                return tpe.get_expression_prompt(EXPRESSIONS, enc.device, tokens=tokens)[:2]
        return fn
    rec, outs = compare(run(False), run(True), samples)
    rec.update(expressions=E, texts=E * P, dense_tokens=E * P * L, kept_tokens=kept,
               max_abs_diff=max(float((a - b).abs().max()) for a, b in zip(outs["dense"], outs["ragged"])))
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cases", default="vocab133,vocab1203,expressions4")
    p.add_argument("--samples", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_tower_bench_v1.json"))
    args = p.parse_args()
    enc = cases.build_text_encoder(cases.TEXT_FULL, "cuda")
    tok = SimpleTokenizer(BPE)
    result = {"geometry": cases.TEXT_FULL, "samples": args.samples, "device": torch.cuda.get_device_name(0), "cases": {}}
    for case in args.cases.split(","):
        with torch.no_grad():
            rec = expression_case(enc, tok, args.samples) if case == "expressions4" else vocab_case(int(case[len("vocab"):]), enc, tok, args.samples)
        result["cases"][case] = rec
        print(case, json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:                                  # (after every case: a long run leaves what it finished)
            json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
