"""A class vocabulary from a list of names: the table the category-guided results classify against, made by this project's own CLIP text
tower instead of read from the reference's 3938-row file.

Counterpart of the reference's `tools/clip_concept_extraction/extract_concept_emb/extract_concept_emb.py` (extract_concept_embeddings,
:53-78): per name `clean_strings`, the 81 prompt templates of `pre_tokenize`, `encode_text` at the end-of-text token, the mean over the
templates.  There one name is one call of the tower on 81 x 77 tokens; here all names go through the ragged tower as one batch
(CLIPLangEncoder.encode_text_ragged: a templated class name holds about 9 tokens of the 77).

  class_embeddings(names, lang_encoder, tokenizer=None)   -> float32 [N, embed_dim]
  Vocabulary(names, table, things=None)                    names + table (+ which names are things); save / load, from_file
  install(model, vocab, name="custom", sub_task="vis")     makes `name` a vocabulary of that model's decoder, targets and drivers
  python -m univs_amd.vocabulary --names FILE --clip-weights W [--bpe V] --out table.pth

Files: `table.pth` holds the bare tensor, exactly as the reference's file does (it loads wherever `CLIP_CLASS_EMBED_PATH` is read); the
sidecar `table.json` holds {"names", "isthing"}.

Deliberate deviation: the table is always [N, D]; the reference's `squeeze` makes a one-name table one-dimensional.
"""
import argparse
import json
import os

import torch

from .modeling.language import clean_strings, pre_tokenize

MAX_TOKENS = 4096 * 77          # kept tokens per call of the ragged tower: the activation memory of get_expression_prompt's max_batch


def vocabulary_tokens(names, tokenizer=None):
    """[N, 81, 77] int64: the templated texts of the cleaned names, template-major as the reference's `pre_tokenize([name])[0]`."""
    cleaned = [clean_strings(str(n)) for n in names]
    return pre_tokenize(cleaned, tokenizer)


@torch.no_grad()
def class_embeddings(names, lang_encoder, tokenizer=None, max_tokens=MAX_TOKENS):
    """float32 [N, embed_dim] on the encoder's device: row i is the mean over the 81 templates of the end-of-text feature of name i.
    On the GPU all names run through the ragged tower, in chunks of whole texts of at most `max_tokens` kept tokens; on the CPU through
    the dense `encode_text`, one name (81 texts) per call as the reference does."""
    names = list(names)
    if not names:
        raise ValueError("class_embeddings: no names")
    return embeddings_of_tokens(vocabulary_tokens(names, tokenizer), lang_encoder, max_tokens)


@torch.no_grad()
def embeddings_of_tokens(tokens, lang_encoder, max_tokens=MAX_TOKENS):
    """`class_embeddings` from the [N, 81, 77] ids of `vocabulary_tokens` (on the host: their lengths cost no synchronisation)."""
    N, P, L = tokens.shape
    if lang_encoder.device.type != "cuda":
        return torch.stack([lang_encoder.encode_text(tokens[i].to(lang_encoder.device)).mean(0) for i in range(N)])
    flat = tokens.reshape(N * P, L)
    lengths = lang_encoder.kept_lengths(flat)
    eots, lo = [], 0
    while lo < N * P:
        hi, budget = lo + 1, max_tokens - lengths[lo]
        while hi < N * P and lengths[hi] <= budget:
            budget -= lengths[hi]
            hi += 1
        eots.append(lang_encoder.encode_text_ragged(flat[lo:hi], lengths=lengths[lo:hi]))
        lo = hi
    return torch.cat(eots).view(N, P, -1).mean(1)


def read_names(path):
    """(names, isthing or None) of a text file (one name per line, empty lines skipped) or of a json that holds a `categories` list
    (data.load_categories_json: names in the file's order, `isthing` as the file says; None unless every category states it)."""
    if str(path).endswith(".json"):
        from .data.image_datasets import load_categories_json
        table = load_categories_json(path)
        with open(path) as f:                                           # (the class table takes a missing `isthing` for 1: here it is "not stated")
            stated = all("isthing" in c for c in json.load(f)["categories"])
        return list(table["names"]), ([bool(t) for t in table["isthing"]] if stated else None)
    with open(path) as f:
        names = [line.strip() for line in f]
    return [n for n in names if n], None


class Vocabulary:
    """`names` (as given, not cleaned), their `table` [N, D], and `things`: the contiguous indices that are things (None: not stated;
    every name is then taken for a thing where a driver needs to know)."""

    def __init__(self, names, table, things=None):
        names = [str(n) for n in names]
        if table.dim() != 2 or table.shape[0] != len(names) or not names:
            raise ValueError(f"Vocabulary: {len(names)} names and a table of shape {tuple(table.shape)}")
        if things is not None:
            things = sorted(int(c) for c in things)
            if any(not 0 <= c < len(names) for c in things) or len(set(things)) != len(things):
                raise ValueError("Vocabulary: things are distinct indices into names")
        self.names, self.table, self.things = names, table, things

    def __len__(self):
        return len(self.names)

    @property
    def isthing(self):
        return None if self.things is None else [i in set(self.things) for i in range(len(self.names))]

    @classmethod
    def from_names(cls, names, lang_encoder, tokenizer=None, isthing=None):
        things = None if isthing is None else [i for i, t in enumerate(isthing) if t]
        return cls(names, class_embeddings(names, lang_encoder, tokenizer).float(), things)

    @classmethod
    def from_file(cls, path, lang_encoder, tokenizer=None):
        """From a text file (one name per line) or a categories json."""
        names, isthing = read_names(path)
        return cls.from_names(names, lang_encoder, tokenizer, isthing)

    @staticmethod
    def sidecar(path):
        return os.path.splitext(str(path))[0] + ".json"

    def save(self, path):
        """`path` (.pth): the bare tensor on the CPU; beside it `<stem>.json` with {"names", "isthing"}."""
        torch.save(self.table.detach().cpu().contiguous(), path)
        with open(self.sidecar(path), "w") as f:
            json.dump({"names": self.names, "isthing": self.isthing}, f, indent=1)

    @classmethod
    def load(cls, path):
        table = torch.load(path, map_location="cpu")
        with open(cls.sidecar(path)) as f:
            side = json.load(f)
        isthing = side.get("isthing")
        return cls(side["names"], table, None if isthing is None else [i for i, t in enumerate(isthing) if t])


SUB_TASKS = ("vis", "vss", "vps")


def install(model, vocab, name="custom", sub_task="vis"):
    """Make `name` a vocabulary of THIS model, everywhere it looks one up.  The rows of `vocab.table` are appended to the model's class
    table and `name` becomes the slice (N, rows before) that selects exactly them; the named vocabularies keep their slices and
    their rows, and a model `install` was never called on shares nothing that is changed here (the tables and slice maps become
    per-model copies).  Touched, where the model has them:
      the decoder (`sem_seg_head.predictor`): `clip_cls_text_emb` (detection prompts, class head), `_clip_norm_cache` cleared, its slice map
      `prepare_targets`: `clip_cls_text_emb` and its slice map -- a "detection" target of `name` is handed exactly `vocab.table`
      `inference_video_entity`: `dataset_category_info`; a video of `name` runs under `sub_task` ("vis", "vss" or "vps"; "vps" needs
          `vocab.things`) with the vocabulary's things
      `inference_img_generic_seg`: `dataset_category_info`, `thing_contiguous_ids[name]` = `vocab.things` (every name where None)
    The MinVIS-style drivers and the VOS driver stay with the named vocabularies.  Returns the slice (N, start)."""
    from .modeling.transformer_decoder.univs_decoder import combined_datasets_category_info
    if sub_task not in SUB_TASKS:
        raise ValueError(f"install: sub_task {sub_task!r} (one of {SUB_TASKS})")
    if sub_task == "vps" and vocab.things is None:
        raise ValueError("install: the panoptic sub-task needs to know which names are things (a categories json with `isthing`)")
    predictor = model.sem_seg_head.predictor
    info = dict(getattr(predictor, "dataset_category_info", None) or combined_datasets_category_info)
    if name in info or name.startswith(("coco", "ade20k", "ytvis", "ovis", "vipseg", "vspw")):
        raise ValueError(f"install: {name!r} is a named vocabulary (or installed already); choose another name")
    old = predictor.clip_cls_text_emb
    if vocab.table.shape[1] != old.shape[1]:
        raise ValueError(f"install: the table has {vocab.table.shape[1]} channels, the model's {old.shape[1]}")
    N, start = len(vocab), int(old.shape[0])
    rows = vocab.table.detach().to(device=old.device, dtype=old.dtype)
    info[name] = (N, start)
    predictor.clip_cls_text_emb = torch.cat([old, rows])
    predictor._clip_norm_cache = None
    predictor.dataset_category_info = info
    pt = getattr(model, "prepare_targets", None)
    if pt is not None:
        if pt.clip_cls_text_emb.shape[0] != start:
            raise ValueError("install: prepare_targets and the decoder hold class tables of different lengths")
        pt.clip_cls_text_emb = torch.cat([pt.clip_cls_text_emb, rows.to(pt.clip_cls_text_emb)])
        pt.dataset_category_info = dict(info)
    things = list(range(N)) if vocab.things is None else list(vocab.things)
    entity = getattr(model, "inference_video_entity", None)
    if entity is not None:
        entity.dataset_category_info = {**entity.dataset_category_info, name: (N, start)}
        entity.installed_vocabularies = {**getattr(entity, "installed_vocabularies", {}),     # (category ids there are 1-based)
                                         name: {"sub_task": sub_task, "thing_dataset_ids": frozenset(c + 1 for c in things)}}
    image = getattr(model, "inference_img_generic_seg", None)
    if image is not None:
        image.dataset_category_info = {**image.dataset_category_info, name: (N, start)}
        ids = image.thing_contiguous_ids
        ids = dict(ids) if isinstance(ids, dict) else {n: list(ids) for n in image.dataset_category_info if n != name}
        ids[name] = things
        image.thing_contiguous_ids = ids
        image.installed_vocabularies = {*getattr(image, "installed_vocabularies", ()), name}
    model.installed_vocabularies = {**getattr(model, "installed_vocabularies", {}), name: vocab}
    return N, start


def build_lang_encoder(clip_weights, depth=200, device=None):
    """The CLIP text tower of `MODEL.CLIP.RESNETS_DEPTH = depth` (200: RN50x4, UniVS's) with the converted checkpoint `clip_weights`."""
    from .modeling.language.text_encoder import CLIP_TEXT_CONFIGS, CLIPLangEncoder, load_checkpoint
    embed_dim, width, heads = CLIP_TEXT_CONFIGS[depth]
    model = CLIPLangEncoder(embed_dim, 77, 49408, width, heads, 12)
    load_checkpoint(model, clip_weights)
    return model.eval().to(device or ("cuda" if torch.cuda.is_available() else "cpu"))


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m univs_amd.vocabulary", description="class names -> CLIP class-embedding table")
    p.add_argument("--names", required=True, help="text file (one name per line) or a json with a `categories` list")
    p.add_argument("--clip-weights", required=True, help="converted CLIP text-tower checkpoint (MODEL.CLIP.WEIGHTS)")
    p.add_argument("--clip-depth", type=int, default=200, choices=(50, 101, 200), help="MODEL.CLIP.RESNETS_DEPTH (200: RN50x4)")
    p.add_argument("--bpe", default=None, help="CLIP's BPE merge table (default: UNIVS_BPE_VOCAB or the packaged one)")
    p.add_argument("--out", required=True, help="table.pth; table.json is written beside it")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    tokenizer = None
    if args.bpe:
        from .modeling.language import SimpleTokenizer
        tokenizer = SimpleTokenizer(args.bpe)
    vocab = Vocabulary.from_file(args.names, build_lang_encoder(args.clip_weights, args.clip_depth), tokenizer)
    vocab.save(args.out)
    print(f"{len(vocab)} names -> {args.out} {tuple(vocab.table.shape)}, {Vocabulary.sidecar(args.out)}")


if __name__ == "__main__":
    main()
