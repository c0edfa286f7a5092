"""CPU: `vocabulary.install` on the synthetic model: a vocabulary whose table is the ytvis21 slice of the synthetic class table,
installed under a name of its own, behaves as ytvis21 does -- and nothing else changes."""
import types

import pytest
import torch

from oracle.cpu_path import cpu_ops
from tests import cases
from univs_amd import synth, vocabulary, workloads
from univs_amd.inference.image_generic_seg import InferenceImageGenericSegmentation
from univs_amd.inference.video_entity import COMBINED_DATASETS_CATEGORY_INFO, ImageList, InferenceVideoEntity
from univs_amd.prepare_targets import PrepareTargets

NAME = "custom"
N, START = COMBINED_DATASETS_CATEGORY_INFO["ytvis21"]                   # (40, 2203)
THINGS = list(range(0, N, 2))


def make_vocab():
    return vocabulary.Vocabulary([f"name {i}" for i in range(N)], workloads.clip_table()[START:START + N].clone(), THINGS)


def image_cfg():
    from tests.test_image_seg_cpu import image_cfg as base
    return base(SEMANTIC_ON=True, INSTANCE_ON=True, PANOPTIC_ON=True)


def make_model(device):
    """Backbone and head of the clip-loop case with the drivers and the target preparation around them, as the meta-architecture holds them."""
    case = cases.LOOP_CASE
    return types.SimpleNamespace(backbone=workloads.build_swin(device), sem_seg_head=workloads.build_head(case, device),
                                 prepare_targets=PrepareTargets(num_frames=case["T"], clip_class_embed_path=workloads.clip_table()),
                                 inference_video_entity=InferenceVideoEntity(**cases.loop_kwargs(case, stability_score_thresh=0.0)).to(device),
                                 inference_img_generic_seg=InferenceImageGenericSegmentation(image_cfg(), thing_contiguous_ids=range(80)))


def detection_targets(pt, name):
    tv = [{"task": "detection", "dataset_name": name, "video_len": 3, "file_names": ["a", "b", "c"]}]
    return pt.process_inference(tv, (64, 96), "cpu")[0]


def vis_run(model, name, device):
    case = cases.LOOP_CASE
    x = cases.preprocess(cases.loop_frames(case)).to(device)
    targets = cases.loop_targets(case)
    targets[0]["dataset_name"] = name
    with torch.no_grad():
        torch.manual_seed(1)
        return model.inference_video_entity.inference_video(model, cases.loop_batched_inputs(case), ImageList(x, [case["image_size"]] * case["n_frames"]),
                                                            targets, merge_results=False)


def check_install(device):
    """Shared with tests/test_vocabulary_install_gpu.py."""
    vocab = make_vocab()
    model, other = make_model(device), make_model(device)
    predictor, pt, entity, image = model.sem_seg_head.predictor, model.prepare_targets, model.inference_video_entity, model.inference_img_generic_seg
    before = predictor.clip_cls_text_emb.clone()
    named = dict(entity.dataset_category_info)
    base_run = vis_run(other, "ytvis21", device)
    predictor._clip_normalized(torch.zeros(1, device=device))           # (a cache to clear)
    assert vocabulary.install(model, vocab, NAME) == (N, 3938)

    # the tables: the named rows keep their bits, the installed slice is exactly the vocabulary
    assert predictor._clip_norm_cache is None and torch.equal(predictor.clip_cls_text_emb[:3938], before)
    n, start = entity.dataset_category_info[NAME]
    assert (n, start) == (N, 3938) == image.dataset_category_info[NAME] == entity._class_slice("vis", NAME)
    assert torch.equal(predictor.clip_cls_text_emb[start:start + n].cpu(), vocab.table)
    assert {k: v for k, v in entity.dataset_category_info.items() if k != NAME} == named == COMBINED_DATASETS_CATEGORY_INFO
    assert NAME not in COMBINED_DATASETS_CATEGORY_INFO and NAME not in other.inference_video_entity.dataset_category_info
    assert torch.equal(detection_targets(pt, NAME)["clip_cls_text_emb"], vocab.table)
    assert torch.equal(detection_targets(pt, "ytvis21")["clip_cls_text_emb"], before[START:START + N].cpu())
    assert image.things(NAME) == THINGS and image.things("coco_panoptic") == list(range(80))
    for again in (NAME, "ytvis21", "coco"):
        with pytest.raises(ValueError, match="named vocabulary"):
            vocabulary.install(model, vocab, again)
    with pytest.raises(ValueError, match="things"):
        vocabulary.install(model, vocabulary.Vocabulary(vocab.names, vocab.table), "other", sub_task="vps")

    # the model nobody installed anything on: its parent's tables and its parent's output, bit for bit
    assert other.sem_seg_head.predictor.clip_cls_text_emb.shape[0] == 3938 and not hasattr(other.sem_seg_head.predictor, "dataset_category_info")
    again = vis_run(other, "ytvis21", device)
    assert len(again) == len(base_run) and all(len(a) == len(b) for a, b in zip(again, base_run))
    for ca, cb in zip(again, base_run):
        for a, b in zip(ca, cb):
            assert a["obj_id"] == b["obj_id"] and torch.equal(a["score"], b["score"]) and torch.equal(a["masks"], b["masks"])

    # a VIS run under the installed name: the entities and labels of the ytvis21 run, scores within 1e-3
    got = vis_run(model, NAME, device)
    assert sum(len(c) for c in base_run) > 0, "the ytvis21 run keeps no entity: nothing is compared"
    assert [[r["obj_id"] for r in c] for c in got] == [[r["obj_id"] for r in c] for c in base_run]
    for cg, cb in zip(got, base_run):
        for a, b in zip(cg, cb):
            sa, sb = torch.as_tensor(a["score"]).float().cpu(), torch.as_tensor(b["score"]).float().cpu()
            assert sa.shape == sb.shape and sa.shape[-1] == N
            assert torch.equal(sa.argmax(-1), sb.argmax(-1)) and (sa - sb).abs().max().item() < 1e-3
    return model


def test_install_on_the_synthetic_model():
    with cpu_ops():
        check_install("cpu")


def check_image_driver(device):
    """The per-image driver under the installed name, through the meta-architecture's dispatch.  Shared with the GPU test."""
    from tests.test_image_seg_cpu import image_input
    from univs_amd.modeling.build import build_model
    model = build_model(image_cfg()).eval()
    synth.load_synthetic(model)
    model = model.to(device)
    vocab = make_vocab()
    vocabulary.install(model, vocab, NAME)
    model.inference_img_generic_seg.sem_seg_as = "labels"
    item = image_input(NAME)
    item[0]["image_id"] = "0"
    r = model(item)[0]
    labels = r["sem_seg_labels"]
    assert tuple(labels.shape) == (60, 75) and int(labels.max()) < N
    inst = r["instances"]
    assert len(inst.scores) > 0 and int(inst.pred_classes.max()) < len(THINGS)      # a class is its column among the things
    pan, info = r["panoptic_seg"]
    assert all(0 <= i["category_id"] < N and i["isthing"] == (i["category_id"] in THINGS) for i in info)
    item[0].pop("image_id")                                                        # a video of that name goes to the entity loop, not here
    seen = []
    model.inference_video_entity.eval = lambda m, b: seen.append(b[0]["dataset_name"]) or "video"
    assert model(item) == "video" and seen == [NAME]
    with pytest.raises(NotImplementedError, match="vocabulary"):                    # an unknown name stays loud
        model.inference_img_generic_seg.eval(model, image_input("elsewhere"))


def test_image_driver_under_the_installed_name():
    with cpu_ops():
        check_image_driver("cpu")
