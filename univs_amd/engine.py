"""The loop of detectron2's `inference_on_dataset` for videos, one record at a time: map, run the model, hand both to the evaluator."""
import torch


def inference_on_videos(model, records, mapper, evaluator=None, on_output=None):
    """For every record: `inputs = [mapper(record)]`, `outputs = model(inputs)` without gradients, then `evaluator.process(inputs,
    outputs)` (the protocol of evaluation.YTVISEvaluator / VPSEvaluator / VSSEvaluator) and `on_output(inputs, outputs)` where given.
    Returns `evaluator.evaluate()`; without an evaluator the list of outputs, which a caller that gives `on_output` (to write each
    video's output away, say) does not get: nothing is kept for it."""
    if evaluator is not None:
        evaluator.reset()
    kept = [] if evaluator is None and on_output is None else None
    for record in records:
        inputs = [mapper(record)]
        with torch.no_grad():
            outputs = model(inputs)
        if evaluator is not None:
            evaluator.process(inputs, outputs)
        if on_output is not None:
            on_output(inputs, outputs)
        if kept is not None:
            kept.append(outputs)
    return evaluator.evaluate() if evaluator is not None else kept


def inference_on_images(model, records, mapper, evaluators=None, on_output=None, batch=1):
    """The same loop for images, `batch` mapped records per model call (the per-image driver's `eval` takes several): for every batch
    `inputs = [mapper(r) for r in batch]`, `outputs = model(inputs)` (one result per image), then every evaluator's `process(inputs,
    outputs)` and `on_output(inputs, outputs)`.  `evaluators`: None, one evaluator or a list of them; with several the returned
    dictionaries are merged into one, as detectron2's `DatasetEvaluators` does (a key two of them return is an error).  Without an
    evaluator the list of per-image outputs, unless `on_output` takes them."""
    if evaluators is None:
        evaluators = []
    elif not isinstance(evaluators, (list, tuple)):
        evaluators = [evaluators]
    for ev in evaluators:
        ev.reset()
    kept = [] if not evaluators and on_output is None else None
    records = list(records)
    batch = max(1, int(batch))
    for first in range(0, len(records), batch):
        inputs = [mapper(r) for r in records[first:first + batch]]
        with torch.no_grad():
            outputs = model(inputs)
        for ev in evaluators:
            ev.process(inputs, outputs)
        if on_output is not None:
            on_output(inputs, outputs)
        if kept is not None:
            kept += list(outputs)
    if not evaluators:
        return kept
    merged = {}
    for ev in evaluators:
        for k, v in (ev.evaluate() or {}).items():
            assert k not in merged, f"Different evaluators produce results with the same key {k}"
            merged[k] = v
    return merged
