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
