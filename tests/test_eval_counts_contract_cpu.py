"""The contract of the three count wrappers of univs_amd/evaluation (pair_counts.py, vss_counts.py, davis_counts.py over _counts.py) with
the library stubbed: what tests/test_ops_contract_cpu.py pins for the wrappers of ops.py.  No GPU, no library."""
import pytest
import torch

from univs_amd import _lib, ops
from univs_amd.evaluation import davis_counts as dc
from univs_amd.evaluation import pair_counts as pc
from univs_amd.evaluation import vss_counts as vc


class _Stub:
    """Every `univs_*` function of the library: records (name, args), returns `code`."""

    def __init__(self, code):
        self.code, self.calls = code, []

    def __getattr__(self, fn):
        if not fn.startswith("univs_"):
            raise AttributeError(fn)

        def call(*args):
            self.calls.append((fn, args))
            return self.code
        return call

    def univs_last_error(self):
        return b"stub"


def _u8(*shape):
    return torch.zeros(*shape, dtype=torch.uint8)


RGB, I32 = _u8(2, 4, 6, 3), torch.zeros(2, 4, 6, dtype=torch.int32)
GI, PI = torch.arange(3), torch.arange(5)
U8 = _u8(2, 4, 6)

# name -> (the wrapper, the library's function, a covered call, its integer arguments in the capi order, (shape, initial value) of each
#          output, the calls beyond a coverage bound, the call exactly at the bounds)
WRAPPERS = {
    "panoptic_pair_counts": (
        pc.panoptic_pair_counts, "univs_panoptic_pair_counts", (RGB, I32, GI, PI), [1, 0, 2, 4, 6, 3, 5],      # gt_rgb, pred_rgb, T, H, W, G, P
        [((2, 4, 6), 0), ((2, 2), -1)],
        [(RGB, I32, torch.arange(127), torch.arange(128)),                                                      # 128 x 129 cells
         (RGB, I32, torch.arange(1025), GI)],
        (RGB, I32, torch.arange(127), torch.arange(127))),                                                      # 128 x 128 = 16384 cells
    "vss_video_counts": (
        vc.vss_video_counts, "univs_vss_video_counts", (U8, U8, 19), [2, 4, 6, 19],                             # T, H, W, C
        [((19, 19), 0), ((2, 2, 2), 0), ((1,), -1)],
        [(U8, U8, 129), (_u8(1025, 1, 1), _u8(1025, 1, 1), 19)],
        (_u8(1024, 1, 1), _u8(1024, 1, 1), 128)),                                                               # 128 x 128 = 16384 cells
    "davis_video_counts": (
        dc.davis_video_counts, "univs_davis_counts", (U8, U8, 3, 5, 7, True), [2, 4, 6, 3, 5, 7, 1],            # T, H, W, G, P, radius, use_void
        [((3, 5, 2, 2), 0), ((3, 2), 0), ((5, 2), 0), ((3, 5, 2, 2), 0)],
        [(U8, U8, 33, 5, 7, True), (U8, U8, 3, 33, 7, True), (U8, U8, 3, 5, 37, True)],
        (U8, U8, 32, 32, 36, True)),
}


@pytest.mark.parametrize("name", list(WRAPPERS))
def test_wrapper_contract_with_the_library_stubbed(monkeypatch, name):
    """Through `ops._call`, stream last, the outputs freshly allocated and handed over just before it, None on ERR_NOT_IMPLEMENTED, the
    wrapper's name on a launch error, no launch beyond a coverage bound and one exactly at it."""
    wrapper, fn, call, ints, outputs, beyond, at = WRAPPERS[name]
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    monkeypatch.setattr(ops, "_stream_ptr", lambda t: "stream")
    lib = _Stub(_lib.OK)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    out = wrapper(*call)
    assert len(out) == len(outputs)
    for o, (shape, value) in zip(out, outputs):
        assert tuple(o.shape) == shape and o.dtype == torch.int32 and bool((o == value).all())
    ((called, args),) = lib.calls
    assert called == fn
    assert args[-1] == "stream" and [a for a in args if isinstance(a, int) and a < 1 << 32] == ints
    assert list(args[-1 - len(out):-1]) == [o.data_ptr() for o in out]
    lib.code = _lib.ERR_NOT_IMPLEMENTED
    assert wrapper(*call) is None
    lib.code = _lib.ERR_LAUNCH
    with pytest.raises(_lib.UnivsHipError) as e:
        wrapper(*call)
    assert str(e.value) == f"{name} failed (code -3): stub"
    lib.code, lib.calls = _lib.OK, []
    for c in beyond:
        assert wrapper(*c) is None
    assert lib.calls == []
    assert wrapper(*at) is not None and len(lib.calls) == 1
