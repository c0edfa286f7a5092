"""CPU: the third header of the C ABI (include/univs_fused_hip.h) and its wrappers (univs_amd/fused_ops.py): the symbols are exported
and bound, the binding read from the header is the recorded one (tests/fused_capi_signatures.txt), the entries validate before any launch,
the wrappers keep the contract of every wrapper (CPU tensors raise, None on ERR_NOT_IMPLEMENTED), and what hipcc made of the new
instantiations uses no more scratch than the kernels they extend."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_capi_contract_cpu import signature_lines
from tests.test_isa_cpu import listing
from univs_amd import _lib, build, fused_ops, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["univs_conv1x1_fused_presplit_f32", "univs_cross_attention_partials_f32", "univs_small_linear_merged_presplit_f32"]


def _declared():
    text = open(os.path.join(ROOT, "include", "univs_fused_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert _declared() == NAMES == sorted(_lib.FUSED_SIGNATURES)
    lib = _lib.load()
    for n in NAMES:
        assert hasattr(raw, n), f"{n} declared in include/univs_fused_hip.h but not exported"
        res, args = _lib.FUSED_SIGNATURES[n]
        assert getattr(lib, n).restype is res and list(getattr(lib, n).argtypes) == args


def test_signatures_are_the_recorded_ones_and_the_other_headers_keep_theirs():
    recorded = open(os.path.join(ROOT, "tests", "fused_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.FUSED_SIGNATURES) == recorded and [l.split()[0] for l in recorded] == NAMES
    assert len(_lib.SIGNATURES) == 76 and list(_lib.EVAL_SIGNATURES) == ["univs_vis_overlap_counts"]
    assert not set(_lib.FUSED_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EVAL_SIGNATURES))


@pytest.fixture
def host():
    """A host buffer's address: never read, the entries answer before any launch."""
    buf = (ctypes.c_int * 64)()
    yield ctypes.addressof(buf)
    del buf


def _conv(lib, p, T, Cin, Cout, H, W, layout=0, affine=None, x=None):
    return lib.univs_conv1x1_fused_presplit_f32(p if x is None else x, layout, affine, p, p, p, T, Cin, Cout, H, W, p, None)


@pytest.mark.parametrize("dims", [(-1, 96, 256, 41, 51), (2, 0, 256, 41, 51), (2, 96, -16, 41, 51), (2, 96, 256, -1, 51), (2, 96, 256, 41, -1)])
def test_conv_bad_dimensions_are_invalid_arguments(host, dims):
    lib = _lib.load()
    assert _conv(lib, host, *dims) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode().startswith("univs_conv1x1_fused_presplit_f32: bad dimensions")


def test_conv_null_pointer_and_empty_shape(host):
    lib = _lib.load()
    assert lib.univs_conv1x1_fused_presplit_f32(None, 0, None, host, host, None, 2, 96, 256, 41, 51, host, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == "univs_conv1x1_fused_presplit_f32: NULL data pointer"
    assert _conv(lib, host, 0, 96, 256, 41, 51) == _lib.OK


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("dims,affine", [((2, 96, 256, 8, 8), False),        # 128 pixels < 4096
                                         ((2, 80, 256, 41, 51), False),      # Cin neither % 96 nor % 128
                                         ((2, 96, 40, 41, 51), False),       # Cout % 16
                                         ((32, 256, 256, 12, 12), True),     # H W < 256 with the affine
                                         ((2, 1152, 256, 41, 51), True)])    # Cin > 1024 with the affine
def test_conv_uncovered_shapes_answer_not_implemented_before_any_launch(host, layout, dims, affine):
    lib = _lib.load()
    assert _conv(lib, host, *dims, layout=layout, affine=host if affine else None) == _lib.ERR_NOT_IMPLEMENTED
    assert "not covered (Cin % 96 or % 128" in lib.univs_last_error().decode()


def test_conv_unaligned_operand_is_not_covered(host):
    lib = _lib.load()
    assert _conv(lib, host, 2, 96, 256, 41, 51, x=host + 4) == _lib.ERR_NOT_IMPLEMENTED


def _partials(lib, p, L, S, N, H, hd=32, plan=None, q=None):
    out = ctypes.c_int(-7)
    rc = lib.univs_cross_attention_partials_f32(p if q is None else q, p, p, None, None, 0, L, S, N, H, hd, 0, 0, 0, 0.17, p,
                                                ctypes.byref(out) if plan is None else plan, None)
    return rc, out.value


def test_partials_validate_before_any_launch(host):
    lib = _lib.load()
    for dims in [(-1, 64, 1, 8), (4, 0, 1, 8), (4, 64, -1, 8), (4, 64, 1, 0)]:
        assert _partials(lib, host, *dims) == (_lib.ERR_INVALID_ARGUMENT, 0)
    assert lib.univs_cross_attention_partials_f32(host, host, host, None, None, 0, 4, 64, 1, 8, 32, 0, 0, 0, 0.17, host, None, None) \
        == _lib.ERR_INVALID_ARGUMENT                                                                     # no plan pointer
    assert _partials(lib, host, 0, 64, 1, 8) == (_lib.OK, 0)                                             # nothing to do: plan 0
    assert _partials(lib, host, 4, 64, 1, 8, q=0)[0] == _lib.ERR_INVALID_ARGUMENT                        # NULL q
    assert _partials(lib, host, 4, 64, 1, 8, hd=64) == (_lib.ERR_NOT_IMPLEMENTED, 0)                     # head_dim != 32
    assert _partials(lib, host, 4, 16, 1, 8) == (_lib.ERR_NOT_IMPLEMENTED, 0)                            # S < 32
    assert _partials(lib, host, 4, 64, 1, 8, q=host + 4) == (_lib.ERR_NOT_IMPLEMENTED, 0)                # unaligned q
    assert "univs_cross_attention_partials_f32" in lib.univs_last_error().decode()


def _merged(lib, p, ws_floats, plan, L, N, H, n_out=256, n_w=256, f_off=0, ln=False, ws=None, y=None):
    return lib.univs_small_linear_merged_presplit_f32(p if ws is None else ws, ws_floats, plan, L, N, H, p, p, p, n_w, f_off, None,
                                                      p if ln else None, None, 1e-5, n_out, p if y is None else y, None)


def test_merged_linear_validates_before_any_launch(host):
    lib = _lib.load()
    plan = 8 + 65536 * 7                                           # 8 segments x 7 query blocks: Lp = 112
    need = 1 * 5 * 8 * 8 * 112 * 34                                # L = 100: one chunk
    assert _merged(lib, host, need, plan, -1, 5, 8) == _lib.ERR_INVALID_ARGUMENT
    assert _merged(lib, host, need, plan, 100, 5, 0) == _lib.ERR_INVALID_ARGUMENT
    assert _merged(lib, host, need, plan, 100, 5, 8, n_out=256, n_w=128) == _lib.ERR_INVALID_ARGUMENT
    assert _merged(lib, host, need, plan, 0, 5, 8) == _lib.OK
    for bad_plan in (0, 8, 8 + 65536 * 8, -1):                     # no query blocks, more than seven, nonsense
        assert _merged(lib, host, need, bad_plan, 100, 5, 8) == _lib.ERR_INVALID_ARGUMENT
        assert "is not segments + 65536 * query blocks per wave" in lib.univs_last_error().decode()
    assert _merged(lib, host, need - 1, plan, 100, 5, 8) == _lib.ERR_INVALID_ARGUMENT                    # a workspace too small for the plan
    assert f"takes {need}" in lib.univs_last_error().decode()
    assert _merged(lib, host, need, plan, 100, 5, 8, ws=0) == _lib.ERR_INVALID_ARGUMENT                  # NULL workspace
    assert lib.univs_last_error().decode() == "univs_small_linear_merged_presplit_f32: NULL data pointer"
    assert _merged(lib, host, need * 2, plan, 100, 5, 16) == _lib.ERR_NOT_IMPLEMENTED                    # K = 512 > 256
    assert _merged(lib, host, need, plan, 100, 5, 8, n_out=40, n_w=40) == _lib.ERR_NOT_IMPLEMENTED       # n_out % 16
    assert _merged(lib, host, need, plan, 100, 5, 8, n_out=128, n_w=128, ln=True) == _lib.ERR_NOT_IMPLEMENTED   # LayerNorm needs 256
    assert _merged(lib, host, need, plan, 100, 5, 8, y=host + 4) == _lib.ERR_NOT_IMPLEMENTED             # unaligned y
    assert "not covered (H <= 8" in lib.univs_last_error().decode()


# ---- the wrappers, with the library stubbed

class _Stub:
    """Every `univs_*` function of the library: records (name, args), returns `code` (the workspace query: a size)."""

    def __init__(self, code, plan=0):
        self.code, self.plan, self.calls = code, plan, []

    def __getattr__(self, fn):
        if not fn.startswith("univs_"):
            raise AttributeError(fn)

        def call(*args):
            self.calls.append((fn, args))
            if fn == "univs_cross_attention_workspace":
                return 4096
            if fn == "univs_cross_attention_partials_f32" and self.code == _lib.OK:
                args[-2]._obj.value = self.plan                  # (ctypes.byref(plan))
            return self.code
        return call

    def univs_last_error(self):
        return b"stub"


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    monkeypatch.setattr(ops, "_stream_ptr", lambda t: "stream")
    monkeypatch.setattr(ops, "presplit_weights", lambda w, **k: (torch.zeros(4), torch.zeros(4)))
    lib = _Stub(_lib.OK, plan=2 + 65536 * 1)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    return lib


def test_wrappers_refuse_cpu_tensors():
    x, w = torch.zeros(2, 96, 48, 48), torch.zeros(256, 96, 1, 1)
    with pytest.raises(RuntimeError, match="conv1x1_fused: Not implemented on the CPU"):
        fused_ops.conv1x1_fused(x, w)
    q, k = torch.zeros(4, 1, 256), torch.zeros(64, 1, 256)
    with pytest.raises(RuntimeError, match="attention_out_proj: Not implemented on the CPU"):
        fused_ops.attention_out_proj(q, k, k, None, 8, 0.17, torch.zeros(256, 256))


def test_conv_wrapper_contract(stub):
    x, w, b = torch.zeros(2, 96, 48, 48), torch.zeros(256, 96, 1, 1), torch.zeros(256)
    y = fused_ops.conv1x1_fused(x, w, b)
    assert tuple(y.shape) == (2, 256, 48, 48) and y.is_contiguous()
    ((fn, args),) = stub.calls
    assert fn == "univs_conv1x1_fused_presplit_f32" and args[-1] == "stream" and args[-2] == y.data_ptr()
    assert args[0] == x.data_ptr() and args[1] == 0 and args[2] is None and list(args[6:11]) == [2, 96, 256, 48, 48]
    stub.calls.clear()
    x_cl = torch.zeros(2, 48, 48, 96).permute(0, 3, 1, 2)
    aff = torch.zeros(2 * 96, 2)
    assert fused_ops.conv1x1_fused(x_cl, w, b, aff) is not None
    ((fn, args),) = stub.calls
    assert args[0] == x_cl.data_ptr() and args[1] == 1 and args[2] == aff.data_ptr()                     # read in place: the view's own storage
    stub.calls.clear()
    assert fused_ops.conv1x1_fused(torch.zeros(2, 96, 48, 96)[..., ::2], w, b) is None and stub.calls == []   # neither layout: no launch, no copy
    with pytest.raises(RuntimeError, match="affine must be contiguous float32"):
        fused_ops.conv1x1_fused(x, w, b, torch.zeros(96, 2))
    stub.code = _lib.ERR_NOT_IMPLEMENTED
    assert fused_ops.conv1x1_fused(x, w, b) is None
    stub.code = _lib.ERR_LAUNCH
    with pytest.raises(_lib.UnivsHipError, match=r"conv1x1_fused failed \(code -3\): stub"):
        fused_ops.conv1x1_fused(x, w, b)


def test_attention_wrapper_contract(stub):
    q, k, w, b = torch.zeros(100, 5, 256), torch.zeros(920, 5, 256), torch.zeros(256, 256), torch.zeros(256)
    res, ln = torch.zeros(100, 5, 256), (torch.ones(256), torch.zeros(256), 1e-5)
    y = fused_ops.attention_out_proj(q, k, k, None, 8, 0.17, w, b, residual=res, ln=ln)
    assert tuple(y.shape) == (100, 5, 256)
    assert [c[0] for c in stub.calls] == ["univs_cross_attention_workspace", "univs_cross_attention_partials_f32",
                                         "univs_small_linear_merged_presplit_f32"]
    merged = stub.calls[2][1]
    assert merged[1] == 4096 and merged[2] == 2 + 65536 and list(merged[3:6]) == [100, 5, 8] and merged[-1] == "stream" and merged[-2] == y.data_ptr()
    assert merged[0] == stub.calls[1][1][-3]                                                             # the partials' workspace
    stub.calls.clear()
    assert fused_ops.attention_out_proj(q, k, k, None, 8, 0.17, torch.zeros(256, 512)) is None           # not the out-projection's K
    assert fused_ops.attention_out_proj(torch.zeros(5000, 1, 256), k[:, :1], k[:, :1], None, 8, 0.17, w) is None   # more than 4096 rows
    assert stub.calls == []
    stub.code = _lib.ERR_NOT_IMPLEMENTED
    assert fused_ops.attention_out_proj(q, k, k, None, 8, 0.17, w, b) is None
    assert [c[0] for c in stub.calls] == ["univs_cross_attention_workspace", "univs_cross_attention_partials_f32"]


# ---- what hipcc made of the new instantiations

@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    return listing(tmp_path_factory, "gemm_f16x3_stream.hip")[1]


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    return listing(tmp_path_factory, "small_linear.hip")[1]


def _stream_inst(usage, rb, ring, xmode, aff):
    return usage[next(n for n in usage if f"gemm_f16x3_streamILi{rb}ELi{ring}ELi{xmode}ELb{aff}E" in n)]


def test_affine_instantiations_use_no_scratch_beyond_the_plain_mask_feature_kernel(stream):
    """No new instantiation uses scratch, with the one exception the plain kernel already is: eight feature blocks at ring 4 (the
    mask-feature convolution, 256 -> 256) sit at the 256-register limit and spill 24 registers WITHOUT the affine, in the parent too;
    with it, not one more.  The plans in between (five to seven blocks, eight at ring 3) are not built: csrc/gemm_plan.h."""
    built = sorted(tuple(int(v) for v in m.groups()) for n in stream for m in [re.search(r"gemm_f16x3_streamILi(\d)ELi(\d)ELi(\d)ELb1E", n)] if m)
    assert built == sorted((rb, ring, xmode) for xmode in (1, 2) for ring in (3, 4) for rb in (1, 2, 3, 4, 8) if rb <= 4 or ring == 4)
    for rb, ring, xmode in built:
        aff = _stream_inst(stream, rb, ring, xmode, 1)
        if rb <= 4:
            assert aff["VGPRs Spill"] == 0 and aff["ScratchSize [bytes/lane]"] == 0, (rb, ring, xmode, aff)
        else:
            plain = _stream_inst(stream, rb, ring, xmode, 0)
            assert plain["VGPRs Spill"] == 24 and plain["ScratchSize [bytes/lane]"] == 100, plain      # the parent's figures
            assert aff["VGPRs Spill"] <= plain["VGPRs Spill"] and aff["ScratchSize [bytes/lane]"] <= plain["ScratchSize [bytes/lane]"], (xmode, aff)


def test_merging_linear_uses_no_scratch(small):
    for name, u in small.items():
        assert u["VGPRs Spill"] == 0 and u["ScratchSize [bytes/lane]"] == 0, (name, u)
    assert sum("small_linear_kernelILb1E" in n for n in small) == 1 and sum("small_linear_kernelILb0E" in n for n in small) == 1
