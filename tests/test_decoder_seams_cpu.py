"""CPU: the sixteenth header of the C ABI (include/univs_seam_hip.h) and its wrappers (univs_amd/seam_ops.py, `ops.small_seam`, the
`pre_ln` / `side` keywords of `ops.small_mlp`): the two symbols are exported and bound, the binding read from the header is the recorded
one (tests/seam_capi_signatures.txt), the entries answer invalid and uncovered arguments before any launch, the wrappers answer None
where they do not apply and hand the library what their docstrings say, and a head on the CPU is the same with SWITCHES.decoder_seams
on and off (no seam applies there).  What the kernels compute: tests/test_decoder_seams_gpu.py."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_capi_contract_cpu import signature_lines
from tests.test_isa_cpu import listing
from univs_amd import _lib, build, ops, seam_ops
from univs_amd.switches import SWITCHES, override

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MLP, SEAM = "univs_small_mlp_seam_presplit_f32", "univs_small_seam_presplit_f32"


def _declared():
    text = open(os.path.join(ROOT, "include", "univs_seam_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert _declared() == [MLP, SEAM] == sorted(_lib.SEAM_SIGNATURES)
    lib = _lib.load()
    for n in (MLP, SEAM):
        assert hasattr(raw, n), f"{n} declared in include/univs_seam_hip.h but not exported"
        res, args = _lib.SEAM_SIGNATURES[n]
        assert getattr(lib, n).restype is res and list(getattr(lib, n).argtypes) == args


def test_signatures_are_the_recorded_ones_and_the_other_tables_keep_theirs():
    recorded = open(os.path.join(ROOT, "tests", "seam_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.SEAM_SIGNATURES) == recorded == [MLP + " I PPPPFPPPPPIIPIPPPPPPFPLIPP", SEAM + " I PPPPPPPFPPPPPIILIIIIIPP"]
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES") and n != "SEAM_SIGNATURES"]
    assert len(others) == 15 and not any(set(_lib.SEAM_SIGNATURES) & set(t) for t in others)
    assert len(_lib.SIGNATURES) == 76 and len(_lib.FUSED_SIGNATURES) == 3
    assert "small_linear.hip" in build.SOURCES and any(h.endswith("univs_seam_hip.h") for h in build.HEADERS)
    assert SWITCHES.decoder_seams is True or os.environ.get("UNIVS_DECODER_SEAMS") is not None


@pytest.fixture
def host():
    """A host buffer's address: never read, the entries answer before any launch."""
    buf = (ctypes.c_int * 64)()
    yield ctypes.addressof(buf)
    del buf


def _seam(lib, p, M=16, Ka=256, Na=256, Nb=768, n_wb=768, f_off=0, add_features=0, null=(), **ptr):
    a = {k: (None if k in null else ptr.get(k, p)) for k in ("x", "wpa", "winv_a", "residual", "ln", "t", "wpb", "winv_b", "y")}
    return getattr(lib, SEAM)(a["x"], a["wpa"], a["winv_a"], None, a["residual"], a["ln"], None, 1e-5, a["t"], None, a["wpb"], a["winv_b"],
                              None, n_wb, f_off, M, Ka, Na, Nb, 0, add_features, a["y"], None)


def test_seam_entry_validates_before_any_launch(host):
    lib = _lib.load()
    for bad in (dict(M=-1), dict(Nb=-256), dict(n_wb=0), dict(f_off=-4), dict(f_off=256), dict(Ka=0), dict(Na=0)):
        assert _seam(lib, host, **bad) == _lib.ERR_INVALID_ARGUMENT, bad
        assert lib.univs_last_error().decode().startswith(SEAM + ": bad arguments M=")
    assert _seam(lib, None, M=0) == _lib.OK and _seam(lib, None, Nb=0) == _lib.OK           # nothing to do: nothing is read
    for null in ("x", "wpa", "winv_a", "residual", "ln", "t", "wpb", "winv_b", "y"):
        assert _seam(lib, host, null=(null,)) == _lib.ERR_INVALID_ARGUMENT, null
        assert lib.univs_last_error().decode() == SEAM + ": NULL data pointer"
    for uncovered in (dict(Ka=128), dict(Na=512), dict(Nb=384), dict(Nb=128, n_wb=128), dict(f_off=2, n_wb=1024), dict(add_features=48),
                      dict(M=16 * 65535 + 1), dict(x=host + 4), dict(y=host + 8), dict(t=host + 4)):
        assert _seam(lib, host, **uncovered) == _lib.ERR_NOT_IMPLEMENTED, uncovered
        assert "not covered (Ka == Na == 256, Nb % 256 == 0" in lib.univs_last_error().decode()


def _mlp(lib, p, M=16, stages=3, out_T=0, pre=None, side=None, side_n_w=768, side_f_off=0, x=None, null_tables=False):
    P3, I3 = ctypes.c_void_p * 3, ctypes.c_int * 3
    tab = None if null_tables else P3(p, p, p)
    pre = pre if pre is not None else (None, None, None, None)
    side = side if side is not None else (None, None, None, None, None)
    return getattr(lib, MLP)(p if x is None else x, pre[0], pre[1], pre[2], 1e-5, pre[3], side[0], side[1], side[2], side[3], side_n_w,
                             side_f_off, side[4], stages, tab, tab, tab, None if null_tables else I3(1, 1, 0), None, None, 1e-5, None, M,
                             out_T, p, None)


def test_mlp_entry_validates_before_any_launch(host):
    lib = _lib.load()
    p = host
    for bad in (dict(M=-1), dict(stages=0), dict(stages=4), dict(out_T=-1), dict(side=(None, p, p, None, p), side_n_w=0),
                dict(side=(None, p, p, None, p), side_f_off=-4), dict(side=(None, p, p, None, p), side_f_off=640)):
        assert _mlp(lib, p, **bad) == _lib.ERR_INVALID_ARGUMENT, bad
        assert lib.univs_last_error().decode().startswith(MLP + ": bad arguments M=")
    assert _mlp(lib, None, M=0, null_tables=True) == _lib.OK
    assert _mlp(lib, p, null_tables=True) == _lib.ERR_INVALID_ARGUMENT and lib.univs_last_error().decode() == MLP + ": NULL pointer"
    for uncovered in (dict(out_T=5), dict(M=16 * 65535 + 1), dict(x=p + 4),
                      dict(pre=(p, p, None, p)), dict(pre=(p, None, p, p)), dict(pre=(p, p, p, None)), dict(pre=(None, p, p, None)),
                      dict(pre=(p + 4, p, p, p)), dict(side=(None, p, None, None, p)), dict(side=(None, p, p, None, None)),
                      dict(side=(p, None, None, None, None)), dict(side=(None, p, p, None, p), side_f_off=2),
                      dict(side=(None, p, p, None, p + 4))):
        assert _mlp(lib, p, **uncovered) == _lib.ERR_NOT_IMPLEMENTED, uncovered
        assert lib.univs_last_error().decode().startswith(MLP + ": M=")


# ---- the wrappers

def z(*shape):
    return torch.zeros(*shape)


def test_wrappers_answer_none_on_the_cpu_and_ops_keeps_its_public_set():
    ln = (torch.ones(256), z(256), 1e-5)
    assert ops.small_seam is seam_ops.small_seam
    assert ops.small_seam(z(4, 256), z(256, 256), None, z(4, 256), ln, z(768, 256)) is None
    lay = [(z(256, 256), None, False)]
    assert ops.small_mlp(z(4, 256), lay, pre_ln=(z(4, 256), ln[0], ln[1], 1e-5)) is None
    assert ops.small_mlp(z(4, 256), lay, side=(z(768, 256), None, (0, 256), None)) is None
    import inspect
    assert "small_seam" not in {n for n, f in vars(ops).items() if inspect.isfunction(f)}      # (tests/test_ops_contract_cpu.py pins that set)
    with pytest.raises(AttributeError):
        ops.no_such_wrapper


class _Stub:
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


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True), raising=False)
    monkeypatch.setattr(ops, "_stream_ptr", lambda t: "stream")
    splits = {}
    monkeypatch.setattr(ops, "presplit_weights", lambda w, **k: splits.setdefault(id(w), (torch.zeros(4), torch.zeros(4))))
    lib = _Stub(_lib.OK)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    lib.splits = splits
    return lib


def test_small_seam_hands_over_what_it_says(stub):
    x, res, add = z(6, 5, 256), z(6, 5, 256), z(6, 5, 256)
    wa, ba, wb, bb = z(256, 256), z(256), z(768, 256), z(768)
    ln = (torch.ones(256), z(256), 1e-5)
    with torch.no_grad():
        t, y = ops.small_seam(x, wa, ba, res, ln, wb, bb, add=add, add_features=512)
    assert tuple(t.shape) == (6, 5, 256) and tuple(y.shape) == (6, 5, 768)
    ((fn, a),) = stub.calls
    assert fn == SEAM and a[-1] == "stream" and a[-2] == y.data_ptr() and a[8] == t.data_ptr()
    assert a[0] == x.data_ptr() and a[1] == stub.splits[id(wa)][0].data_ptr() and a[3] == ba.data_ptr() and a[4] == res.data_ptr()
    assert a[5] == ln[0].data_ptr() and a[6] == ln[1].data_ptr() and abs(a[7] - 1e-5) < 1e-12 and a[9] == add.data_ptr()
    assert a[10] == stub.splits[id(wb)][0].data_ptr() and a[12] == bb.data_ptr() and list(a[13:21]) == [768, 0, 30, 256, 256, 768, 0, 512]
    stub.calls.clear()
    with torch.no_grad():
        t, y = ops.small_seam(x, wa, None, res, (ln[0], None, 1e-5), z(2048, 256), None, rows=(256, 1024), relu=True)
    a = stub.calls[0][1]
    assert tuple(y.shape) == (6, 5, 1024) and a[3] is None and a[6] is None and a[9] is None and list(a[13:21]) == [2048, 256, 30, 256, 256, 1024, 1, 0]
    stub.calls.clear()
    with torch.no_grad():
        for bad in (dict(rows=(0, 128)), dict(rows=(2, 256)), dict(rows=(512, 512)), dict(add=z(6, 5, 128)), dict(add_features=48)):
            assert ops.small_seam(x, wa, ba, res, ln, wb, bb, **bad) is None, bad
        assert ops.small_seam(x, wa[:, :128], ba, res, ln, wb, bb) is None and ops.small_seam(x, wa, ba, res[:3], ln, wb, bb) is None
        assert ops.small_seam(x, wa, ba, res, ln, wb[:256], bb[:256]) is None                   # a view of a parameter: no split of its own
        assert ops.small_seam(z(5000, 256), wa, ba, z(5000, 256), ln, wb, bb) is None
    assert ops.small_seam(x.requires_grad_(), wa, ba, res, ln, wb, bb) is None                 # autograd has to see these Linears
    assert stub.calls == []
    stub.code = _lib.ERR_NOT_IMPLEMENTED
    with torch.no_grad():
        assert ops.small_seam(z(6, 5, 256), wa, ba, res, ln, wb, bb) is None
    stub.code = _lib.ERR_LAUNCH
    with torch.no_grad(), pytest.raises(_lib.UnivsHipError, match=r"small_seam failed \(code -3\): stub"):
        ops.small_seam(z(6, 5, 256), wa, ba, res, ln, wb, bb)


def test_small_mlp_keywords_hand_over_what_they_say(stub):
    x, res, qpos = z(3, 2, 256), z(3, 2, 256), z(3, 2, 256)
    lay = [(z(256, 256), z(256), True), (z(256, 256), None, False)]
    g, b = torch.ones(256), z(256)
    wq, bq = z(768, 256), z(768)
    with torch.no_grad():
        y, xn, xr, q = ops.small_mlp(x, lay, in_ln=(g, b, 1e-5), want_normed=True, transpose01=True, pre_ln=(res, g, b, 1e-6),
                                     side=(wq, bq, (256, 256), qpos))
    assert tuple(y.shape) == (2, 3, 256) and tuple(xn.shape) == tuple(xr.shape) == tuple(q.shape) == (3, 2, 256)
    ((fn, a),) = stub.calls
    assert fn == MLP and a[-1] == "stream" and a[-2] == y.data_ptr() and list(a[-4:-2]) == [6, 2] and a[-5] == xn.data_ptr()
    assert a[0] == x.data_ptr() and a[1] == res.data_ptr() and a[2] == g.data_ptr() and a[3] == b.data_ptr() and abs(a[4] - 1e-6) < 1e-12
    assert a[5] == xr.data_ptr() and a[6] == qpos.data_ptr() and a[7] == stub.splits[id(wq)][0].data_ptr() and a[9] == bq.data_ptr()
    assert list(a[10:12]) == [768, 256] and a[12] == q.data_ptr() and a[13] == 2 and list(a[17]) == [1, 0, 0]
    stub.calls.clear()
    with torch.no_grad():
        r = ops.small_mlp(x, lay, side=(wq, None, None, None))
        assert r is None and stub.calls == []                                               # the whole packed weight is not 256 features
        y, xr = ops.small_mlp(x, lay, pre_ln=(res, g, b, 1e-5))
        a = stub.calls[0][1]
        assert a[6] is None and a[7] is None and a[12] is None and a[5] == xr.data_ptr() and a[-5] is None
        stub.calls.clear()
        assert ops.small_mlp(x, lay, pre_ln=(res[:1], g, b, 1e-5)) is None and ops.small_mlp(x, lay, pre_ln=(res, g, None, 1e-5)) is None
        assert ops.small_mlp(x, lay, side=(wq, bq, (0, 256), qpos[:1])) is None and ops.small_mlp(x, lay, side=(wq[:256], None, None, None)) is None
        assert stub.calls == []
        ops.small_mlp(x, lay)                                                                # without the keywords: the entry of univs_hip.h
        assert [c[0] for c in stub.calls] == ["univs_small_mlp_presplit_f32"]


# ---- what hipcc made of the kernels

def test_few_rows_kernels_keep_their_residency(tmp_path_factory):
    """No scratch, and at most 168 registers (three waves per SIMD, the `launch_bounds` of the family): csrc/small_linear.hip's header
    has what 256 registers cost."""
    lines, usage = listing(tmp_path_factory, "small_linear.hip")
    seam = [u for n, u in usage.items() if "small_seam_kernel" in n]
    chain = [u for n, u in usage.items() if "small_chain_kernel" in n]
    assert len(seam) == 1 and len(chain) == 1
    for u in seam + chain:
        assert u["VGPRs Spill"] == 0 and u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs"] <= 168, u
    for kernel in ("small_seam_kernel", "small_chain_kernel"):                              # three workgroups' LDS fit a CU's 160 KB
        at = next(i for i, l in enumerate(lines) if l.strip().startswith(".amdhsa_kernel") and kernel in l)
        lds = int(next(l for l in lines[at:] if ".amdhsa_group_segment_fixed_size" in l).split()[-1])
        assert 0 < 3 * lds <= 160 * 1024, (kernel, lds)


# ---- routing

def test_a_head_on_the_cpu_is_the_same_with_the_switch_on_and_off():
    from oracle.cpu_path import cpu_ops
    from univs_amd import workloads as cases
    case = dict(cases.HEAD_CASE, name="head_seams_cpu", Q=6)
    feats = cases.backbone_features(case)
    head = cases.build_head(case, "cpu", return_aux=False)
    with cpu_ops(), torch.no_grad():
        with override(decoder_seams=False):
            ref = head(feats, targets=cases.targets_first_clip(case))
        with override(decoder_seams=True):
            out = head(feats, targets=cases.targets_first_clip(case))
    for k in ("pred_masks", "pred_logits", "pred_embds"):
        assert torch.equal(out[k], ref[k]), k
