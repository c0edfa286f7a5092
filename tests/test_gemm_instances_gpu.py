"""GPU: every compiled kernel of the three-product GEMM family (tests/gemm_instances.py: one case per instantiation, routed by the
settings the case names; tests/test_gemm_instances_cpu.py pins that the case selects that kernel at any CU count) against fp64.

Per case:
  plain     x ~ N(0, 1), w ~ N(0, 1 / K), bias, residual as in test_linear_fused_matches_torch; reference = the fp64 Linear / convolution /
            two-Linear MLP with the epilogue in fp64; err < max(4 err32, 5e-6), err32 = ATen's fp32 result against the same reference.
  moving    (the kernels with a running row scale; epilogues none / ReLU / residual / blocked) the inputs of
            gemm_instances.moving_scale_inputs; the error element-wise relative to |x| |w|^T + |b| (the MLP: |h| |w2|^T + |b2|), as
            test_linear_f16x3_row_scaling measures it: e3 < max(4 e32, 3e-7) -- the factor is the family's own, the floor the per-product
            bound 2^-21.7 of linear_f16x3.hip; the CPU file shows the bound holds for the reference arithmetic (e3 <= 1.5e-7 there).
            The operand-affine kernels get the moving scale through GroupNorm's weight, and their reference is the fp64 convolution of
            the materialised relu(group_norm(x)): the GroupNorm in front fixes the scale of x itself.
  identity  torch.equal with the sibling the project claims the same bits for: PRE against raw W (asserted in the PRE case), tile against stream (linear_ablate = 6),
            a channels-last against an NCHW operand (in the XMODE 2 case), the operand affine against group_norm(relu=True) + the plain convolution, the
            blocked output against the permuted standard layout, the phase-shifted MLP against the lockstep one.
  padding   every tensor a wrapper allocates lies inside a larger NaN-filled buffer (256 floats in front and behind, 16-byte aligned):
            the padding is still NaN afterwards, and an output element the kernel did not write fails the error bound as NaN.
Every line printed is `GI <case> <kernel> err err32 e3 e32` (profiles/gemm_instances_v1.txt)."""
import contextlib
import math

import pytest
import torch

from tests import gemm_instances as gi
from univs_amd import fused_ops, ops
from univs_amd.switches import override

pytestmark = pytest.mark.gpu
F = torch.nn.functional
PAD = 256


@contextlib.contextmanager
def nan_padded_outputs():
    """Inside the block every float32 GPU tensor from torch.empty -- what the wrappers allocate their outputs with -- is a slice of a
    larger buffer of NaN; yields the list of (buffer, first element, elements)."""
    real, made = torch.empty, []

    def empty(*size, **kw):
        dev = kw.get("device")
        if kw.get("dtype") != torch.float32 or dev is None or torch.device(dev).type != "cuda" or set(kw) - {"dtype", "device"}:
            return real(*size, **kw)
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        n = math.prod(shape)
        buf = real(2 * PAD + (n + 3) // 4 * 4, dtype=torch.float32, device=dev)
        buf.fill_(float("nan"))
        made.append((buf, n))
        return buf[PAD:PAD + n].view(shape)
    torch.empty = empty
    try:
        yield made
    finally:
        torch.empty = real


def _wrapper(c, t):
    call = c["call"]
    if call == "linear_fused":
        return ops.linear_fused(t["x"], t["w"], t["b"], act=c["epi"] if c["epi"] in ("relu", "gelu") else None,
                                residual=t["r"] if c["epi"] == "residual" else None)
    if call == "linear_blocked":
        return ops.linear_blocked(t["x"], t["w"], t["b"], c["shape"][3], c["shape"][4])
    if call == "conv3x3":
        return ops.conv3x3(t["x"], t["w"])
    if call == "conv1x1":
        return ops.conv1x1(t["x"], t["w"], t["b"])
    if call == "conv1x1_fused":
        return fused_ops.conv1x1_fused(t["x_cl"] if c["channels_last"] else t["x"], t["w"], t["b"], t.get("affine"))
    assert call == "mlp_fused", call
    return ops.mlp_fused(t["x"], t["w"], t["b"], t["w2"], t["b2"], c["epi"], residual=t["r"] if c["residual"] else None)


def run(c, t, fn=None, switches=None, config=None):
    """The case's wrapper (or `fn`) under its settings (overridden by `switches` / `config`), outputs NaN-padded; never None"""
    with override(**{**c["switches"], **(switches or {})}), ops.configured(**{**c["config"], **(config or {})}), nan_padded_outputs() as made:
        y = fn() if fn else _wrapper(c, t)
    assert y is not None, "the wrapper answered None: the case is not covered"
    assert made, "the wrapper allocated no output through torch.empty"
    for buf, n in made:
        assert torch.isnan(buf[:PAD]).all() and torch.isnan(buf[PAD + n:]).all(), "a kernel wrote into the padding around its output"
    return y


def _dev(t, cuda):
    return {k: (v.to(cuda) if v is not None else None) for k, v in t.items()}


# ---- the three kinds of case: inputs on the GPU, the kernel's result as rows [M, N], the two references and the error's own scale
def _linear(c, cuda, moving):
    M, K, N = c["shape"][:3]
    x, w, b, r = (gi.moving_scale_inputs if moving else gi.plain_inputs)(M, K, N, c["id"])
    t = _dev({"x": x, "w": w, "b": b, "r": r}, cuda)

    def rows(y):
        return y.permute(0, 2, 1, 3).reshape(M, N) if c["epi"] == "blocked" else y.view(M, N)

    def ref(dt):
        y = F.linear(t["x"].to(dt), t["w"].to(dt), t["b"].to(dt))
        y = F.gelu(y) if c["epi"] == "gelu" else y.relu() if c["epi"] == "relu" else y
        return y + t["r"].to(dt) if c["epi"] == "residual" else y
    scale = t["x"].double().abs() @ t["w"].double().abs().t() + t["b"].double().abs()[None]
    return t, rows, ref, scale


def _conv(c, cuda, moving):
    T, Cin, Cout, H, W = c["shape"]
    M, taps = T * H * W, 9 if c["call"] == "conv3x3" else 1
    gen = gi.moving_scale_inputs if moving and not c["affine"] else gi.plain_inputs
    x = gen(M, Cin, Cout, c["id"])[0].view(T, H, W, Cin)                      # a row = a pixel: the scale moves along the channels
    _, w, b, _ = (gi.moving_scale_inputs if moving else gi.plain_inputs)(16, taps * Cin, Cout, c["id"] + "/w")
    t = _dev({"x_cl": x.permute(0, 3, 1, 2), "w": w.view(Cout, Cin, *((3, 3) if taps == 9 else (1, 1))), "b": b if c["epi"] == "bias" else None},
             cuda)
    t["x"] = t["x_cl"].contiguous()
    assert not t["x_cl"].is_contiguous()
    operand = t["x"]
    if c["affine"]:
        g = torch.Generator().manual_seed(Cin)
        gamma, beta = 1.0 + 0.2 * torch.randn(Cin, generator=g), 0.1 * torch.randn(Cin, generator=g)
        if moving:
            gamma = gamma * torch.logspace(-2, 2, Cin)
        t["gamma"], t["beta"] = gamma.to(cuda), beta.to(cuda)
        t["affine"] = ops.group_norm_affine(t["x"], 32, t["gamma"], t["beta"], 1e-5)
        t["normed"] = ops.group_norm(t["x"], 32, t["gamma"], t["beta"], 1e-5, relu=True)
        if moving:
            operand = t["normed"]                                              # (the fp64 convolution of the materialised operand)

    def rows(y):
        return y.permute(0, 2, 3, 1).reshape(M, y.shape[1])

    def ref(dt):
        xo = operand.to(dt)
        if c["affine"] and not moving:
            xo = F.group_norm(xo, 32, t["gamma"].to(dt), t["beta"].to(dt), 1e-5).relu()
        bias = t["b"].to(dt) if t["b"] is not None else None
        if taps == 9:
            return rows(F.conv2d(xo, t["w"].to(dt), bias, 1, 1))
        return F.linear(rows(xo), t["w"].to(dt).view(Cout, Cin), bias)          # a 1 x 1 is the Linear of its pixels (no solver search)
    xa = (t["normed"] if c["affine"] else t["x"]).double().abs()
    if taps == 9:
        scale = rows(F.conv2d(xa, t["w"].double().abs(), None, 1, 1))
    else:
        scale = rows(xa) @ t["w"].double().abs().view(Cout, Cin).t()
    if t["b"] is not None:
        scale = scale + t["b"].double().abs()[None]
    return t, rows, ref, scale


def _mlp(c, cuda, moving):
    M, C, Hd = c["shape"]
    gen = gi.moving_scale_inputs if moving else gi.plain_inputs
    x, w1, b1, _ = gen(M, C, Hd, c["id"] + "/1")
    _, w2, b2, r = gi.plain_inputs(M, Hd, C, c["id"] + "/2")
    if moving:
        w2 = w2 * torch.logspace(-3, 3, C).view(C, 1)
        r = r * x.abs().amax(1, keepdim=True) * 0.01
    t = _dev({"x": x, "w": w1, "b": b1, "w2": w2, "b2": b2, "r": r}, cuda)
    act = F.relu if c["epi"] == "relu" else F.gelu

    def hidden(dt):
        return act(F.linear(t["x"].to(dt), t["w"].to(dt), t["b"].to(dt)))

    def ref(dt):
        y = F.linear(hidden(dt), t["w2"].to(dt), t["b2"].to(dt))
        return y + t["r"].to(dt) if c["residual"] else y
    scale = hidden(torch.float64).abs() @ t["w2"].double().abs().t() + t["b2"].double().abs()[None]
    return t, (lambda y: y.view(M, C)), ref, scale


def _siblings(c, t, y):
    """The bit identities: (what, the sibling's result shaped as y)"""
    inst = c["inst"]
    if c["epi"] == "blocked":
        M, K, N, rows, cb = c["shape"]
        std = run(c, t, fn=lambda: ops.linear_fused(t["x"], t["w"], t["b"]))
        yield "the permuted standard layout", std.view(M // rows, rows, N // cb, cb).permute(0, 2, 1, 3)
    if inst.startswith("linear_f16x3") and c["switches"]["resident_presplit"]:
        yield "the same <RB, ring> splitting W itself (PRE = false)", run(c, t, switches={"resident_presplit": False})
    if inst.startswith("gemm_f16x3_tile"):
        yield "the streamed kernel (linear_ablate = 6)", run(c, t, config={"linear_ablate": 6})
    if inst.startswith("mlp_f16x3_ps"):
        yield "the lockstep MLP kernel", run(c, t, config={"linear_ablate": 0})
    if c["call"] in ("conv1x1", "conv1x1_fused"):
        if c["affine"]:
            yield "group_norm(relu=True) + the plain convolution", run(c, t, fn=lambda: ops.conv1x1(t["normed"], t["w"], t["b"]))
        elif c["channels_last"]:
            yield "the NCHW operand (XMODE 1)", run(c, t, fn=lambda: ops.conv1x1(t["x"], t["w"], t["b"]))


@pytest.mark.parametrize("c", gi.CASES, ids=lambda c: c["id"])
def test_every_instantiation_against_fp64(cuda, linear_terms, c):
    linear_terms(c["config"].get("linear_terms", 3))
    build = _mlp if c["call"] == "mlp_fused" else _linear if c["call"].startswith("linear") else _conv
    figures, failures = {}, []
    for moving in ((False, True) if gi.carries_row_scale(c) else (False,)):
        t, rows, ref, scale = build(c, cuda, moving)
        y = run(c, t)
        ref64 = ref(torch.float64)
        d, d32 = (rows(y).double() - ref64).abs(), (ref(torch.float32).double() - ref64).abs()
        if moving:
            e3, e32 = (d / (scale + 1e-300)).max().item(), (d32 / (scale + 1e-300)).max().item()
            figures.update(e3=e3, e32=e32)
            if not e3 < max(4.0 * e32, 3e-7):
                failures.append(f"moving scale: e3 {e3:.3e} against max(4 x {e32:.3e}, 3e-7)")
        else:
            err, err32 = d.max().item(), d32.max().item()
            figures.update(err=err, err32=err32)
            if not err < max(4.0 * err32, 5e-6):
                failures.append(f"plain: err {err:.3e} against max(4 x {err32:.3e}, 5e-6)")
        for what, other in _siblings(c, t, y):
            if not (other.shape == y.shape and torch.equal(other, y)):
                failures.append(f"{'moving' if moving else 'plain'} inputs: not the bits of {what} "
                                f"(largest difference {(other.double() - y.double()).abs().max().item():.3e})")
    print("GI", c["id"], c["inst"], *(f"{figures[k]:.3e}" if k in figures else "-" for k in ("err", "err32", "e3", "e32")))
    assert not failures, c["inst"] + ":\n  " + "\n  ".join(failures)
