"""CPU: the arithmetic contract of the three-product GEMM family exists once (csrc/f16x3.h, csrc/f16x3_wstream.h, csrc/f16x3_kstep.h),
from the source text, and tools/isa_compare.py tells an unchanged kernel from a changed one:
  (a) in the family's sources the matrix builtin of the products occurs only in f16x3.h and on mlp_f16x3.hip's ML_PS_MMA line, the
      LDS-DMA instruction only in f16x3_wstream.h, and the counted LDS wait only in f16x3_wstream.h and f16x3_kstep.h;
  (b) the literals of the running-scale rule are spelled out in none of the family's .hip files;
  (c) isa_compare.py reports both kernels of conv3x3_wide.hip identical for a clean tree of HEAD against HEAD (exit status 0), and a
      difference (exit status 1) for a copy with one sched_barrier removed.
The family: every .hip that includes one of the three headers, without the attention kernels (window_attn*.hip, cross_attn.hip,
proca_attn.hip), whose cores are their own."""
import fnmatch
import io
import os
import re
import shutil
import subprocess
import sys
import tarfile

import pytest

from univs_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("f16x3.h", "f16x3_kstep.h", "f16x3_wstream.h")
ATTENTION = ("window_attn*.hip", "cross_attn.hip", "proca_attn.hip")
MFMA = "__builtin_amdgcn_mfma_f32_16x16x32_f16"


def _text(name):
    with open(os.path.join(build.CSRC, name)) as f:
        return f.read()


def _code_lines(name):
    """the file's lines without their // comments"""
    return [ln.split("//", 1)[0] for ln in _text(name).split("\n")]


def _family():
    out = []
    for name in sorted(os.listdir(build.CSRC)):
        if name.endswith(".hip") and not any(fnmatch.fnmatch(name, p) for p in ATTENTION):
            if re.search(r'#include "(%s)"' % "|".join(re.escape(h) for h in HEADERS), _text(name)):
                out.append(name)
    return out


def test_the_family_is_the_expected_set_of_sources_and_the_headers_are_built_with():
    fam = _family()
    for name in ("linear_f16x3.hip", "linear_pair_f16x3.hip", "gemm_f16x3_stream.hip", "gemm_f16x3_tile.hip", "mlp_f16x3.hip",
                 "linear_pair_xres.hip", "conv3x3_wide.hip", "small_linear.hip"):
        assert name in fam, (name, fam)
    for h in HEADERS:
        assert any(os.path.basename(p) == h for p in build.HEADERS), h


def test_product_builtin_dma_and_counted_wait_occur_in_the_shared_headers_only():
    where = {"mfma": set(), "dma": set(), "wait": set()}
    for name in _family() + list(HEADERS):
        for ln in _code_lines(name):
            if MFMA in ln and not (name == "mlp_f16x3.hip" and "ML_PS_MMA" in ln):
                where["mfma"].add(name)
            if "global_load_lds" in ln:
                where["dma"].add(name)
            if "s_waitcnt lgkmcnt(" in ln:
                where["wait"].add(name)
    assert where["mfma"] == {"f16x3.h"}, where
    assert where["dma"] == {"f16x3_wstream.h"}, where
    assert where["wait"] == {"f16x3_wstream.h", "f16x3_kstep.h"}, where
    # the one exception is one macro definition, and the phase-shifted kernel alone uses it
    defs = [ln for ln in _code_lines("mlp_f16x3.hip") if MFMA in ln]
    assert len(defs) == 1 and defs[0].lstrip().startswith("#define ML_PS_MMA("), defs


def test_scale_rule_literals_are_not_restated_in_the_kernels():
    for name in _family():
        text = _text(name)
        assert "127 + 12 -" not in text and "127 - 12 +" not in text, name
        assert not re.search(r"eset[^\n;]*\+ 2\)", text), name
        assert not re.search(r"max\(-100, min\(", text) and "-126)" not in text, name
    kstep = _text("f16x3_kstep.h")
    assert "127 + 12" not in kstep and "127 - 12" not in kstep and not re.search(r"eset[^\n;]*\+ 2\)", kstep)
    assert re.search(r"constexpr int L3_SCALE_SET = 12, L3_SCALE_MARGIN = 2, L3_EXP_MIN = -100, L3_EXP_MAX = 128, L3_RATIO_MIN = -126;",
                     _text("f16x3.h"))


def _git_head_tree(dst):
    """univs_amd/csrc and include of HEAD under dst; False without git or a repository"""
    if shutil.which("git") is None:
        return False
    p = subprocess.run(["git", "-C", ROOT, "archive", "HEAD", "univs_amd/csrc", "include"], capture_output=True, timeout=120)
    if p.returncode != 0:
        return False
    with tarfile.open(fileobj=io.BytesIO(p.stdout)) as t:
        t.extractall(dst)
    return True


def test_isa_compare_tells_identical_from_changed(tmp_path):
    try:
        build._hipcc()
    except RuntimeError:
        pytest.skip("no hipcc")
    clean, changed = str(tmp_path / "clean"), str(tmp_path / "changed")
    os.makedirs(clean)
    if not _git_head_tree(clean):
        pytest.skip("no git repository")
    shutil.copytree(clean, changed)
    src = os.path.join(changed, "univs_amd", "csrc", "conv3x3_wide.hip")
    with open(src) as f:
        text = f.read()
    assert text.count("__builtin_amdgcn_sched_barrier(0);") >= 2
    with open(src, "w") as f:
        f.write(text.replace("__builtin_amdgcn_sched_barrier(0);", "", 1))

    def run(tree):
        return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_compare.py"), "HEAD", "conv3x3_wide.hip", "--tree", tree],
                              capture_output=True, text=True, timeout=600)

    same = run(clean)
    rows = [ln for ln in same.stdout.split("\n") if ln.startswith("  conv3x3_wide.hip")]
    assert same.returncode == 0 and len(rows) == 2, same.stdout + same.stderr
    assert all(" identical " in r and r.rstrip().endswith(" same") for r in rows), same.stdout
    diff = run(changed)
    rows = [ln for ln in diff.stdout.split("\n") if ln.startswith("  conv3x3_wide.hip")]
    assert diff.returncode == 1 and len(rows) == 2, diff.stdout + diff.stderr
    assert any("lines differing" in r for r in rows), diff.stdout
