"""ctypes binding of libunivs_hip.so (the C ABI declared in include/univs_hip.h, include/univs_eval_hip.h,
include/univs_fused_hip.h, include/univs_pvos_hip.h, include/univs_semantic_hip.h, include/univs_encoder_hip.h,
include/univs_swin_hip.h, include/univs_frames_hip.h, include/univs_prompts_hip.h, include/univs_png_hip.h,
include/univs_hota_hip.h, include/univs_pngread_hip.h, include/univs_jpeg_hip.h, include/univs_jpegenc_hip.h, include/univs_idmap_hip.h,
include/univs_seam_hip.h, include/univs_imagelabels_hip.h, include/univs_text_hip.h and include/univs_polygons_hip.h).

The header is the one statement of the ABI: `SIGNATURES` (restype / argtypes of every `univs_*` symbol) and `CONFIG_FIELDS` (the
members of `struct UnivsConfig`) are read from its text when this module loads -- no table is kept by hand.
tests/capi_signatures.txt pins the result.

No fallback: if the shared library is missing or a symbol cannot be resolved this raises.  The
product path never routes through `oracle/` or a CPU implementation.
"""
import ctypes
import os
import re

# Load order matters: PyTorch-ROCm bundles its own libamdhip64 and must bring the HIP runtime into the
# process FIRST.  If libunivs_hip.so (linked against the system ROCm) is dlopen'ed before torch, two
# runtime instances coexist and launches on torch's streams fail with "no ROCm-capable device".
import torch  # noqa: F401  (kept first on purpose)

_HERE = os.path.dirname(os.path.abspath(__file__))
# UNIVS_HIP_LIB: debug override (tools/msda_trace.py loads an instrumented build of the same sources)
LIB_PATH = os.environ.get("UNIVS_HIP_LIB") or os.path.join(_HERE, "libunivs_hip.so")

OK = 0
ERR_INVALID_ARGUMENT = -1
ERR_NOT_IMPLEMENTED = -2
ERR_LAUNCH = -3

# The binding is read from the public header when this module loads: the header is the one statement of the ABI.
HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_hip.h")
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float,
            "uint32_t": ctypes.c_uint32}
_RETURNS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "const char*": ctypes.c_char_p}
_STRUCT = r"typedef struct UnivsConfig \{(.*?)\} UnivsConfig;"


def strip_header(text):
    """The header without its comments, preprocessor lines and extern "C" braces."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    return re.sub(r"^[ \t]*(#.*|extern \"C\" \{|\})[ \t]*$", "", text, flags=re.M)


def parse_signatures(text):
    """name -> (restype, argtypes) of every `univs_*` prototype in the header `text`.  Any pointer parameter is a c_void_p;
    a type outside the two maps raises and names the symbol -- it is never guessed."""
    def ctype(words, table, name):
        t = " ".join(words).replace(" *", "*")
        if t.endswith("*") and table is _SCALARS:
            return ctypes.c_void_p
        if t not in table:
            raise TypeError(f"{name}: type {t!r} in include/univs_hip.h has no ctypes mapping")
        return table[t]

    sigs = {}
    text = re.sub(_STRUCT, "", strip_header(text), flags=re.S)
    for ret, name, params in re.findall(r"([\w \t*]+?)\b(univs_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [] if params.strip() == "void" else [p.replace("*", " * ").split()[:-1] for p in params.split(",")]   # [:-1]: the name
        sigs[name] = (ctype(ret.replace("*", " * ").split(), _RETURNS, name), [ctype(p, _SCALARS, name) for p in params])
    return sigs


def parse_config_fields(text):
    """The members of `struct UnivsConfig` as ctypes fields: plain ints and int arrays (`reserved[2]`)."""
    fields = []
    for decl in re.search(_STRUCT, strip_header(text), flags=re.S).group(1).split(";")[:-1]:
        m = re.fullmatch(r"\s*int\s+(\w+)\s*(?:\[(\d+)\])?\s*", decl)
        if not m:
            raise TypeError(f"UnivsConfig: member {decl.strip()!r} in include/univs_hip.h is not an int or an int array")
        fields.append((m.group(1), ctypes.c_int * int(m.group(2)) if m.group(2) else ctypes.c_int))
    return fields


with open(HEADER_PATH) as _f:
    _HEADER = _f.read()
SIGNATURES = parse_signatures(_HEADER)
CONFIG_FIELDS = parse_config_fields(_HEADER)
# The second header (include/univs_eval_hip.h: the entries added after the first one's symbols were pinned) has a table of its own.
EVAL_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_eval_hip.h")
with open(EVAL_HEADER_PATH) as _f:
    EVAL_SIGNATURES = parse_signatures(_f.read())
# The third header (include/univs_fused_hip.h: consumers that fold a producer's transform into their operand load), likewise.
FUSED_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_fused_hip.h")
with open(FUSED_HEADER_PATH) as _f:
    FUSED_SIGNATURES = parse_signatures(_f.read())
# The fourth header (include/univs_pvos_hip.h: the panoptic-VOS counts; the three above are pinned symbol by symbol), likewise.
PVOS_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_pvos_hip.h")
with open(PVOS_HEADER_PATH) as _f:
    PVOS_SIGNATURES = parse_signatures(_f.read())
# The fifth header (include/univs_semantic_hip.h: the mask-quality counts of the semantic-feature decoder), likewise.
SEMANTIC_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_semantic_hip.h")
with open(SEMANTIC_HEADER_PATH) as _f:
    SEMANTIC_SIGNATURES = parse_signatures(_f.read())
# The sixth header (include/univs_encoder_hip.h: the two projections at the head of a deformable-encoder layer in one launch), likewise.
ENCODER_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_encoder_hip.h")
with open(ENCODER_HEADER_PATH) as _f:
    ENCODER_SIGNATURES = parse_signatures(_f.read())
# The seventh header (include/univs_swin_hip.h: Swin window attention that computes q, k, v from the tokens itself), likewise.
SWIN_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_swin_hip.h")
with open(SWIN_HEADER_PATH) as _f:
    SWIN_SIGNATURES = parse_signatures(_f.read())
# The eighth header (include/univs_frames_hip.h: the test-time resize of decoded frames), likewise.
FRAMES_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_frames_hip.h")
with open(FRAMES_HEADER_PATH) as _f:
    FRAMES_SIGNATURES = parse_signatures(_f.read())
# The ninth header (include/univs_prompts_hip.h: the first-frame masks of a VOS video, resized from their run-length codes), likewise.
PROMPTS_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_prompts_hip.h")
with open(PROMPTS_HEADER_PATH) as _f:
    PROMPTS_SIGNATURES = parse_signatures(_f.read())
# The tenth header (include/univs_png_hip.h: the zlib streams of result PNGs, encoded from the id maps), likewise.
PNG_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_png_hip.h")
with open(PNG_HEADER_PATH) as _f:
    PNG_SIGNATURES = parse_signatures(_f.read())
# The eleventh header (include/univs_hota_hip.h: the HOTA tables of a video and the batched assignment solver), likewise.
HOTA_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_hota_hip.h")
with open(HOTA_HEADER_PATH) as _f:
    HOTA_SIGNATURES = parse_signatures(_f.read())
# The twelfth header (include/univs_pngread_hip.h: label PNGs inflated and unfiltered on the device), likewise.
PNGREAD_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_pngread_hip.h")
with open(PNGREAD_HEADER_PATH) as _f:
    PNGREAD_SIGNATURES = parse_signatures(_f.read())
# The thirteenth header (include/univs_jpeg_hip.h: baseline JPEG frames decoded on the device), likewise.
JPEG_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_jpeg_hip.h")
with open(JPEG_HEADER_PATH) as _f:
    JPEG_SIGNATURES = parse_signatures(_f.read())
# The fourteenth header (include/univs_jpegenc_hip.h: baseline JPEG files encoded on the device, with the result overlay), likewise.
JPEGENC_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_jpegenc_hip.h")
with open(JPEGENC_HEADER_PATH) as _f:
    JPEGENC_SIGNATURES = parse_signatures(_f.read())
# The fifteenth header (include/univs_idmap_hip.h: the census of a VOS video's id maps and the prompt masks gathered from them), likewise.
IDMAP_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_idmap_hip.h")
with open(IDMAP_HEADER_PATH) as _f:
    IDMAP_SIGNATURES = parse_signatures(_f.read())
# The sixteenth header (include/univs_seam_hip.h: the seams of a decoder layer, two few-rows kernels in one launch), likewise.
SEAM_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_seam_hip.h")
with open(SEAM_HEADER_PATH) as _f:
    SEAM_SIGNATURES = parse_signatures(_f.read())
# The seventeenth header (include/univs_imagelabels_hip.h: the labels of a per-image semantic result and the confusion matrix of two
# label maps), likewise.  (IMAGELABELS_BINDING, not *_SIGNATURES: the sixteenth header's test counts the tables of that name it is
# disjoint from; tests/test_imagelabels_capi_cpu.py checks this one against all of them.)
IMAGELABELS_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_imagelabels_hip.h")
with open(IMAGELABELS_HEADER_PATH) as _f:
    IMAGELABELS_BINDING = parse_signatures(_f.read())
# The eighteenth header (include/univs_text_hip.h: causal attention over packed sequences of unequal length, the CLIP text tower's core),
# likewise (TEXT_BINDING, for the same reason).
TEXT_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_text_hip.h")
with open(TEXT_HEADER_PATH) as _f:
    TEXT_BINDING = parse_signatures(_f.read())
# The nineteenth header (include/univs_polygons_hip.h: polygon segmentations to run-length boundaries, one workgroup per object), likewise
# (POLYGONS_BINDING, for the same reason).
POLYGONS_HEADER_PATH = os.path.join(_HERE, "..", "include", "univs_polygons_hip.h")
with open(POLYGONS_HEADER_PATH) as _f:
    POLYGONS_BINDING = parse_signatures(_f.read())

_lib = None


class UnivsHipError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle.  Raises if the library is absent -- build it with
    `python -m univs_amd.build` (or `__graft_entry__.build()`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise UnivsHipError(
            f"{LIB_PATH} not found: the HIP extension is mandatory (no CPU fallback). "
            "Build it with `python -m univs_amd.build`.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in (*SIGNATURES.items(), *EVAL_SIGNATURES.items(), *FUSED_SIGNATURES.items(),
                              *PVOS_SIGNATURES.items(), *SEMANTIC_SIGNATURES.items(), *ENCODER_SIGNATURES.items(), *SWIN_SIGNATURES.items(),
                              *FRAMES_SIGNATURES.items(), *PROMPTS_SIGNATURES.items(), *PNG_SIGNATURES.items(), *HOTA_SIGNATURES.items(),
                              *PNGREAD_SIGNATURES.items(), *JPEG_SIGNATURES.items(), *JPEGENC_SIGNATURES.items(), *IDMAP_SIGNATURES.items(),
                              *SEAM_SIGNATURES.items(), *IMAGELABELS_BINDING.items(), *TEXT_BINDING.items(), *POLYGONS_BINDING.items()):
        fn = getattr(lib, name)  # AttributeError if the symbol is missing -> loud
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc == OK:
        return
    msg = load().univs_last_error().decode("utf-8", "replace")
    if rc == ERR_NOT_IMPLEMENTED:
        raise NotImplementedError(f"{what}: {msg}")
    raise UnivsHipError(f"{what} failed (code {rc}): {msg}")
