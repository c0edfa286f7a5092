"""CPU: the host contract of the C ABI and its ctypes binding, pinned against the commit before the entries of csrc/capi.hip were folded
into one skeleton and the binding was read from the header.

tests/capi_contract_table.txt: what every entry answers (return code, univs_last_error()) to NULL data pointers with bad, empty and valid
shapes (univs_configure: to host structs), printed by tools/capi_contract_dump.py from that commit's library.  No row gets past an entry's NULL check, so nothing is launched.
tests/capi_signatures.txt: that commit's hand-typed ctypes table, one line per symbol: return code and argument codes (P pointer, I int,
L long long, F float, U uint32, S C string)."""
import contextlib
import ctypes
import importlib.util
import io
import os
import re

import pytest

from univs_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = {ctypes.c_void_p: "P", ctypes.c_int: "I", ctypes.c_longlong: "L", ctypes.c_float: "F", ctypes.c_uint32: "U", ctypes.c_char_p: "S"}


def signature_lines(sigs):
    return [f"{n} {CODES[r]} {''.join(CODES[a] for a in args) or '-'}" for n, (r, args) in sorted(sigs.items())]


def test_contract_table_is_the_recorded_one():
    build.build()
    spec = importlib.util.spec_from_file_location("capi_contract_dump", os.path.join(ROOT, "tools", "capi_contract_dump.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        tool.main()
    got = out.getvalue().splitlines()
    want = open(os.path.join(ROOT, "tests", "capi_contract_table.txt")).read().splitlines()
    assert len(want) > 450 and not any(line.split(" | ")[2] == str(_lib.ERR_LAUNCH) for line in want)   # nothing in it reached a launcher
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


def test_signatures_read_from_the_header_are_the_recorded_ones():
    want = open(os.path.join(ROOT, "tests", "capi_signatures.txt")).read().splitlines()
    assert len(want) == 76
    assert signature_lines(_lib.SIGNATURES) == want


@pytest.mark.parametrize("prototype, what", [
    ("int univs_new_entry(const float* x, double eps, void* stream);", "univs_new_entry.*'double'"),
    ("int univs_new_entry(const float* x, unsigned n, void* stream);", "univs_new_entry.*'unsigned'"),
    ("float* univs_new_entry(int n);", "univs_new_entry.*'float\\*'"),
])
def test_a_type_outside_the_map_is_an_error_that_names_the_symbol(prototype, what):
    with pytest.raises(TypeError, match=what):
        _lib.parse_signatures("/* a header */\n#include <stdint.h>\nint univs_known(int n);\n" + prototype)


def test_prototypes_inside_comments_are_not_bound():
    sigs = _lib.parse_signatures("/* int univs_a(int n); */\n// int univs_b(int n);\nint univs_c(int n);  // int univs_d(double x);\n")
    assert list(sigs) == ["univs_c"]


def test_config_fields_are_the_members_of_the_headers_struct():
    from univs_amd import ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "univs_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct UnivsConfig \{(.*?)\}", text, flags=re.S).group(1)
    members = re.findall(r"\bint\s+(\w+)", body)
    assert members[0] == "size" and members[-1] == "reserved" and len(members) == 19
    assert [n for n, _ in ops.UnivsConfig._fields_] == members
    assert ctypes.sizeof(ops.UnivsConfig) == 4 * (len(members) + 1)          # plain ints and `int reserved[2]`
    build.build()
    assert list(ops.get_config()) == members[1:-1]
    with pytest.raises(TypeError, match="UnivsConfig"):
        _lib.parse_config_fields("typedef struct UnivsConfig {\n  int size;\n  float scale;\n} UnivsConfig;")
