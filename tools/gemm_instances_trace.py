"""Condense the kernel_stats CSV of
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python -m pytest tests/test_gemm_instances_gpu.py
into profiles/gemm_instances_trace_v*.txt: one line `<instantiation> <calls>` per kernel of the three-product GEMM family, named as
tests/gemm_instances.py names them.      python tools/gemm_instances_trace.py out > profiles/gemm_instances_trace_v1.txt"""
import csv
import glob
import re
import sys

FAMILY = "linear_f16x3|linear_bf16x6|gemm_f16x3_stream|gemm_f16x3_tile|mlp_f16x3_ps|mlp_f16x3"


def instantiation(demangled):
    m = re.search(r"univs::(" + FAMILY + r")<([^>]*)>", demangled)
    if not m:
        return None
    args = [{"true": "1", "false": "0"}.get(a.strip(), a.strip()) for a in m.group(2).split(",")]
    args = [re.sub(r"^\(\w+\)", "", a) for a in args]
    if m.group(1) == "gemm_f16x3_stream" and args[-1] == "0":
        args = args[:-1]                       # (AFF = false: the name tools/gemm_plan_dump.cpp prints)
    return f"{m.group(1)}<{','.join(args)}>"


def main():
    files = glob.glob(sys.argv[1] + "/**/*kernel_stats.csv", recursive=True)
    calls = {}
    for r in csv.DictReader(open(files[0])):
        inst = instantiation(r["Name"])
        if inst:
            calls[inst] = calls.get(inst, 0) + int(r["Calls"])
    print("# kernels of the three-product GEMM family launched by one run of tests/test_gemm_instances_gpu.py (rocprofv3 --kernel-trace --stats)")
    print("# instantiation calls")
    for k in sorted(calls):
        print(k, calls[k])


if __name__ == "__main__":
    main()
