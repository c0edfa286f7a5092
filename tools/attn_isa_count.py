"""Instruction counts of the attention kernels' loops from a `hipcc -S` listing, by class.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -S --cuda-device-only univs_amd/csrc/cross_attn.hip -o x.s
    python tools/attn_isa_count.py x.s xattn_partial

Per kernel whose name contains the pattern: the loop with the most matrix instructions (the 32-key iteration of xattn_partial, the
query-block loop of window_attn_img_f16), counted twice -- every instruction of the loop's basic blocks (`static`: the rarely taken
blocks included), and the instructions of the path an ordinary iteration takes (`hot`): at a conditional branch the
side whose block carries the kernels' `; rare` marker (an assembly comment the source puts into the range-scale, maximum-raise and
partial-iteration blocks) is not followed.  Listings of sources without the markers have the static count only."""
import collections
import re
import sys

LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^s_(cbranch_\w+|branch) (\.LBB\d+_\d+)")
BLOCK = re.compile(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)")          # a basic block's first line; hipcc notes the loop it belongs to beside it


def bodies(path):
    lines = open(path).read().splitlines()
    out, i = {}, 0
    while i < len(lines):
        l = lines[i]
        if l.startswith("_Z") and l.split(";")[0].strip().endswith(":"):
            j = i
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            out[l.split(":")[0]] = [x.strip() for x in lines[i:j]]
            i = j
        i += 1
    return out


def block_loops(body):
    """line -> header label of the innermost loop its basic block belongs to (None outside loops), from hipcc's block annotations"""
    out, cur = [], None
    for i, l in enumerate(body):
        if BLOCK.match(l):
            note = " ".join(body[i:i + 3]) if LABEL.match(l) else l
            m = re.search(r"in Loop: Header=(BB\d+_\d+)", l)
            cur = ".L" + m.group(1) if m else (LABEL.match(l).group(1) if LABEL.match(l) and "Loop Header" in note else None)
        out.append(cur)
    return out


def main_loop(body):
    """header label of the loop with the most matrix instructions in its own blocks"""
    loops = block_loops(body)
    count = collections.Counter(h for l, h in zip(body, loops) if h and l.startswith("v_mfma"))
    return count.most_common(1)[0][0]


def is_instruction(l):
    return bool(l) and not l.startswith((";", ".")) and not l.endswith(":") and not LABEL.match(l)


def in_loop_lines(body, header):
    """the lines of the loop's own basic blocks, wherever they are laid out"""
    return [l for l, h in zip(body, block_loops(body)) if h == header]


def classes(seg):
    c = collections.Counter()
    for l in seg:
        if not is_instruction(l):
            continue
        op = l.split()[0]
        for prefix, name in (("v_mfma", "mfma"), ("v_exp", "v_exp"), ("v_fma_mix", "v_fma_mix"), ("v_cvt", "v_cvt"), ("v_cmp", "v_cmp/cndmask"),
                             ("v_cndmask", "v_cmp/cndmask"), ("v_", "valu other"), ("ds_", "lds"), ("global_", "vmem"), ("buffer_", "vmem"),
                             ("scratch_", "scratch"), ("s_nop", "s_nop"), ("s_waitcnt", "s_waitcnt"), ("s_", "salu")):
            if op.startswith(prefix):
                c[name] += 1
                break
    c["total"] = sum(c.values())
    return c


def hot_path(body, header):
    """the lines an iteration executes when no `; rare` block is entered"""
    labels = {LABEL.match(l).group(1): i for i, l in enumerate(body) if LABEL.match(l)}
    loops = block_loops(body)
    first = labels[header]

    def block_is_rare(i):                                       # the straight-line block that starts at line i
        start = i
        while i < len(body) and not BRANCH.match(body[i]) and not (LABEL.match(body[i]) and i != start):
            if body[i] == "; rare":
                return True
            i += 1
        return False

    path, i = [], first
    for _ in range(100000):
        if (i != first or path) and (i == first or loops[i] != header):   # back at the header, or out of the loop
            break
        l = body[i]
        path.append(l)
        m = BRANCH.match(l)
        if m:
            t = labels[m.group(2)]
            leaves, exits = loops[i + 1] != header, loops[t] != header
            if m.group(1) == "branch" or (leaves and not exits) or (block_is_rare(i + 1) and not block_is_rare(t) and not exits):
                i = t
                continue
        i += 1
    return path


def main():
    for name, body in bodies(sys.argv[1]).items():
        if len(sys.argv) > 2 and sys.argv[2] not in name:
            continue
        header = main_loop(body)
        order = ("total", "mfma", "v_exp", "v_fma_mix", "v_cvt", "v_cmp/cndmask", "valu other", "lds", "vmem", "scratch", "salu", "s_nop", "s_waitcnt")
        for what, seg in (("static", in_loop_lines(body, header)), ("hot", hot_path(body, header) if "; rare" in body else None)):
            if seg is not None:
                c = classes(seg)
                print(f"{name[:64]:64s} {what:6s} " + "  ".join(f"{k} {c[k]}" for k in order if c[k]))


if __name__ == "__main__":
    main()
