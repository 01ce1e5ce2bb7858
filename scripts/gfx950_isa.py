"""dev only: compile one kernel source of probpose_code_amd/csrc to gfx950 device assembly with the flags its Makefile gives it
(hipcc cross-compiles without a GPU). scripts/scratch_in_loops.py and scripts/loop_waitcnt.py read kernels through this module.
Run as a program it compares two source trees, the acceptance check of a change that must not move the generated code:
    python scripts/gfx950_isa.py OLD_TREE NEW_TREE          (each the root of a checkout; exit status 1 if any file differs)"""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = "/opt/rocm/bin/hipcc"
BASE_FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function"]
# per-source flags: keep in step with probpose_code_amd/csrc/Makefile
EXTRA_FLAGS = {
    "pp_mlp.hip": ["-fno-slp-vectorize"],
    "pp_ffn_split.hip": ["-fno-slp-vectorize"],
    "pp_ffn_dma.hip": ["-fno-slp-vectorize"],
    "pp_render.hip": ["-ffp-contract=off"],
    "pp_warp.hip": ["-ffp-contract=off"],
    "pp_render_batch.hip": ["-ffp-contract=off"],
    "pp_jpeg.hip": ["-fwrapv"],
}


def isa_text(src, extra=()):
    """The gfx950 assembly of one .hip, compiled from its own directory under its bare name, so that two checkouts of the same source
    give the same `.file` directives; `-cuid` fixes the compilation-unit id, which hipcc otherwise hashes from the absolute path (it
    names one marker symbol, `__hip_cuid_*`, and no code)."""
    src = os.path.abspath(src)
    name = os.path.basename(src)
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([HIPCC] + BASE_FLAGS + EXTRA_FLAGS.get(name, []) + list(extra) + ["-cuid=gfx950isa", "-c", name, "-o", os.path.join(td, "x.o"), "--save-temps=obj"],
                           cwd=os.path.dirname(src), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        if r.returncode:
            raise RuntimeError(f"{name} does not compile:\n{r.stderr[-4000:]}")
        asm = [f for f in os.listdir(td) if f.endswith("gfx950.s")][0]
        return open(os.path.join(td, asm)).read()


def functions(src, extra=()):
    """{mangled name: its instruction lines} of every function in the device assembly of src"""
    funcs, cur = {}, None
    for l in isa_text(src, extra).split("\n"):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = m.group(1); funcs[cur] = []
        elif l.startswith(".Lfunc_end"):
            cur = None
        elif cur:
            funcs[cur].append(l)
    return funcs


def loops(body):
    """(all, innermost) loops of one function as (first, last) line indices: a backward branch to a local label closes one"""
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", l)] if m}
    found = []
    for i, l in enumerate(body):
        m = re.search(r"s_cbranch_\w+ (\.LBB\d+_\d+)|s_branch (\.LBB\d+_\d+)", l)
        if m:
            t = m.group(1) or m.group(2)
            if t in labels and labels[t] < i:
                found.append((labels[t], i))
    inner = [(a, b) for a, b in found if not any(a2 >= a and b2 <= b and (a2, b2) != (a, b) for a2, b2 in found)]
    return found, inner


# The closed list of instructions whose two source operands compare() may reorder: IEEE addition, multiplication, maxNum and minNum give
# the same result for (a, b) and (b, a) - only which NaN payload survives when both are NaN depends on the order. `_e32`, and `_e64`
# without modifiers (neg / abs, clamp, omod, op_sel would bind to an operand position or follow the operands as further tokens).
COMMUTATIVE = re.compile(r"^(\s*v_(?:add|mul|max|min)_f32_e(?:32|64)\s+)([^,\s]+), ([^,\s]+), ([^,\s]+)$", re.M)
_PLAIN_OPERAND = re.compile(r"^(?:[vs]\d+|vcc_lo|vcc_hi|m0|exec_lo|exec_hi|-?\d+|0x[0-9a-f]+|-?\d*\.\d+)$")


def canonical_order(code):
    """code (comments stripped) with the two sources of every COMMUTATIVE instruction sorted; an operand that carries a modifier is left alone"""
    def one(m):
        a, b = m.group(3), m.group(4)
        if not (_PLAIN_OPERAND.match(a) and _PLAIN_OPERAND.match(b)):
            return m.group(0)
        a, b = sorted((a, b))
        return f"{m.group(1)}{m.group(2)}, {a}, {b}"
    return COMMUTATIVE.sub(one, code)


def compare(a, b):
    """The verdict on two assembly texts of one source file. Three of the four pass:
      identical;
      identical but for comments: the assembler's comments carry IR block labels (`; %.preheader194`, `; %_ZN2pp8gelu_erfEf.exit`), which
        are numbered and named by what was inlined; instructions, directives, kernel descriptors and metadata are outside comments;
      identical but for commutative operand order: as above once the two source operands of v_add_f32, v_mul_f32, v_max_f32 and v_min_f32
        are put in a canonical order. Code moved into an inlined helper reaches the instruction selector with the operands of such a node
        the other way round; IEEE results do not depend on the operand order (a NaN payload aside), so the arithmetic is the same. The
        list is closed - these four - and everything else must still match line for line."""
    if a == b:
        return "identical"
    code = lambda s: re.sub(r"[ \t]*;.*", "", s)
    a, b = code(a), code(b)
    if a == b:
        return "identical but for comments"
    return "identical but for commutative operand order" if canonical_order(a) == canonical_order(b) else "DIFFERS"


def main(old, new, jobs=8):
    csrc = os.path.join("probpose_code_amd", "csrc")
    names = sorted(f for f in os.listdir(os.path.join(new, csrc)) if f.endswith(".hip"))
    def one(f):
        if not os.path.exists(os.path.join(old, csrc, f)):
            return "new file"
        return compare(*(isa_text(os.path.join(t, csrc, f)) for t in (old, new)))
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        results = list(ex.map(one, names))
    for f, r in zip(names, results):
        print(f"{f:28s} {r}")
    return int(any(r == "DIFFERS" for r in results))


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
