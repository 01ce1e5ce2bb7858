"""dev only: per kernel of a source file, the s_waitcnt instructions (and barriers, scratch, MFMAs) inside its hottest loop (the
innermost loop with the most MFMAs) - a compiler-inserted `vmcnt(0)` in a stage loop drains the whole DMA ring.
    python scripts/loop_waitcnt.py probpose_code_amd/csrc/pp_winograd.hip [kernel-name-substring]"""
import collections, sys
import gfx950_isa
pat = sys.argv[2] if len(sys.argv) > 2 else ""
for name, body in gfx950_isa.functions(sys.argv[1]).items():
    if pat not in name: continue
    loops, inner = gfx950_isa.loops(body)
    if not loops: continue
    a, b = max(inner, key=lambda ab: sum("v_mfma" in x for x in body[ab[0]:ab[1]]))
    nm = sum("v_mfma" in x for x in body[a:b])
    if nm == 0: continue
    wc = collections.Counter(l.strip() for l in body[a:b] if "s_waitcnt" in l)
    print(f"{name[:90]}\n   hottest inner loop: {b - a} instructions, {nm} MFMAs, {sum('s_barrier' in x for x in body[a:b])} barriers, "
          f"{sum('scratch_' in x for x in body[a:b])} scratch, {sum('buffer_load' in x for x in body[a:b])} buffer loads, {sum('ds_read' in x for x in body[a:b])} ds_read")
    for k, v in wc.most_common(): print(f"      {v:3d} x {k}")
