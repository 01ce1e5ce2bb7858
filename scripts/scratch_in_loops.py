"""dev only: compile a kernel source to gfx950 ISA and list, per kernel with scratch memory, the scratch loads / stores that sit
INSIDE loops (a spilled register or an un-promoted local in a stage loop costs a memory round trip and an s_waitcnt per pass).
    python scripts/scratch_in_loops.py probpose_code_amd/csrc/pp_panel_split.hip [extra hipcc flags]"""
import sys
import gfx950_isa
for name, body in gfx950_isa.functions(sys.argv[1], sys.argv[2:]).items():
    scr = [i for i, l in enumerate(body) if "scratch_" in l]
    if not scr:
        continue
    loops, inner = gfx950_isa.loops(body)
    print(f"{name[:100]}: {len(scr)} scratch instructions")
    for a, b in sorted(set(loops)):
        ns = sum(a <= i <= b for i in scr)
        nm = sum("v_mfma" in x for x in body[a:b])
        if ns:
            print(f"    loop lines {a}-{b} ({'innermost' if (a, b) in inner else 'outer'}): {ns} scratch ops, {nm} MFMAs, {b - a} instructions")
