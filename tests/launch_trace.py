"""The launch trace of one eager ``ProbPoseEngine.forward``: every C-ABI call with its arguments, pointers as symbolic names.

What the engine does on the host is exactly the sequence of ``_lib.call`` invocations and what it hands them. ``trace_forward`` replaces
``probpose_code_amd._lib.call`` for one forward and records each call as ``name(arg, arg, ...)``: integers as they are, floats as the hex
of their float32 value, every pointer as ``<buffer name>+<byte offset>`` through a reverse map over the weights (``eng.w.t``), the
workspace (``ws:<key>``), the packed FFN / projection buffers, the decode tables, the padded final-conv weights, the flip-index tensor,
the host arrays ``mean`` / ``std``, the input and the two stream handles. A pointer that maps to nothing is an error.

``python tests/launch_trace.py --record`` writes ``tests/golden/launch_plans.json`` for ``CASES``. The file pins the launch plans of the
engine as it stood when this file was added (the plan still decided in `_workspace`, `backbone`, `heatmap_logits` / `towers` and `run_head`,
each on its own): it was recorded once, from that engine, and is never regenerated from later code - ``tests/test_launch_plan_gpu.py`` holds
every later engine to it entry for entry, so that the decision can move into one place without a launch changing.
"""
import ctypes
import json
import os
import struct
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "launch_plans.json")

ARCHS = {
    "S3": dict(embed_dims=384, num_layers=3, num_heads=12, feedforward_channels=1536),
    "B3": dict(embed_dims=768, num_layers=3, num_heads=12, feedforward_channels=3072),
    "L2": dict(embed_dims=1024, num_layers=2, num_heads=16, feedforward_channels=4096),
    "H2": dict(embed_dims=1280, num_layers=2, num_heads=16, feedforward_channels=5120),
}


def _case(name, arch="S3", precision="f16x3", B=2, plan=None, img_size=(256, 192), head="probmap", decode=None, return_heatmaps=False,
          shift_heatmap=False, flip_test=True, warns=False):
    return dict(name=name, arch=arch, precision=precision, B=B, plan=plan, img_size=img_size, head=head, decode=decode,
                return_heatmaps=return_heatmaps, shift_heatmap=shift_heatmap, flip_test=flip_test, warns=warns)


_BF16_SWITCHES = ("fuse_attn", "fuse_qkv", "fuse_proj", "fuse_mlp", "split_k", "fuse_head", "fuse_pool", "fuse_resln")

CASES = [
    # f16x3, ViT-S width: the small plan, the boundary to the row-owner plan (6 528 / 6 912 rows around SMALL_PLAN_ROWS_BELOW), one switch at a time
    _case("s3_b1", B=1),
    _case("s3_b4", B=4),
    _case("s3_b17", B=17),
    _case("s3_b18", B=18),
    _case("s3_b18_no_ln_fold", B=18, plan=dict(ln_fold=False)),
    _case("s3_b18_no_fuse_qkv_attn", B=18, plan=dict(fuse_qkv_attn=False)),
    _case("s3_b18_no_fuse_proj", B=18, plan=dict(fuse_proj=False)),
    _case("s3_b18_no_fuse_mlp", B=18, plan=dict(fuse_mlp=False)),
    _case("s3_b18_no_winograd", B=18, plan=dict(winograd=False)),
    _case("s3_b18_no_fuse_pool_no_winograd", B=18, plan=dict(fuse_pool=False, winograd=False)),
    _case("s3_b18_no_split_k", B=18, plan=dict(split_k=False)),
    _case("s3_b18_no_fuse_head", B=18, plan=dict(fuse_head=False)),
    _case("s3_b1_one_stream", B=1, plan=dict(head_two_streams=False)),
    _case("s3_b1_no_small_plan", B=1, plan=dict(small_plan=False)),
    _case("s3_384x288_b2_no_small_plan", B=2, plan=dict(small_plan=False), img_size=(384, 288), warns=True),
    # f16x3, ViT-B width: LayerNorm folded into the Linear layers / generic / small
    _case("b3_b18", arch="B3", B=18),  # (the first row-owner batch: still generic, 6 912 rows are 144 tiles of the twelve-wave Linear kernel)
    _case("b3_b64", arch="B3", B=64),  # 24 576 rows: 512 tiles for the narrowest layer, the first batch at which _ln_fold_at holds
    _case("b3_b2_no_small_plan", arch="B3", B=2, plan=dict(small_plan=False)),
    _case("b3_b2", arch="B3", B=2),
    _case("b3_b2_no_small_plan_resln", arch="B3", B=2, plan=dict(small_plan=False, fuse_resln=True)),
    _case("l2_b1", arch="L2", B=1),
    _case("h2_b1", arch="H2", B=1),
    # bf16: one launch per layer, and each switch off
    _case("bf16_s3_b8", precision="bf16", B=8),
    *[_case(f"bf16_s3_b8_no_{k}", precision="bf16", B=8, plan={k: False}) for k in _BF16_SWITCHES],
    _case("f32_s3_b2", precision="f32", B=2),
    # heads and decoders
    _case("s3_b2_heatmap", head="heatmap"),
    _case("s3_b2_heatmap_expmax", head="heatmap", decode="expmax"),
    _case("s3_b2_probmap_dark", decode="dark"),
    _case("s3_b2_return_heatmaps", return_heatmaps=True),
    _case("s3_b2_shift_heatmap", shift_heatmap=True),
    _case("s3_b2_no_flip", flip_test=False),
]

_state_dicts = {}


def build_engine(case):
    """The engine of a case (synthetic weights, reduced depth) and whether its construction warned about the 192-token kernel."""
    from probpose_code_amd import ProbPoseEngine
    from probpose_code_amd import synthetic as S

    key = (case["arch"], tuple(case["img_size"]), case["head"])
    if key not in _state_dicts:
        _state_dicts[key] = S.synthetic_state_dict(ARCHS[case["arch"]], img_size=tuple(case["img_size"]), seed=0, head=case["head"])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        eng = ProbPoseEngine(_state_dicts[key], ARCHS[case["arch"]]["num_heads"], img_size=tuple(case["img_size"]), precision=case["precision"],
                             device="cuda:0", plan=case["plan"], decode=case["decode"])
    warned = any(issubclass(c.category, RuntimeWarning) and "miss the fused qkv + attention kernel" in str(c.message) for c in caught)
    return eng, warned


def case_inputs(case):
    from probpose_code_amd import synthetic as S

    imgs = S.synthetic_crops(case["B"], img_size=tuple(case["img_size"]), seed=1).cuda()
    return imgs, (S.COCO_FLIP_INDICES if case["flip_test"] else None)


class _PointerMap:
    """address -> "<name>+<offset>" over everything the engine may legitimately hand to a kernel."""

    def __init__(self):
        self.ranges = []  # (start, end, name)

    def add(self, name, start, nbytes):
        if start and nbytes > 0:
            self.ranges.append((int(start), int(start) + int(nbytes), name))

    def add_tensor(self, name, t):
        if t is not None:
            self.add(name, t.data_ptr(), t.numel() * t.element_size())

    def name(self, p):
        # the innermost buffer that holds p (weights may be views of one another); ties by name, so that the answer does not depend on dict order
        hits = sorted((e - s, n, p - s) for s, e, n in self.ranges if s <= p < e)
        if not hits:
            raise AssertionError(f"pointer {p:#x} handed to a kernel maps to no weight, workspace buffer or input")
        return f"{hits[0][1]}+{hits[0][2]}"


def _pointer_map(eng, ws, imgs, flip_indices):
    m = _PointerMap()
    for k, t in eng.w.t.items():
        m.add_tensor(k, t)
    for k, t in ws.items():
        m.add_tensor("ws:" + k, t)
    for i, t in eng._ffn_packed.items():
        m.add_tensor(f"packed:ffn:{i}", t)
    for i, t in eng._proj_packed.items():
        m.add_tensor(f"packed:proj:{i}", t)
    m.add_tensor("taps", getattr(eng, "taps", None))
    m.add_tensor("radius", getattr(eng, "radius", None))
    if eng._final_padded is not None:
        m.add_tensor("_final_padded.w", eng._final_padded[0])
        m.add_tensor("_final_padded.b", eng._final_padded[1])
    if flip_indices is not None:
        m.add_tensor("flip_indices", eng._flip_indices(flip_indices))
    m.add("mean", eng.mean.ctypes.data, eng.mean.nbytes)
    m.add("std", eng.std.ctypes.data, eng.std.nbytes)
    m.add_tensor("input", imgs)
    return m


def _f32hex(v):
    return struct.pack(">f", float(v)).hex()


def trace_forward(eng, imgs, case, flip_indices):
    """-> (list of "fn(args)" strings of one eager forward, the forward's result). Runs on a stream of its own, so that the launch stream's
    handle is never NULL and the head's second stream is told from it."""
    import torch

    from probpose_code_amd import _lib

    passes = 2 if case["flip_test"] else 1
    ws = eng._workspace(imgs.shape[0], passes, 0)
    pm = _pointer_map(eng, ws, imgs, flip_indices)
    main = torch.cuda.Stream(device=eng.device)
    handle = main.cuda_stream
    assert handle
    calls, real_call, sides = [], _lib.call, set()

    def record(fn, *args):
        argtypes = _lib.SIGNATURES[fn][1]
        assert len(argtypes) == len(args), (fn, len(argtypes), len(args))
        out = []
        for k, (a, ty) in enumerate(zip(args, argtypes)):
            if ty is ctypes.c_void_p:
                if k == len(args) - 1:  # every launch's last argument: the stream
                    if a != handle:
                        sides.add(a)
                    out.append("stream" if a == handle else "side")
                else:
                    out.append("null" if a is None else pm.name(int(a)))
            elif ty in (ctypes.c_float, ctypes.c_double):
                out.append("f:" + _f32hex(a))
            else:
                assert isinstance(a, (int, bool)), (fn, k, a)
                out.append(str(int(a)))
        calls.append(f"{fn}({', '.join(out)})")
        return real_call(fn, *args)

    torch.cuda.synchronize(eng.device)
    _lib.call = record
    try:
        with torch.cuda.stream(main):
            res = eng.forward(imgs, case["flip_test"], flip_indices, case["return_heatmaps"], shift_heatmap=case["shift_heatmap"])
    finally:
        _lib.call = real_call
    torch.cuda.synchronize(eng.device)
    assert len(sides) <= 1 and None not in sides and 0 not in sides, f"launches on more than one stream beside the main one: {sides}"
    return calls, res


def run_case(case):
    """One case end to end -> the record the golden file keeps for it."""
    eng, warned = build_engine(case)
    imgs, flip = case_inputs(case)
    calls, _ = trace_forward(eng, imgs, case, flip)
    ws = eng._workspace(case["B"], 2 if case["flip_test"] else 1, 0)
    return dict(layer_plan=eng.layer_plan, warned=warned, logits_phased=bool(eng._logits_phased),
                ws_keys=sorted(k for k, v in ws.items() if v is not None), trace=calls)


def main():
    if sys.argv[1:] != ["--record"]:
        raise SystemExit("usage: python tests/launch_trace.py --record   (on the commit whose plans are to be pinned, on the GPU)")
    out = {}
    for case in CASES:
        out[case["name"]] = run_case(case)
        print(f"{case['name']}: {len(out[case['name']]['trace'])} calls", flush=True)
    with open(GOLDEN_FILE, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN_FILE}")


if __name__ == "__main__":
    main()
