"""GPU: the pose tracker. ``pp_track_update`` and ``pp_track_affine_params`` against ``tracking.next_boxes_host`` / ``affine_params_host`` bit
for bit (crafted and seeded random cases, canaries around every output, inputs unchanged, a repeat launch identical), the closed loop of
``tracking.PoseTracker`` against ``apis.inference_topdown`` frame by frame, slot refill, and ``demo/video_demo.py --track``."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_cases as C  # noqa: E402

CFG_PROB = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_coco-256x192.py")
CFG_VITPOSE = os.path.join(ROOT, "configs", "td-hm_ViTPose-small_mi355x_coco-256x192.py")
DEV = "cuda:0"
GUARD = 8  # canary elements on either side of every output

pytestmark = pytest.mark.gpu


class _Guarded:
    """An output buffer between two canary zones."""

    def __init__(self, shape, dtype, fill):
        self.n = int(np.prod(shape))
        self.shape, self.fill = shape, fill
        self.buf = torch.full((self.n + 2 * GUARD,), fill, dtype=dtype, device=DEV)

    @property
    def ptr(self):
        return self.buf[GUARD:].data_ptr()

    def get(self):
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == self.fill).all() and (host[GUARD + self.n:] == self.fill).all(), "a canary was overwritten"
        return host[GUARD:GUARD + self.n].reshape(self.shape).copy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _device_update(c, size=C.INPUT, pad=1.25, in_place=False):
    """One launch of pp_track_update with the fused crop parameters; returns (boxes, alive, lost, centers, scales, maps)."""
    from probpose_code_amd import _lib, tracking

    n, K = c["records"].shape[:2]
    p = tracking.track_params(**c["params"])
    host_in = [np.ascontiguousarray(c["records"], np.float64), np.ascontiguousarray(c["centers"], np.float32), np.ascontiguousarray(c["scales"], np.float32),
               C.sigmas(K), np.ascontiguousarray(c["boxes"], np.float32), np.ascontiguousarray(c["alive"], np.int32), np.ascontiguousarray(c["lost"], np.int32)]
    dev_in = [torch.from_numpy(a.copy()).to(DEV) for a in host_in]
    if in_place:
        outs = None
        ob, oa, ol = dev_in[4].data_ptr(), dev_in[5].data_ptr(), dev_in[6].data_ptr()
    else:
        outs = [_Guarded((n, 4), torch.float32, -7.0), _Guarded((n,), torch.int32, -7), _Guarded((n,), torch.int32, -7)]
        ob, oa, ol = (o.ptr for o in outs)
    nxt = [_Guarded((n, 2), torch.float32, -7.0), _Guarded((n, 2), torch.float32, -7.0), _Guarded((n, 2, 3), torch.float64, -7.0)]
    _lib.call("pp_track_update", dev_in[0].data_ptr(), dev_in[1].data_ptr(), dev_in[2].data_ptr(), n, K, size[0], size[1],
              tracking.GATE_PROB if c["gate"] == "prob" else tracking.GATE_CONF, dev_in[3].data_ptr(), dev_in[4].data_ptr(), dev_in[5].data_ptr(),
              dev_in[6].data_ptr(), p["kpt_thr"], p["min_keypoints"], p["expand"], p["min_side"], p["smooth"], p["max_lost"], p["dup_oks_thr"],
              ob, oa, ol, pad, nxt[0].ptr, nxt[1].ptr, nxt[2].ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if in_place:
        state = [dev_in[4].cpu().numpy(), dev_in[5].cpu().numpy(), dev_in[6].cpu().numpy()]
        unchanged = range(4)
    else:
        state = [o.get() for o in outs]
        unchanged = range(7)
    for k in unchanged:
        assert np.array_equal(_bits(dev_in[k].cpu().numpy()), _bits(host_in[k])), f"input {k} was written"
    return state + [o.get() for o in nxt]


def _check_case(c, name):
    from probpose_code_amd import tracking

    wb, wa, wl, pairs = C.run_host(c, return_oks=True)
    thr = tracking.track_params(**c["params"])["dup_oks_thr"]
    for i, j, oks in pairs:  # the comparison must not hang on the last bits of exp()
        assert not np.isfinite(oks) or abs(oks - thr) > C.OKS_GUARD, (name, i, j, oks, thr)
    got = _device_update(c)
    assert np.array_equal(_bits(got[0]), _bits(wb)), (name, got[0], wb)
    assert np.array_equal(got[1], wa) and np.array_equal(got[2], wl), (name, got[1], wa, got[2], wl)
    with np.errstate(all="ignore"):
        wc, ws, wm = tracking.affine_params_host(wb, C.INPUT, 1.25)
    assert np.array_equal(_bits(got[3]), _bits(wc)) and np.array_equal(_bits(got[4]), _bits(ws)) and np.array_equal(_bits(got[5]), _bits(wm)), name
    again = _device_update(c)
    inplace = _device_update(c, in_place=True)
    for a, b, d in zip(got, again, inplace):
        assert np.array_equal(_bits(a), _bits(b)), f"{name}: a repeat launch differs"
        assert np.array_equal(_bits(a), _bits(d)), f"{name}: the in-place update differs"
    return got


@pytest.mark.parametrize("K", [17, 1])
def test_rule_kernel_on_the_crafted_cases(K):
    from probpose_code_amd import _lib

    _lib.reset_launch_counts()
    cases = C.crafted(K)
    for name, c in cases.items():
        _check_case(c, f"{name} K={K}")
    assert _lib.launch_count("track_update") == 3 * len(cases) and _lib.launch_count("pp_track.hip") == 3 * len(cases)


@pytest.mark.parametrize("n,K", [(1, 17), (2, 17), (5, 17), (64, 17), (1, 1), (2, 1), (5, 1), (64, 1), (7, 33), (3, 256)])
def test_rule_kernel_on_seeded_random_records(n, K):
    seen = np.zeros(4, int)  # updates, misses, deaths by max_lost, deaths as duplicates
    for seed in range(6):
        c = C.random_case(n, K, 100 * n + seed)
        b, a, l = _check_case(c, f"n={n} K={K} seed={seed}")[:3]
        was = c["alive"] != 0
        seen += [int((was & (l == 0)).sum()), int((was & (l > 0)).sum()), int((was & (a == 0) & (l > 0)).sum()), int((was & (a == 0) & (l == 0)).sum())]
    assert seen[0] > 0 and (n < 5 or K > 17 or (seen[1:] > 0).all()), f"branches not met: {seen}"  # (with many keypoints every track updates)


def test_entry_points_refuse_before_any_launch():
    from probpose_code_amd import _lib

    d = [torch.zeros(4096, dtype=torch.float64, device=DEV).data_ptr()] * 13
    s = torch.cuda.current_stream().cuda_stream
    _lib.reset_launch_counts()

    def update(n=3, ptrs=d):
        return _lib.lib.pp_track_update(ptrs[0], ptrs[1], ptrs[2], n, 17, 192, 256, 0, ptrs[3], ptrs[4], ptrs[5], ptrs[6], 0.3, 4, 1.25, 8.0, 0.0, 10, 0.9,
                                        ptrs[7], ptrs[8], ptrs[9], 1.25, ptrs[10], ptrs[11], ptrs[12], s)

    assert update(n=0) == _lib.PP_ERR_INVALID_ARG and update(n=65) == _lib.PP_ERR_INVALID_ARG
    for k in range(10):
        assert update(ptrs=[None if i == k else d[0] for i in range(13)]) == _lib.PP_ERR_INVALID_ARG, k
    assert update(ptrs=[None if i == 11 else d[0] for i in range(13)]) == _lib.PP_ERR_INVALID_ARG
    for n in (0, 65):
        assert _lib.lib.pp_track_affine_params(d[0], n, 192, 256, 1.25, d[0], d[0], d[0], s) == _lib.PP_ERR_INVALID_ARG
    for k in (0, 5, 6, 7):
        args = [d[0], 3, 192, 256, 1.25, d[0], d[0], d[0]]
        args[k] = None
        assert _lib.lib.pp_track_affine_params(*args, s) == _lib.PP_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert _lib.launch_count("pp_track.hip") == 0


@pytest.mark.parametrize("size,pad", [((192, 256), 1.25), ((288, 384), 1.25), ((192, 256), 1.1)])
def test_affine_kernel_equals_the_host_bit_for_bit(size, pad):
    from test_track_host import AFFINE_BOXES

    from probpose_code_amd import _lib, tracking
    from probpose_code_amd import transforms as T

    rng = np.random.default_rng(21)
    x0, y0 = rng.uniform(-200, 2000, 117), rng.uniform(-200, 1200, 117)
    boxes = np.concatenate([AFFINE_BOXES, np.stack([x0, y0, x0 + rng.uniform(0.5, 900, 117), y0 + rng.uniform(0.5, 900, 117)], -1).astype(np.float32)])
    tie = boxes[:64].copy()  # more boxes on the aspect-ratio tie w == (w / h) h, at sizes where the products are exact
    tie[:, 2] = tie[:, 0] + np.float32(size[0] / size[1]) * np.arange(1, 65, dtype=np.float32) * 4
    tie[:, 3] = tie[:, 1] + np.arange(1, 65, dtype=np.float32) * 4
    boxes = np.concatenate([boxes, tie])
    wc, ws, mats = T.topdown_affine_params(boxes, size, input_padding=pad)
    wm = np.stack([T.invert_affine(m) for m in mats])
    hc, hs, hm = tracking.affine_params_host(boxes, size, pad)
    assert np.array_equal(_bits(hc), _bits(wc)) and np.array_equal(_bits(hs), _bits(ws)) and np.array_equal(_bits(hm), _bits(wm))
    for lo in range(0, len(boxes), 64):
        part = boxes[lo:lo + 64]
        n = len(part)
        src = torch.from_numpy(part.copy()).to(DEV)
        outs = [_Guarded((n, 2), torch.float32, -7.0), _Guarded((n, 2), torch.float32, -7.0), _Guarded((n, 2, 3), torch.float64, -7.0)]
        for _ in range(2):
            _lib.call("pp_track_affine_params", src.data_ptr(), n, size[0], size[1], pad, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                      torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            gc, gs, gm = (o.get() for o in outs)
            assert np.array_equal(_bits(gc), _bits(wc[lo:lo + n])) and np.array_equal(_bits(gs), _bits(ws[lo:lo + n])), (size, pad, lo)
            assert np.array_equal(_bits(gm), _bits(wm[lo:lo + n])), (size, pad, lo)
        assert np.array_equal(src.cpu().numpy(), part)


# ------------------------------------------------------------------------------------------------------------------ the closed loop
H, W = 96, 128
FIRST_BOXES = np.array([[8, 6, 60, 80], [50, 10, 120, 90], [30, 20, 90, 70]], np.float32)


def _frames(count=6):
    """Seeded frames with structure: a gradient, noise and a bright block that moves 6 px per frame."""
    out = []
    for i in range(count):
        yy, xx = np.mgrid[0:H, 0:W]
        a = np.stack([(xx * 255) // (W - 1), (yy * 255) // (H - 1), ((xx + 3 * yy) * 2) % 256], axis=2) + np.random.default_rng(i).integers(-20, 21, (H, W, 3))
        a[30:60, 10 + 6 * i:40 + 6 * i] = (250, 240, 20)
        out.append(torch.from_numpy(np.clip(a, 0, 255).astype(np.uint8)).to(DEV))
    return out


def _model(cfg_path):
    from probpose_code_amd import apis, synthetic
    from probpose_code_amd.config import Config

    cfg = Config.fromfile(cfg_path)
    sd = synthetic.synthetic_state_dict(synthetic.arch_of(cfg), seed=0, logit_scale=2.0, head=synthetic.head_kind_of(cfg))
    return apis.init_model(cfg_path, dict(state_dict=sd), device=DEV)


@pytest.fixture(scope="module")
def prob_model():
    return _model(CFG_PROB)


def _gates(samples, gate):
    return np.stack([np.asarray(s.pred_instances.keypoints_probs if gate == "prob" else s.pred_instances.keypoints_conf
                                if "keypoints_conf" in s.pred_instances else s.pred_instances.keypoint_scores).reshape(-1) for s in samples])


def _threshold_between_the_tracks(model, frame, gate, min_keypoints=4):
    """A kpt_thr at which, in the first frame, one track updates and another misses: half way between the tracks' min_keypoints-th largest gates."""
    from probpose_code_amd import apis

    g = _gates(apis.inference_topdown(model, frame, FIRST_BOXES), gate)
    kth = np.sort(np.sort(g, axis=1)[:, -min_keypoints])
    assert kth[0] < kth[-1], f"the tracks' gates do not differ: {kth}"
    gaps = np.diff(kth)
    i = int(np.argmax(gaps))
    return float((kth[i] + kth[i + 1]) / 2)


def _same_sample(got, want, what):
    gp, wp = got.pred_instances, want.pred_instances
    keys = sorted(k for k, _ in wp.all_items())
    assert sorted(k for k, _ in gp.all_items()) == keys, what
    for k in keys:
        a, b = np.asarray(getattr(gp, k)), np.asarray(getattr(wp, k))
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a) if a.dtype.itemsize in (4, 8) else a, _bits(b) if b.dtype.itemsize in (4, 8) else b), (what, k)
    for k in ("input_center", "input_scale", "input_size", "ori_shape", "img_shape", "flip_indices", "dataset_name"):
        assert np.array_equal(np.asarray(got.metainfo[k]), np.asarray(want.metainfo[k])), (what, k)
    assert np.array_equal(got.gt_instances.bboxes, want.gt_instances.bboxes), what


def _run_loop(model, frames, thr, depth, graph_replay):
    from probpose_code_amd import tracking

    tr = tracking.PoseTracker(model, 3, depth=depth, graph_replay=graph_replay, kpt_thr=thr)
    assert tr.start(FIRST_BOXES) == [0, 1, 2]
    out, k = [], 0
    with torch.no_grad():
        for f in frames:
            while tr.in_flight >= depth:
                out.append((tr.result(), tr.frame_state))
            assert tr.submit(f) == k
            k += 1
        while tr.in_flight:
            out.append((tr.result(), tr.frame_state))
    return tr, out


def _check_closed_loop(model, gate):
    from probpose_code_amd import apis, tracking

    frames = _frames()
    thr = _threshold_between_the_tracks(model, frames[0], gate)
    tr, base = _run_loop(model, frames, thr, depth=2, graph_replay=True)
    assert tr.gate == gate and len(base) == len(frames)
    sig = C.sigmas(17)
    moved = missed = 0
    for t, (samples, st) in enumerate(base):
        assert st["index"] == t
        live = [s for s in range(3) if st["alive"][s]]
        assert [s.metainfo["track_id"] for s in samples] == live and [s.metainfo["track_slot"] for s in samples] == live
        if t == 0:
            assert np.array_equal(st["boxes"], FIRST_BOXES) and st["alive"].tolist() == [1, 1, 1] and st["lost"].tolist() == [0, 0, 0]
        # the delivered samples are inference_topdown's on the boxes reported for the frame
        want = apis.inference_topdown(model, frames[t], st["boxes"][live])
        assert len(want) == len(samples)
        for s, (g, w) in enumerate(zip(samples, want)):
            _same_sample(g, w, f"frame {t} track {live[s]}")
        # the records the rule read are those samples
        kp = tracking.image_space_keypoints(st["records"], st["centers"], st["scales"], tr.input_size)
        for g, s in zip(samples, live):
            assert np.array_equal(_bits(np.asarray(g.pred_instances.keypoints)[0]), _bits(kp[s]))
            assert np.array_equal(_gates([g], gate)[0], st["records"][s, :, 3 if gate == "prob" else 2].astype(np.float32))
        hc, hs, _ = tracking.affine_params_host(st["boxes"], tr.input_size, tr.input_padding)
        assert np.array_equal(_bits(hc), _bits(st["centers"])) and np.array_equal(_bits(hs), _bits(st["scales"]))
        if t + 1 < len(base):  # the boxes reported for frame t + 1 are next_boxes_host of frame t
            nb, na, nl, pairs = tracking.next_boxes_host(st["records"], st["centers"], st["scales"], tr.input_size, st["boxes"], st["alive"], st["lost"], sig,
                                                         gate=gate, return_oks=True, kpt_thr=thr)
            assert all(abs(o - 0.9) > C.OKS_GUARD for _, _, o in pairs)
            nst = base[t + 1][1]
            assert np.array_equal(_bits(nst["boxes"]), _bits(nb)) and np.array_equal(nst["alive"], na) and np.array_equal(nst["lost"], nl), t
            moved += int((nb != st["boxes"]).any(axis=1).sum())
            missed += int((nl > st["lost"]).sum())
    assert moved > 0 and missed > 0, f"nothing to see: {moved} box updates, {missed} misses"
    for depth, graph in ((1, True), (2, False), (1, False)):
        _, other = _run_loop(model, frames, thr, depth=depth, graph_replay=graph)
        for t, ((sa, sta), (sb, stb)) in enumerate(zip(base, other)):
            for k in ("records", "boxes", "centers", "scales", "maps", "alive", "lost", "track_ids"):
                assert np.array_equal(_bits(sta[k]) if sta[k].dtype.kind == "f" else sta[k], _bits(stb[k]) if stb[k].dtype.kind == "f" else stb[k]), (depth, graph, t, k)
            assert len(sa) == len(sb)
            for a, b in zip(sa, sb):
                _same_sample(b, a, f"depth {depth} graph {graph} frame {t}")


def test_closed_loop_probpose(prob_model):
    _check_closed_loop(prob_model, "prob")


def test_closed_loop_vitpose_uses_the_conf_gate():
    _check_closed_loop(_model(CFG_VITPOSE), "conf")


def test_generator_form_and_heatmaps(prob_model):
    """``apis.inference_topdown_track`` is the same loop; with ``test_cfg.output_heatmaps`` the samples carry ``pred_fields.heatmaps``, those of
    ``inference_topdown`` on the same boxes."""
    from probpose_code_amd import apis

    frames = _frames(3)
    thr = _threshold_between_the_tracks(prob_model, frames[0], "prob")
    got = list(apis.inference_topdown_track(prob_model, iter(frames), FIRST_BOXES, depth=2, kpt_thr=thr))
    _, base = _run_loop(prob_model, frames, thr, depth=2, graph_replay=True)
    assert len(got) == 3
    for a, (b, _) in zip(got, base):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same_sample(x, y, "generator")
    prob_model.test_cfg["output_heatmaps"] = True
    try:
        with_maps = list(apis.inference_topdown_track(prob_model, iter(frames), FIRST_BOXES, depth=2, kpt_thr=thr))
        for t, (a, (b, st)) in enumerate(zip(with_maps, base)):
            want = apis.inference_topdown(prob_model, frames[t], st["boxes"][[s.metainfo["track_slot"] for s in b]])
            for x, y, w in zip(a, b, want):
                _same_sample(x, y, "with heatmaps")
                assert torch.equal(x.pred_fields.heatmaps, w.pred_fields.heatmaps)
    finally:
        prob_model.test_cfg["output_heatmaps"] = False


def test_add_refills_a_dead_slot_with_a_fresh_track_id(prob_model):
    from probpose_code_amd import apis, tracking

    frames = _frames(4)
    tr = tracking.PoseTracker(prob_model, 2, depth=2, kpt_thr=2.0, max_lost=0)  # no gate reaches 2: every track misses, and dies at once
    assert tr.start(FIRST_BOXES[:1]) == [0] and tr.free_slots() == [1]
    with pytest.raises(RuntimeError, match="free slot"):
        tr.add(FIRST_BOXES)
    with torch.no_grad():
        tr.submit(frames[0])
        tr.submit(frames[1])
        with pytest.raises(RuntimeError, match="in flight"):
            tr.submit(frames[2])
        first = tr.result()
        assert [s.metainfo["track_id"] for s in first] == [0] and tr.frame_state["alive"].tolist() == [1, 0] and tr.free_slots() == [1]
        assert tr.result() == [] and tr.frame_state["alive"].tolist() == [0, 0] and tr.frame_state["lost"].tolist() == [1, 0]
        assert tr.free_slots() == [0, 1]
        assert tr.add(FIRST_BOXES[1:2]) == [1]  # slot 0 again, under a new id
        assert tr.free_slots() == [1]
        tr.submit(frames[2])
        got = tr.result()
        assert [(s.metainfo["track_id"], s.metainfo["track_slot"]) for s in got] == [(1, 0)]
        st = tr.frame_state
        assert np.array_equal(st["boxes"][0], FIRST_BOXES[1]) and st["alive"].tolist() == [1, 0] and st["lost"].tolist() == [0, 0]
        assert np.array_equal(got[0].pred_instances.bboxes[0], FIRST_BOXES[1])
        want = apis.inference_topdown(prob_model, frames[2], st["boxes"])  # (both slots: the batch the tracker ran)
        assert np.array_equal(_bits(np.asarray(got[0].pred_instances.keypoints)), _bits(np.asarray(want[0].pred_instances.keypoints)))
        assert tr.add(FIRST_BOXES[2:3]) == [2] and tr.free_slots() == []
        tr.submit(frames[3])
        assert [(s.metainfo["track_id"], s.metainfo["track_slot"]) for s in tr.result()] == [(2, 1)]  # track 1 died in frame 2


def test_refusals(prob_model):
    from probpose_code_amd import tracking

    with pytest.raises(ValueError, match="max_tracks"):
        tracking.PoseTracker(prob_model, 65)
    with pytest.raises(TypeError, match="unknown tracking parameter"):
        tracking.PoseTracker(prob_model, 2, threshold=1)
    affine = tracking._udp_affine_of(prob_model)[1]
    affine.use_udp = False
    try:
        with pytest.raises(NotImplementedError, match="use_udp=False"):
            tracking.PoseTracker(prob_model, 2)
    finally:
        affine.use_udp = True
    tr = tracking.PoseTracker(prob_model, 2)
    with pytest.raises(RuntimeError, match="before start"):
        tr.submit(_frames(1)[0])


def test_video_demo_track(tmp_path, prob_model):
    import io

    from PIL import Image

    from probpose_code_amd import apis, jpeg
    from probpose_code_amd.video import MjpegAviWriter, read_mjpeg_avi

    sys.path.insert(0, os.path.join(ROOT, "demo"))
    import video_demo

    src, dst, poses, plain = str(tmp_path / "in.avi"), str(tmp_path / "out.avi"), str(tmp_path / "poses.json"), str(tmp_path / "plain.json")
    with MjpegAviWriter(src, 12.5) as w:
        for f in _frames(4):
            b = io.BytesIO()
            Image.fromarray(f.flip(-1).cpu().numpy()).save(b, "JPEG", quality=90)
            w.write(b.getvalue())
    box = "10,4,80,60;40,20,120,90"
    done = video_demo.main([src, CFG_PROB, "synthetic", "--out-video", dst, "--out-file", poses, "--decode", "device", "--bboxes", box, "--device", DEV,
                            "--track", "--track-kpt-thr", "0.0", "--track-max-lost", "3", "--track-expand", "1.3", "--track-dup-thr", "0.95"])
    assert done["frames"] == 4
    out = read_mjpeg_avi(dst)
    assert (out.frame_count, out.width, out.height) == (4, W, H)
    for data in out:
        assert tuple(jpeg._host_decode(data).shape) == (H, W, 3)
    records = json.load(open(poses))
    assert len(records) == 4 and all(len(r) == 2 for r in records)
    assert [[p["track_id"] for p in r] for r in records] == [[0, 1]] * 4
    assert records[0][0]["bbox"] == [10, 4, 80, 60] and records[0][1]["bbox"] == [40, 20, 120, 90]
    assert all(records[t][0]["bbox"] != records[t + 1][0]["bbox"] for t in range(3)), "the boxes never moved"
    # the second frame's box is the rule's, from the first frame's pose
    img0 = jpeg.imread_device(next(iter(read_mjpeg_avi(src))), DEV)
    first = apis.inference_topdown(prob_model, img0, np.array([[10, 4, 80, 60], [40, 20, 120, 90]], np.float32))
    kp = np.asarray(first[0].pred_instances.keypoints)[0]
    lo, hi = kp.min(0), kp.max(0)
    side = np.maximum((hi - lo) * 1.3, 8.0)
    want = np.concatenate([(lo + hi) * 0.5 - 0.5 * side, (lo + hi) * 0.5 + 0.5 * side]).astype(np.float32)
    assert np.allclose(records[1][0]["bbox"], want, rtol=0, atol=1e-3)
    # without the flag nothing changed: the same boxes for every frame, no track_id
    video_demo.main([src, CFG_PROB, "synthetic", "--out-video", str(tmp_path / "plain.avi"), "--out-file", plain, "--decode", "device", "--bboxes", box, "--device", DEV])
    rp = json.load(open(plain))
    assert all("track_id" not in p for r in rp for p in r) and all(r[0]["bbox"] == [10, 4, 80, 60] for r in rp)
    assert np.allclose(rp[0][0]["keypoints"], records[0][0]["keypoints"])
