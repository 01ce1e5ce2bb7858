"""GPU: demo/video_demo.py end to end on a three-frame Motion-JPEG AVI made here - decoded on the device, drawn, Huffman-coded
on the device, written - against the same steps taken one frame at a time with the host coder; and
``PoseLocalVisualizer.draw_datasample`` against ``add_datasample``."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "td-pm_ProbPose-small_mi355x_coco-256x192.py")
DEV = "cuda:0"
BOX = "10,4,80,60"
QUALITY = 80

pytestmark = pytest.mark.gpu


def _input_frames():
    """Three 96 x 64 JPEG files with structure (a gradient, a moving square, noise)."""
    from PIL import Image

    out = []
    for i in range(3):
        yy, xx = np.mgrid[0:64, 0:96]
        a = np.stack([(xx * 255) // 95, (yy * 255) // 63, ((xx + 3 * yy) * 2) % 256], axis=2) + np.random.default_rng(i).integers(-12, 13, (64, 96, 3))
        a[20:40, 10 + 20 * i:30 + 20 * i] = (250, 240, 20)
        b = io.BytesIO()
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(b, "JPEG", quality=90)
        out.append(b.getvalue())
    return out


@pytest.fixture(scope="module")
def model():
    from probpose_code_amd import apis, synthetic

    return apis.init_model(CFG, dict(state_dict=synthetic.synthetic_state_dict("small", seed=0, logit_scale=2.0)), device=DEV)


def test_video_demo_writes_the_frames_the_host_coder_writes(tmp_path, model):
    from probpose_code_amd import apis, jpeg
    from probpose_code_amd.structures import merge_data_samples
    from probpose_code_amd.video import MjpegAviWriter, read_mjpeg_avi
    from probpose_code_amd.visualization import PoseLocalVisualizer

    sys.path.insert(0, os.path.join(ROOT, "demo"))
    import video_demo

    frames = _input_frames()
    src, dst, poses = str(tmp_path / "in.avi"), str(tmp_path / "out.avi"), str(tmp_path / "poses.json")
    with MjpegAviWriter(src, 12.5) as w:
        for f in frames:
            w.write(f)
    calls = jpeg.entropy_device_calls
    done = video_demo.main([src, CFG, "synthetic", "--out-video", dst, "--out-file", poses, "--decode", "device", "--entropy", "device", "--bboxes", BOX,
                         "--quality", str(QUALITY), "--encode-batch", "2", "--device", DEV])
    assert done["frames"] == 3 and jpeg.entropy_device_calls == calls + 2, "three frames, encoded two and one at a time"
    out = read_mjpeg_avi(dst)
    assert (out.frame_count, out.width, out.height, out.fps) == (3, 96, 64, 12.5)
    got = list(out)
    assert len(got) == 3
    records = json.load(open(poses))
    assert len(records) == 3 and all(len(r) == 1 and len(r[0]["keypoints"]) == 17 for r in records)
    vis = PoseLocalVisualizer(radius=3, line_width=1, alpha=0.8, device=DEV)
    vis.set_dataset_meta(model.dataset_meta)
    box = np.array([[float(v) for v in BOX.split(",")]], np.float32)
    for i, f in enumerate(frames):
        img = jpeg.imread_device(f, DEV)
        merged = merge_data_samples(apis.inference_topdown(model, img, box))
        drawn = vis.draw_datasample(img.flip(-1), merged)
        assert drawn.is_cuda and tuple(drawn.shape) == (64, 96, 3)
        (want,) = jpeg.encode_batch([drawn], quality=QUALITY, subsampling="4:2:0", channel_order="rgb", entropy="host")
        assert got[i] == want, f"frame {i}: {len(got[i])} bytes against {len(want)}"
        assert np.allclose(records[i][0]["keypoints"], merged.pred_instances.keypoints[0].tolist())
    assert not np.array_equal(drawn.cpu().numpy(), img.flip(-1).cpu().numpy()), "nothing was drawn"


def test_draw_datasample_equals_add_datasample(model):
    from probpose_code_amd import apis, jpeg
    from probpose_code_amd.structures import merge_data_samples
    from probpose_code_amd.visualization import PoseLocalVisualizer

    img = jpeg.imread_device(_input_frames()[1], DEV)
    rgb = img.flip(-1)
    merged = merge_data_samples(apis.inference_topdown(model, img, np.array([[10, 4, 80, 60], [30, 0, 96, 64]], np.float32)))
    vis = PoseLocalVisualizer(radius=3, line_width=1, alpha=0.8, device=DEV)
    vis.set_dataset_meta(model.dataset_meta)
    for kw in (dict(), dict(draw_bbox=False), dict(kpt_thr=0.0)):
        drawn = vis.draw_datasample(rgb, merged, **kw)
        assert isinstance(drawn, torch.Tensor) and drawn.is_cuda and drawn.dtype == torch.uint8
        added = vis.add_datasample("x", rgb.cpu().numpy(), merged, **kw)
        assert isinstance(added, np.ndarray) and np.array_equal(drawn.cpu().numpy(), added), kw
