"""The video loop of the reference's ``demo/topdown_demo_with_mmdet.py`` (:280-310) without a detector: pose estimation of
every frame of a Motion-JPEG AVI file (or of a directory of ``.jpg`` files in sorted order), drawn on the GPU and written as
a Motion-JPEG AVI - no cv2, no frame ever stored as pixels on the host with ``--decode device --entropy device``.

    python demo/video_demo.py IN.avi configs/td-pm_ProbPose-small_mi355x_coco-256x192.py CHECKPOINT --out-video OUT.avi
    python demo/video_demo.py FRAMES_DIR CONFIG CHECKPOINT --out-video OUT.avi --decode device --entropy device --out-file poses.json

Frames go through ``apis.inference_topdown_stream`` (``--depth`` frames in flight), are drawn with
``PoseLocalVisualizer.draw_datasample`` (the frame stays a device tensor) and encoded ``--encode-batch`` at a time with
``jpeg.encode_batch``. The box of every frame is the whole image, or ``--bboxes x0,y0,x1,y1;...`` for all frames.
With ``--track`` the boxes follow the persons instead: ``--bboxes`` (default: the whole image) are the FIRST frame's boxes, every later frame
is cropped with the boxes the device derived from the poses of the frame before it (``apis.inference_topdown_track``,
``probpose_code_amd/tracking.py``; the defaults of its rule are not validated on real footage), and the ``--out-file`` records gain ``track_id``.
CHECKPOINT may be "synthetic" (seeded random weights: plumbing check)."""
import json
import os
import sys
import time
from argparse import ArgumentParser
from collections import deque

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def frame_source(path):
    """(iterable of JPEG bytes, fps or None) of an MJPEG AVI file or a directory of .jpg / .jpeg files."""
    if os.path.isdir(path):
        names = sorted(n for n in os.listdir(path) if n.lower().endswith((".jpg", ".jpeg")))
        if not names:
            raise ValueError(f"{path}: no .jpg files")

        def read():
            for n in names:
                with open(os.path.join(path, n), "rb") as f:
                    yield f.read()

        return read(), None
    from probpose_code_amd.video import read_mjpeg_avi

    avi = read_mjpeg_avi(path)
    return iter(avi), avi.fps


def main(argv=None):
    from image_demo import parse_cfg_options

    ap = ArgumentParser()
    ap.add_argument("input", help="an MJPEG AVI file or a directory of .jpg files")
    ap.add_argument("config")
    ap.add_argument("checkpoint")
    ap.add_argument("--out-video", required=True, help="the Motion-JPEG AVI file the drawn frames go to")
    ap.add_argument("--out-file", default=None, help="the poses as JSON: one record per frame")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--decode", default="host", choices=["host", "device"],
                    help="device: a frame is Huffman-decoded on the host and reconstructed on the GPU (the same pixels)")
    ap.add_argument("--decode-entropy", default="host", choices=["host", "device"],
                    help="device (needs --decode device): a frame's Huffman codes are decoded on the GPU as well (the same pixels)")
    ap.add_argument("--entropy", default="host", choices=["host", "device"],
                    help="device: the drawn frames are Huffman-coded on the GPU as well (the same files)")
    ap.add_argument("--jpeg-optimize", action="store_true",
                    help="every frame gets Huffman tables built from its own statistics (with --entropy device: built on the GPU): the same pixels, smaller frames")
    ap.add_argument("--restart-rows", type=int, default=0,
                    help="a restart marker every N MCU rows of the written frames (cjpeg -restart N; 0: none), with --entropy host or device: the same files")
    ap.add_argument("--quality", type=int, default=75, help="JPEG quality of the written frames, 1..100")
    ap.add_argument("--fps", type=float, default=None, help="frame rate of the output (default: the input's, 25 for a directory)")
    ap.add_argument("--workers", type=int, default=8, help="host threads of the Huffman coder with --entropy host")
    ap.add_argument("--depth", type=int, default=2, help="frames in flight on the device")
    ap.add_argument("--encode-batch", type=int, default=8, help="drawn frames encoded per jpeg.encode_batch call")
    ap.add_argument("--bboxes", default=None, help="x0,y0,x1,y1;x0,y0,x1,y1;... for every frame (default: the whole image)")
    ap.add_argument("--track", action="store_true",
                    help="--bboxes are the first frame's boxes; later frames are cropped with boxes derived on the GPU from the frame before")
    ap.add_argument("--track-kpt-thr", type=float, default=None, help="with --track: a keypoint counts for the next box from this presence probability on (0.3)")
    ap.add_argument("--track-expand", type=float, default=None, help="with --track: the keypoints' box is grown by this factor (1.25)")
    ap.add_argument("--track-max-lost", type=int, default=None, help="with --track: a track dies after more than this many frames without a box update (10)")
    ap.add_argument("--track-dup-thr", type=float, default=None, help="with --track: two tracks whose poses have an OKS above this are one person (0.9)")
    ap.add_argument("--precision", default=None, choices=[None, "f16x3", "bf16", "f32"], help="overrides model.precision of the config")
    ap.add_argument("--cfg-options", nargs="+", default=None, metavar="KEY=VALUE", help="override config keys as tools/test.py does")
    ap.add_argument("--draw-heatmap", action="store_true", help="the probability areas of the keypoints under the poses")
    ap.add_argument("--kpt-thr", type=float, default=0.3, help="visibility threshold of the keypoints drawn")
    ap.add_argument("--radius", type=int, default=3, help="keypoint radius for visualization")
    ap.add_argument("--thickness", type=int, default=1, help="link thickness for visualization")
    ap.add_argument("--alpha", type=float, default=0.8, help="opacity of the keypoints")
    args = ap.parse_args(argv)

    from probpose_code_amd import apis, jpeg, synthetic
    from probpose_code_amd.runner import MAX_WORKERS
    from probpose_code_amd.structures import merge_data_samples
    from probpose_code_amd.video import MjpegAviWriter
    from probpose_code_amd.visualization import PoseLocalVisualizer

    if not 1 <= args.workers <= MAX_WORKERS:
        ap.error(f"--workers must be in 1..{MAX_WORKERS}")
    if args.decode_entropy == "device" and args.decode != "device":
        ap.error("--decode-entropy device needs --decode device")
    if args.depth < 1 or args.encode_batch < 1 or not 1 <= args.quality <= 100:
        ap.error("--depth and --encode-batch are at least 1, --quality is in 1..100")
    if not 0 <= args.restart_rows <= 65535:
        ap.error("--restart-rows is in 0..65535")
    frames, fps = frame_source(args.input)
    fps = args.fps if args.fps is not None else (fps or 25.0)

    ckpt = args.checkpoint
    if ckpt == "synthetic":
        from probpose_code_amd.config import Config

        cfg = Config.fromfile(args.config)
        ckpt = dict(state_dict=synthetic.synthetic_state_dict(synthetic.arch_of(cfg), seed=0, logit_scale=2.0, head=synthetic.head_kind_of(cfg)))
    opts = parse_cfg_options(args.cfg_options) or None
    if args.precision:
        opts = dict(opts or {}, **{"model.precision": args.precision})
    if args.draw_heatmap:
        opts = dict(opts or {}, **{"model.test_cfg.output_heatmaps": True})
    model = apis.init_model(args.config, ckpt, device=args.device, cfg_options=opts)
    boxes = None
    if args.bboxes:
        boxes = np.array([[float(v) for v in b.split(",")] for b in args.bboxes.split(";")], np.float32)
    vis = PoseLocalVisualizer(radius=args.radius, line_width=args.thickness, alpha=args.alpha, device=args.device)
    vis.set_dataset_meta(model.dataset_meta)

    shown = deque()  # the decoded frames whose poses are still on their way, oldest first

    def decoded():
        for data in frames:
            img = jpeg.imread_device(data, args.device, entropy=args.decode_entropy) if args.decode == "device" else jpeg._host_decode(data)  # (H, W, 3) BGR
            shown.append(img)
            yield img, boxes

    def tracked():
        """--track: the first frame's boxes are --bboxes (or the whole image), the tracker makes the others."""
        it = decoded()
        try:
            first = next(it)[0]
        except StopIteration:
            return
        first_boxes = boxes if boxes is not None else np.array([[0, 0, first.shape[1], first.shape[0]]], np.float32)
        params = {k: v for k, v in dict(kpt_thr=args.track_kpt_thr, expand=args.track_expand, max_lost=args.track_max_lost,
                                        dup_oks_thr=args.track_dup_thr).items() if v is not None}

        def images():
            yield first
            for img, _ in it:
                yield img

        yield from apis.inference_topdown_track(model, images(), first_boxes, depth=args.depth, **params)

    records, pending, written = [], [], 0
    t0 = time.perf_counter()
    with MjpegAviWriter(args.out_video, fps) as out:

        def flush():
            nonlocal written
            for data in jpeg.encode_batch(pending, quality=args.quality, subsampling="4:2:0", channel_order="rgb", workers=args.workers,
                                          device=args.device, entropy=args.entropy, optimize=args.jpeg_optimize, restart_rows=args.restart_rows):
                out.write(data)
                written += 1
            pending.clear()

        for samples in (tracked() if args.track else apis.inference_topdown_stream(model, decoded(), depth=args.depth)):
            img = shown.popleft()
            rgb = img.flip(-1) if hasattr(img, "flip") else img[:, :, ::-1]
            if not samples:  # --track: every track has died - the frame is written as it came
                import torch

                pending.append(rgb.contiguous() if hasattr(rgb, "contiguous") else torch.from_numpy(np.ascontiguousarray(rgb)).to(args.device))
                records.append([])
                if len(pending) >= args.encode_batch:
                    flush()
                continue
            merged = merge_data_samples(samples)
            pending.append(vis.draw_datasample(rgb, merged, draw_heatmap=args.draw_heatmap, kpt_thr=args.kpt_thr))
            if len(pending) >= args.encode_batch:
                flush()
            if args.out_file:
                pi = merged.pred_instances
                records.append([dict(bbox=pi.bboxes[i].tolist(), keypoints=pi.keypoints[i].tolist(), keypoint_scores=pi.keypoint_scores[i].tolist(),
                                     keypoints_visible=pi.keypoints_visible[i].tolist(),
                                     **(dict(keypoints_probs=pi.keypoints_probs[i].tolist()) if "keypoints_probs" in pi else {}),
                                     **(dict(track_id=int(samples[i].metainfo["track_id"])) if args.track else {}))
                                for i in range(len(pi.keypoints))])
        if pending:
            flush()
    seconds = time.perf_counter() - t0  # first frame read to last frame written (the writer closed)
    if args.out_file:
        with open(args.out_file, "w") as f:
            json.dump(records, f, indent=1)
    print(f"{written} frames -> {args.out_video} in {seconds:.3f} s ({written / max(seconds, 1e-9):.1f} frames/s)")
    return dict(frames=written, seconds=seconds)


if __name__ == "__main__":
    main()
