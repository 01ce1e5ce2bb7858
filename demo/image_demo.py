"""Counterpart of the reference's ``demo/image_demo.py`` (:12-100): pose estimation of the people in one image - the whole
image as one box, or ``--bboxes x0,y0,x1,y1;...`` - printed / saved as JSON; ``--out-img`` also draws the result on the GPU
(probpose_code_amd.visualization), with ``--draw-heatmap`` the probability areas under it.

    python demo/image_demo.py IMG configs/td-pm_ProbPose-small_mi355x_coco-256x192.py CHECKPOINT --out-file out.json
    python demo/image_demo.py IMG CONFIG CHECKPOINT --draw-heatmap --out-img out.png
    python demo/image_demo.py IMG configs/td-hm_ViTPose-small_mi355x_coco-256x192.py CHECKPOINT --cfg-options model.head.decoder.type=UDPExpMaxHeatmap

CHECKPOINT may be "synthetic" (seeded random weights: plumbing check, BASELINE config 1)."""
import ast
import json
import os
import sys
from argparse import ArgumentParser

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_cfg_options(items):
    """``key=value`` pairs as tools/test.py reads them: Python literals where they parse as one, strings otherwise."""
    opts = {}
    for it in items or []:
        if "=" not in it:
            raise ValueError(f"--cfg-options takes key=value pairs, got {it!r}")
        k, v = it.split("=", 1)
        try:
            opts[k] = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            opts[k] = {"true": True, "false": False, "none": None}.get(v.lower(), v)
    return opts


def main():
    ap = ArgumentParser()
    ap.add_argument("img")
    ap.add_argument("config")
    ap.add_argument("checkpoint")
    ap.add_argument("--out-file", default=None)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--decode", default="host", choices=["host", "device"],
                    help="device: a JPEG file is Huffman-decoded on the host and reconstructed on the GPU (the same pixels)")
    ap.add_argument("--decode-entropy", default="host", choices=["host", "device"],
                    help="device (needs --decode device): the file's Huffman codes are decoded on the GPU as well (the same pixels)")
    ap.add_argument("--encode", default="host", choices=["host", "device"],
                    help="device: a .jpg / .jpeg --out-img is transformed on the GPU and Huffman-coded on the host (a file that decodes to the same pixels)")
    ap.add_argument("--jpeg-optimize", action="store_true",
                    help="with --encode device: Huffman tables built from the picture itself (Pillow's optimize=True): the same pixels, a smaller file")
    ap.add_argument("--restart-rows", type=int, default=0,
                    help="with --encode device: a restart marker every N MCU rows of the file (cjpeg -restart N; 0: none): the same pixels")
    ap.add_argument("--encode-png", default="host", choices=["host", "device"],
                    help="device: a .png --out-img is filtered, deflated and checksummed on the GPU (the same pixels, other bytes)")
    ap.add_argument("--png-match", default="runs", choices=["runs", "lz"],
                    help="with --encode-png device: runs (matches at distance 1 only) or lz (also one pixel and one row back: a smaller file)")
    ap.add_argument("--png-code", default="host", choices=["host", "device"],
                    help="with --encode-png device: where the Huffman codes are built - host (a round trip between the writer's halves) or "
                         "device (one launch more, the same file)")
    ap.add_argument("--bboxes", default=None, help="x0,y0,x1,y1;x0,y0,x1,y1;... (default: the whole image)")
    ap.add_argument("--precision", default=None, choices=[None, "f16x3", "bf16", "f32"],
                    help="overrides model.precision of the config (default there: f16x3, the mode within 1e-3 of the fp32 reference)")
    ap.add_argument("--cfg-options", nargs="+", default=None, metavar="KEY=VALUE",
                    help="override config keys as tools/test.py does, e.g. model.head.decoder.type=UDPExpMaxHeatmap (or ArgMaxProbMap)")
    ap.add_argument("--out-img", default=None, help="draw the predictions into this image file (PNG / JPEG by its extension)")
    ap.add_argument("--draw-heatmap", action="store_true", help="with --out-img: the probability areas of the keypoints under the poses")
    ap.add_argument("--kpt-thr", type=float, default=0.3, help="visibility threshold of the keypoints drawn")
    ap.add_argument("--radius", type=int, default=3, help="keypoint radius for visualization")
    ap.add_argument("--thickness", type=int, default=1, help="link thickness for visualization")
    ap.add_argument("--alpha", type=float, default=0.8, help="opacity of the keypoints")
    args = ap.parse_args()
    if args.draw_heatmap and not args.out_img:
        ap.error("--draw-heatmap draws into --out-img")
    if args.decode_entropy == "device" and args.decode != "device":
        ap.error("--decode-entropy device needs --decode device")
    if not 0 <= args.restart_rows <= 65535:
        ap.error("--restart-rows is in 0..65535")

    from probpose_code_amd import apis, synthetic
    from probpose_code_amd.structures import merge_data_samples

    ckpt = args.checkpoint
    if ckpt == "synthetic":  # (the backbone's arch and the head kind - ProbMapHead with its towers, or ViTPose's HeatmapHead - from the config)
        from probpose_code_amd.config import Config

        cfg = Config.fromfile(args.config)
        ckpt = dict(state_dict=synthetic.synthetic_state_dict(synthetic.arch_of(cfg), seed=0, logit_scale=2.0, head=synthetic.head_kind_of(cfg)))
    opts = parse_cfg_options(args.cfg_options) or None
    if args.precision:
        opts = dict(opts or {}, **{"model.precision": args.precision})
    if args.draw_heatmap:
        opts = dict(opts or {}, **{"model.test_cfg.output_heatmaps": True})
    model = apis.init_model(args.config, ckpt, device=args.device, cfg_options=opts)
    if args.decode == "device":
        apis.use_device_decode(model, entropy=args.decode_entropy)
    boxes = None
    if args.bboxes:
        boxes = np.array([[float(v) for v in b.split(",")] for b in args.bboxes.split(";")], np.float32)
    results = merge_data_samples(apis.inference_topdown(model, args.img, boxes))
    pi = results.pred_instances
    out = [dict(bbox=pi.bboxes[i].tolist(), keypoints=pi.keypoints[i].tolist(), keypoint_scores=pi.keypoint_scores[i].tolist(),
                keypoints_visible=pi.keypoints_visible[i].tolist(),
                **(dict(keypoints_probs=pi.keypoints_probs[i].tolist()) if "keypoints_probs" in pi else {}))  # (HeatmapHead gives no probabilities)
           for i in range(len(pi.keypoints))]
    text = json.dumps(out, indent=1)
    if args.out_file:
        open(args.out_file, "w").write(text)
    else:
        print(text)
    if args.out_img:
        from probpose_code_amd.apis import load_image_bgr
        from probpose_code_amd.visualization import PoseLocalVisualizer

        vis = PoseLocalVisualizer(radius=args.radius, line_width=args.thickness, alpha=args.alpha, device=args.device, image_encoder=args.encode,
                                  png_encoder=args.encode_png, png_match=args.png_match, jpeg_optimize=args.jpeg_optimize,
                                  png_code=args.png_code, jpeg_restart_rows=args.restart_rows)
        vis.set_dataset_meta(model.dataset_meta)
        vis.add_datasample("result", load_image_bgr(args.img)[:, :, ::-1], results, draw_heatmap=args.draw_heatmap, kpt_thr=args.kpt_thr,
                           out_file=args.out_img)


if __name__ == "__main__":
    main()
