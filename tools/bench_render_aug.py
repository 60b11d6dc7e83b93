#!/usr/bin/env python3
"""Augmented keypoint renderer line: fvp.heatmaps.render_keypoints(augment=)
(fvp_render_keypoints_aug: the painter with data_augmentation = True in one launch) at Shelf's
native geometry (shelf_native: V = 5, J = 17, 152 x 200, Cp = 32), with the plain render of the
same people in the same run (the method of tools/bench_render.py: HIP events over replays of a
captured chain of launches, three repeats so that the spread shows), the draw helper on the
host, and the numpy painter with augmentation that the launch replaces (tests/render_aug_ref.py,
the reference's loop: one exp patch per view, person and joint).  Prints one JSON line.

    python tools/bench_render_aug.py [--frames 8] [--people 4] [--steps 200] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "faster-voxelpose_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--people", type=int, default=4)
    ap.add_argument("--sigma", type=float, default=3.0)
    ap.add_argument("--steps", type=int, default=200, help="timed launches per figure")
    ap.add_argument("--chain", type=int, default=20, help="launches per captured graph")
    ap.add_argument("--repeats", type=int, default=3, help="repeats of each graphed figure (min, max reported)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import random

    import numpy as np
    import torch

    import render_aug_ref
    from bench_render import people
    from fvp import ops
    from fvp.heatmaps import Augmentation, draw_augmentation
    from fvp.workloads import WORKLOADS

    if not torch.cuda.is_available():
        raise SystemExit("bench_render_aug: no HIP device (nothing is measured on the host alone)")
    dev = torch.device("cuda:0")
    w = WORKLOADS["shelf_native"]
    B, P = args.frames, args.people
    (W, H), J = w.heatmap_size, w.num_joints
    joints_h = torch.from_numpy(people(w, B, P, 7))
    V = joints_h.shape[1]
    count_h = torch.full((B, V), P, dtype=torch.int32)
    kw = dict(image_size=w.image_size, heatmap_size=w.heatmap_size, sigma=args.sigma)

    # the draws, on the host, per frame as a dataset's __getitem__ makes them
    py_rng, np_rng = random.Random(7), np.random.RandomState(7)
    t0 = time.perf_counter()
    augs = [draw_augmentation(joints_h[b], count_h[b], py_rng=py_rng, np_rng=np_rng, **kw) for b in range(B)]
    draw_us = (time.perf_counter() - t0) * 1e6
    aug_h = Augmentation(torch.stack([a.scale for a in augs]), torch.stack([a.rect for a in augs]))

    def events(fn, steps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / steps  # us

    def graphed(fn):
        """us per call of fn, from replays of a captured chain of args.chain calls: one figure per repeat."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.chain):
                fn()
        return [events(g.replay, max(1, args.steps // args.chain)) / args.chain for _ in range(args.repeats)]

    joints, count = joints_h.to(dev), count_h.to(dev)
    scale, rect = aug_h.scale.to(dev), aug_h.rect.to(dev)
    img_w, img_h = w.image_size
    figures = {}
    outs = {}
    for half in (False, True):
        out = torch.empty((B, V, H, W, ops.render_cp(J)), dtype=torch.float16 if half else torch.float32, device=dev)
        tag = "f16" if half else "f32"
        plain = graphed(lambda: ops.render_keypoints_into(joints, count, None, img_w, img_h, args.sigma, out))
        aug = graphed(lambda: ops.render_keypoints_aug_into(joints, count, None, scale, rect, img_w, img_h,
                                                            args.sigma, out))
        plain_again = graphed(lambda: ops.render_keypoints_into(joints, count, None, img_w, img_h, args.sigma, out))
        ops.render_keypoints_aug_into(joints, count, None, scale, rect, img_w, img_h, args.sigma, out)
        torch.cuda.synchronize()
        outs[tag] = out
        both = plain + plain_again
        figures[tag] = {"plain_us": round(min(both), 2), "plain_us_max": round(max(both), 2),
                        "aug_us": round(min(aug), 2), "aug_us_max": round(max(aug), 2),
                        "aug_over_plain": round(min(aug) / min(both), 3),
                        "bytes_written": out.numel() * (2 if half else 4)}

    # the replaced path: the numpy painter with augmentation (then the planar copy and the layout pass,
    # which tools/bench_render.py times)
    jn, cn = joints_h.numpy(), count_h.numpy()
    t0 = time.perf_counter()
    planar_np = render_aug_ref.render(jn, cn, None, aug_h.scale.numpy(), aug_h.rect.numpy(), w.image_size,
                                      w.heatmap_size, args.sigma)
    painter_us = (time.perf_counter() - t0) * 1e6
    planar = torch.from_numpy(planar_np).to(dev)
    got = outs["f32"][..., :J].permute(0, 1, 4, 2, 3)
    max_err = float((got - planar).abs().max())
    same_support = bool(torch.equal(got != 0, planar != 0)) and not bool(outs["f32"][..., J:].any())
    half_equal = bool(torch.equal(outs["f16"], outs["f32"].half()))

    line = {
        "bench": "render_keypoints_aug", "workload": "shelf_native", "B": B, "V": V, "P": P, "J": J, "H": H, "W": W,
        "Cp": ops.render_cp(J), "sigma": args.sigma, "device": torch.cuda.get_device_name(0),
        "f32": figures["f32"], "f16": figures["f16"],
        "draw_augmentation_host_us": round(draw_us, 0), "draw_augmentation_host_us_per_frame": round(draw_us / B, 0),
        "records_bytes": scale.numel() * 4 + rect.numel() * 2,
        "replaced": {"numpy_painter_aug_us": round(painter_us, 0),
                     "numpy_painter_aug_us_per_frame": round(painter_us / B, 0)},
        "largest_scale": float(aug_h.scale.max()), "values_at_one": int((outs["f32"] == 1.0).sum()),
        "max_abs_err_vs_numpy": max_err, "same_support": same_support, "f16_equals_f32_half": half_equal,
        "timing": f"HIP events over replays of a {args.chain}-launch graph, {args.repeats} repeats (plain: "
                  f"{2 * args.repeats}, before and after the augmented one), min and max; host clock (draws, painter)",
    }
    s = json.dumps(line)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
