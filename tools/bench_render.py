#!/usr/bin/env python3
"""Keypoint renderer line: fvp.heatmaps.render_keypoints (fvp_render_keypoints, one launch from
device keypoints to channels-last heatmaps) at Shelf's native geometry (shelf_native: V = 5,
J = 17, 152 x 200, Cp = 32), against the path it replaces -- the numpy painter on the host
(tests/render_ref.py, the reference's loop: one exp patch per view, person and joint), the
host-to-device copy of the planar tensor and the layout pass (to_channels_last) -- and against
the copy rate fvp_copy_f4 reaches in the same run (bench.py's "measured_copy_gbs": 1 GiB
each way, bytes read + written over time).  Prints one JSON line.

    python tools/bench_render.py [--frames 8] [--people 4] [--steps 200] [--out FILE]

The kernel time is taken from HIP events around replays of a captured graph of `--chain`
launches (a launch of tens of microseconds is otherwise timed together with its enqueue).
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


def people(w, B, P, seed):
    """[B, V, P, J, 2] fp64 image pixels: people 100 .. 300 px across, centred on the image."""
    import numpy as np

    rng = np.random.default_rng(seed)
    V, J = 5, w.num_joints
    centre = rng.uniform((0.15 * w.image_size[0], 0.2 * w.image_size[1]),
                         (0.85 * w.image_size[0], 0.8 * w.image_size[1]), size=(B, V, P, 1, 2))
    extent = rng.uniform(100.0, 300.0, size=(B, V, P, 1, 1)) * np.array([0.45, 1.0])
    return centre + rng.uniform(-0.5, 0.5, size=(B, V, P, J, 2)) * extent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--people", type=int, default=4)
    ap.add_argument("--sigma", type=float, default=3.0)
    ap.add_argument("--steps", type=int, default=200, help="timed launches per figure")
    ap.add_argument("--chain", type=int, default=20, help="launches per captured graph")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import render_ref
    from fvp import _lib, ops
    from fvp.heatmaps import render_keypoints, to_channels_last
    from fvp.workloads import WORKLOADS

    if not torch.cuda.is_available():
        raise SystemExit("bench_render: no HIP device (nothing is measured on the host alone)")
    dev = torch.device("cuda:0")
    w = WORKLOADS["shelf_native"]
    B, P = args.frames, args.people
    (W, H), J = w.heatmap_size, w.num_joints
    joints_h = torch.from_numpy(people(w, B, P, 7))
    V = joints_h.shape[1]
    count_h = torch.full((B, V), P, dtype=torch.int32)
    kw = dict(image_size=w.image_size, heatmap_size=w.heatmap_size, sigma=args.sigma)

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
        """us per call of fn, from replays of a captured chain of args.chain calls."""
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
        return events(g.replay, max(1, args.steps // args.chain)) / args.chain

    # the new path: keypoints to the device (a few KB), one launch
    for i in range(3 + 20):
        if i == 3:  # (the first copies initialise the device)
            t0 = time.perf_counter()
        joints, count = joints_h.to(dev), count_h.to(dev)
        torch.cuda.synchronize()
    kp_copy_us = (time.perf_counter() - t0) * 1e6 / 20
    cl = render_keypoints(joints, count, **kw)
    out = cl.t
    nbytes = out.numel() * 4
    img_w, img_h = w.image_size

    def launch():
        ops.render_keypoints_into(joints, count, None, img_w, img_h, args.sigma, out)

    render_us = graphed(launch)
    render_eager_us = events(lambda: render_keypoints(joints, count, **kw), args.steps)
    fill_us = graphed(lambda: out.zero_())  # a plain device fill of the same bytes
    launch()
    torch.cuda.synchronize()

    # the copy rate of this run (bench.py's definition)
    gib = 1 << 30
    src = torch.empty(gib // 4, dtype=torch.float32, device=dev).fill_(1.0)
    dst = torch.empty_like(src)
    cs = torch.cuda.current_stream(dev).cuda_stream
    copy_us = events(lambda: _lib.call("fvp_copy_f4", src.data_ptr(), dst.data_ptr(), gib, cs), 10)
    copy_gbs = 2 * gib / (copy_us * 1e-6) / 1e9
    del src, dst
    floor_us = nbytes / (copy_gbs * 1e9) * 1e6

    # the replaced path: numpy painter, planar host-to-device copy, layout pass
    jn, cn = joints_h.numpy(), count_h.numpy()
    t0 = time.perf_counter()
    planar_np = render_ref.render(jn, cn, None, w.image_size, w.heatmap_size, args.sigma)
    painter_us = (time.perf_counter() - t0) * 1e6
    planar_h = torch.from_numpy(planar_np)
    pinned = planar_h.pin_memory()

    def host_to_device(t):
        t.to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            t.to(dev, non_blocking=True)
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / 10

    h2d_pageable_us, h2d_pinned_us = host_to_device(planar_h), host_to_device(pinned)
    planar = planar_h.to(dev)
    layout_us = graphed(lambda: to_channels_last(planar))
    got = cl.t[..., :J].permute(0, 1, 4, 2, 3)
    max_err = float((got - planar).abs().max())
    same_support = bool(torch.equal(got != 0, planar != 0)) and not bool(cl.t[..., J:].any())

    replaced_us = painter_us + h2d_pinned_us + layout_us
    line = {
        "bench": "render_keypoints", "workload": "shelf_native", "B": B, "V": V, "P": P, "J": J, "H": H, "W": W,
        "Cp": cl.cp, "sigma": args.sigma, "device": torch.cuda.get_device_name(0),
        "bytes_written": nbytes,
        "render_us": round(render_us, 2), "render_eager_us": round(render_eager_us, 2),
        "render_gbs": round(nbytes / render_us / 1e3, 1),
        "copy_gbs": round(copy_gbs, 1), "floor_us": round(floor_us, 2),
        "frac_of_copy_rate": round(floor_us / render_us, 4),
        "device_fill_us": round(fill_us, 2),
        "keypoints_to_device_us": round(kp_copy_us, 1),
        "replaced": {"numpy_painter_us": round(painter_us, 0), "h2d_planar_pinned_us": round(h2d_pinned_us, 1),
                     "h2d_planar_pageable_us": round(h2d_pageable_us, 1), "to_channels_last_us": round(layout_us, 2),
                     "planar_bytes": planar_h.numel() * 4, "sum_us": round(replaced_us, 0)},
        "replaced_over_new": round(replaced_us / (render_eager_us + kp_copy_us), 1),
        "device_only_replaced_over_new": round((h2d_pinned_us + layout_us) / (render_us + kp_copy_us), 2),
        "max_abs_err_vs_numpy": max_err, "same_support": same_support,
        "timing": f"HIP events over replays of a {args.chain}-launch graph (render_us, to_channels_last_us, "
                  f"device_fill_us), over {args.steps} eager calls (render_eager_us), host clock around a "
                  f"synchronised copy (h2d, keypoints), host clock (painter)",
    }
    s = json.dumps(line)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
