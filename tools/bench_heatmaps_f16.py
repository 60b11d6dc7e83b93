#!/usr/bin/env python3
"""fp16 channels-last heatmaps written at their source against the route that existed
before (the fp32 producer, then the cast pass), same process, same inputs.

Three comparisons, each `cast` (fp32 producer + ChannelsLastHeatmaps.half()) against
`direct` (the producer writes fp16 itself), both ending in the same fp16 tensor (checked
bit for bit for the renderer; the head differs by its summation order, inside the fp16
rounding of the fp32 bound -- tests/half_ref.py):

  render    Shelf cameras (5 views, J = 17), B = 8 frames, 4 people a view, 128 x 240
            heatmaps (H x W): render_keypoints + .half()  vs  render_keypoints(dtype=float16)
  tail      the backbone's tail on 40 images' 128 x 240 x 256 features: the fp32 1x1 final
            layer (256 -> 15) + .half()  vs  fvp_conv1x1_cl_f16
  pipeline  the views pipeline from those features on: heatmaps -> cube + xy
            (C2: 8 frames x 5 views, ProjectLayer.forward_fused on the fp16 heatmaps)

Method as tools/bench_cl_half.py: one process, HIP events around blocks of --ops calls
after 3 warm-up calls, --repeats blocks; median [min-max] of the per-call time.  The bar:
direct is not slower than cast by more than the larger of the two lines' spreads.

    python tools/bench_heatmaps_f16.py [--out profiles/heatmaps_f16] [--only render,tail,pipeline]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "faster-voxelpose_amd"))


def timed(fn, ops, repeats, warmup=3):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ops):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) * 1e3 / ops)  # us
    return {"median_us": round(statistics.median(per_call), 2), "min_us": round(min(per_call), 2),
            "max_us": round(max(per_call), 2)}


def compare(name, cast, direct, args, **info):
    out = dict(bench=name, **info)
    out["cast"] = timed(cast, args.ops, args.repeats)
    out["direct"] = timed(direct, args.ops, args.repeats)
    c, d = out["cast"], out["direct"]
    spread = max(c["max_us"] - c["min_us"], d["max_us"] - d["min_us"])
    out["cast_over_direct"] = round(c["median_us"] / d["median_us"], 3)
    out["bar"] = {"direct_minus_cast_us": round(d["median_us"] - c["median_us"], 2), "spread_us": round(spread, 2),
                  "met": bool(d["median_us"] - c["median_us"] <= spread)}
    return out


def render_line(args, dev):
    import numpy as np
    import torch

    from fvp.heatmaps import render_keypoints
    from fvp.workloads import WORKLOADS

    w = dataclasses.replace(WORKLOADS["shelf_native"], heatmap_size=(240, 128))
    B, V, P, J = 8, 5, 4, w.num_joints
    rng = np.random.default_rng(7)  # people 100 .. 300 px across, centred on the image (tools/bench_render.py)
    centre = rng.uniform((0.15 * w.image_size[0], 0.2 * w.image_size[1]),
                         (0.85 * w.image_size[0], 0.8 * w.image_size[1]), size=(B, V, P, 1, 2))
    extent = rng.uniform(100.0, 300.0, size=(B, V, P, 1, 1)) * np.array([0.45, 1.0])
    joints = torch.from_numpy(centre + rng.uniform(-0.5, 0.5, size=(B, V, P, J, 2)) * extent).to(dev)
    count = torch.full((B, V), P, dtype=torch.int32, device=dev)
    kw = dict(image_size=w.image_size, heatmap_size=w.heatmap_size, sigma=3.0)
    a = render_keypoints(joints, count, **kw).half()
    b = render_keypoints(joints, count, dtype=torch.float16, **kw)
    same = bool(torch.equal(a.t.view(torch.int16), b.t.view(torch.int16)))
    return compare("render", lambda: render_keypoints(joints, count, **kw).half(),
                   lambda: render_keypoints(joints, count, dtype=torch.float16, **kw), args,
                   frames=B, views=V, people=P, joints=J, H=128, W=240, Cp=b.cp, bytes_fp16=b.t.numel() * 2,
                   same_bits=same)


def tail_and_pipeline(args, dev, which):
    import torch
    import torch.nn as nn

    from fvp import geometry
    from fvp.backbone import conv1x1_cl_f16
    from fvp.cnn import Act, ConvLayer
    from fvp.heatmaps import ChannelsLastHeatmaps
    from fvp.project_whole import ProjectLayer
    from fvp.workloads import WORKLOADS

    w = WORKLOADS["c2"]
    B, V, J = 8, 5, w.num_joints
    H, W, C = w.heatmap_size[1], w.heatmap_size[0], 256
    g = torch.Generator().manual_seed(11)
    conv = nn.Conv2d(C, J, 1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.016 / C ** 0.5)
        conv.bias.copy_(torch.randn(J, generator=g) * 0.1)
    final = ConvLayer(conv.to(dev), None)
    x = Act(torch.randn((B * V, H, W, C), generator=g).clamp_(min=0).to(dev), C)

    def cast():
        y = final(x, relu=False)
        return ChannelsLastHeatmaps(y.t.view(B, V, H, W, y.Cp), J).half()

    def direct():
        return ChannelsLastHeatmaps(conv1x1_cl_f16(final, x).view(B, V, H, W, final.Cpo), J)

    a, b = cast().t.float(), direct().t.float()
    info = dict(images=B * V, H=H, W=W, Cin=C, joints=J, Cp=final.Cpo, bytes_in=x.t.numel() * 4,
                max_abs_diff=float((a - b).abs().max()), max_abs=float(a.abs().max()))
    del a, b
    lines = []
    if "tail" in which:
        lines.append(compare("tail", cast, direct, args, **info))
        t = lines[-1]["direct"]["median_us"]
        lines[-1]["direct_gbs"] = round((info["bytes_in"] + B * V * H * W * final.Cpo * 2) / t / 1e3, 1)
    if "pipeline" in which:
        layer = ProjectLayer(w.cfg(str(dev)))
        layer.verbose = False
        cams, seq = w.cameras()
        rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float).to(dev)
        meta = {"seq": [seq] * B}
        lines.append(compare("pipeline", lambda: layer.forward_fused(cast(), meta, cams, rt),
                             lambda: layer.forward_fused(direct(), meta, cams, rt), args, workload="c2", **info))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "heatmaps_f16"))
    ap.add_argument("--only", default="render,tail,pipeline")
    ap.add_argument("--ops", type=int, default=20, help="timed calls per block (>= 20)")
    ap.add_argument("--repeats", type=int, default=5, help="blocks (>= 5)")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_heatmaps_f16: no HIP device (times are measured on the GPU only)")
    dev = torch.device("cuda:0")
    which = args.only.split(",")
    lines = []
    if "render" in which:
        lines.append(render_line(args, dev))
    if "tail" in which or "pipeline" in which:
        lines += tail_and_pipeline(args, dev, which)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench.jsonl"), "w") as f:
        for res in lines:
            res.update(ops=args.ops, repeats=args.repeats, device=torch.cuda.get_device_name(0))
            print(json.dumps(res), flush=True)
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
