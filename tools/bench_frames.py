#!/usr/bin/env python3
"""uint8 camera frames as the pipeline's input, against resident fp32 views.

Shapes: `batch40` = validate.py's batch, 8 frames x 5 per-view images of 960 x 512 (W x H);
`service` = one 2 x 2 mosaic frame of 960 x 512 views (run/service.py).

  stem      the backbone's 7x7 stem (fp32 and bf16 kernels), GPU time of three routes:
              a  the existing stem on fp32 views already in HBM (what the tree did before; the baseline)
              b  fvp_frames_to_views, then that stem
              c  the u8 stem reading the frames itself
            c's output is checked bit for bit against a's.  Bars: c - a <= the spread of a in
            this run; c < b.
  upload    with pinned host memory: the uint8 upload, the fp32 upload, and the CPU
            ToTensor + Normalize chain the fp32 upload needs first (host clock)
  pipeline  views -> poses through integration.fused_fvp_forward (C2, 8 frames, bf16
            PoseResNet-50 backbone, fvp CNNs) with a resident fp32 tensor and with Frames

Method as tools/bench_heatmaps_f16.py: one process, HIP events around blocks of --ops calls
after 3 warm-up calls, --repeats blocks, the routes of a comparison alternating block by
block; median [min-max] of the per-call time.

    python tools/bench_frames.py [--out profiles/frames] [--only stem,upload,pipeline]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "faster-voxelpose_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

H, W = 512, 960


def summary(per_call):
    return {"median_us": round(statistics.median(per_call), 2), "min_us": round(min(per_call), 2),
            "max_us": round(max(per_call), 2)}


def timed_alternating(fns, ops, repeats, warmup=3):
    """{name: fn} -> {name: summary}: per repeat one timed block of `ops` calls of each route in turn."""
    import torch

    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    per_call = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(ops):
                fn()
            e1.record()
            torch.cuda.synchronize()
            per_call[k].append(e0.elapsed_time(e1) * 1e3 / ops)  # us
    return {k: summary(v) for k, v in per_call.items()}


def shapes():
    import numpy as np
    import torch

    from fvp.frames import Frames

    rng = np.random.default_rng(3)
    batch = torch.from_numpy(rng.integers(0, 256, (8, 5, H, W, 3), dtype=np.uint8))
    frame = torch.from_numpy(rng.integers(0, 256, (1, 2 * H, 2 * W, 3), dtype=np.uint8))
    return {"batch40": (batch, None), "service": (frame, (2, 2))}, Frames


def stem_lines(args, dev):
    import ctypes

    import torch

    import cnn_arch
    from fvp import _lib, synthetic
    from fvp.backbone import FvpPoseResNet
    from fvp.ops import _ptr, _stream

    cases, Frames = shapes()
    m = cnn_arch.PoseResNet(18, 15).eval()  # the stem is the same layer at every depth
    m.load_state_dict(synthetic.seeded_state_dict(m, 21))
    m = m.to(dev)
    lines = []
    for dtype in (torch.float32, torch.bfloat16):
        bb = FvpPoseResNet(m, dtype)
        bf16 = dtype == torch.bfloat16
        stem = bb._stem7 if bf16 else bb._stem7_f32
        wpack = bb.stem7 if bf16 else bb.stem7_f32
        name = "fvp_conv_stem7_u8_bf16" if bf16 else "fvp_conv_stem7_u8_f32"
        for shape, (data, mosaic) in cases.items():
            fr = Frames(data.to(dev), mosaic=mosaic)
            views = fr.views().flatten(0, 1)
            N = views.shape[0]
            out = torch.empty((N, H // 2, W // 2, 64), dtype=dtype, device=dev)

            def u8():
                _lib.call(name, _ptr(fr.data), fr.B, ctypes.byref(fr.spec), _ptr(wpack), _ptr(bb.stem.scale),
                          _ptr(bb.stem.shift), _ptr(out), _stream(out))
                return out

            same = bool(torch.equal(stem(views).t, u8()))
            t = timed_alternating({"a_stem_on_views": lambda: stem(views),
                                   "b_frames_to_views_then_stem": lambda: stem(fr.views().flatten(0, 1)),
                                   "c_u8_stem": u8, "frames_to_views_alone": fr.views}, args.ops, args.repeats)
            a, b, c = t["a_stem_on_views"], t["b_frames_to_views_then_stem"], t["c_u8_stem"]
            spread_a = a["max_us"] - a["min_us"]
            lines.append(dict(bench="stem", shape=shape, stem="bf16" if bf16 else "fp32", views=N, H=H, W=W,
                              same_bits=same, **t, bytes_u8=fr.data.numel(), bytes_fp32_views=views.numel() * 4,
                              bytes_out=out.numel() * out.element_size(),
                              c_over_a=round(c["median_us"] / a["median_us"], 3),
                              c_over_b=round(c["median_us"] / b["median_us"], 3),
                              bar={"c_minus_a_us": round(c["median_us"] - a["median_us"], 2),
                                   "spread_a_us": round(spread_a, 2),
                                   "c_not_slower_than_a": bool(c["median_us"] - a["median_us"] <= spread_a),
                                   "c_beats_b": bool(c["median_us"] < b["median_us"])}))
            print(json.dumps(lines[-1]), flush=True)
    return lines


def upload_lines(args, dev):
    import torch

    cases, Frames = shapes()
    lines = []
    for shape, (data, mosaic) in cases.items():
        fr = Frames(data, mosaic=mosaic)
        t0 = time.perf_counter()
        cpu_views = fr.views()  # the reference's CPU chain (ToTensor + Normalize), all views at once
        chain = [time.perf_counter() - t0]
        for _ in range(2):
            t0 = time.perf_counter()
            fr.views()
            chain.append(time.perf_counter() - t0)
        u8_host, f32_host = data.pin_memory(), cpu_views.pin_memory()
        u8_dev, f32_dev = torch.empty_like(data, device=dev), torch.empty_like(cpu_views, device=dev)
        t = timed_alternating({"upload_u8": lambda: u8_dev.copy_(u8_host, non_blocking=True),
                               "upload_fp32": lambda: f32_dev.copy_(f32_host, non_blocking=True)},
                              args.ops, args.repeats)
        lines.append(dict(bench="upload", shape=shape, bytes_u8=data.numel(), bytes_fp32=cpu_views.numel() * 4, **t,
                          u8_gbs=round(data.numel() / t["upload_u8"]["median_us"] / 1e3, 1),
                          fp32_gbs=round(cpu_views.numel() * 4 / t["upload_fp32"]["median_us"] / 1e3, 1),
                          cpu_chain_ms=[round(1e3 * v, 1) for v in chain], cpu_threads=torch.get_num_threads()))
        print(json.dumps(lines[-1]), flush=True)
    return lines


def pipeline_lines(args, dev):
    """views -> poses: the reference's FasterVoxelPoseNet flow (faster_voxelpose.py:73-93) on the fused
    HDN / JLN forwards, entered through fused_fvp_forward."""
    import numpy as np
    import torch
    import torch.nn as nn

    import cnn_arch
    from fvp import geometry, integration, jln, synthetic
    from fvp.config import AttrDict
    from fvp.frames import Frames
    from fvp.project_individual import ProjectLayer as PI
    from fvp.project_whole import ProjectLayer
    from fvp.workloads import WORKLOADS

    w = WORKLOADS["c2"]
    J, B, K = w.num_joints, 8, w.max_people
    cams, seq = w.cameras()
    V = len(cams[seq])
    rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float).to(dev)
    meta = {"seq": [seq] * B}

    class Proposal(nn.Module):  # test-mode ProposalLayer constants (tools/bench_pipeline.py)
        scale = [float(s) / (float(n) - 1) for s, n in zip(w.space_size, w.voxels_per_axis)]
        bias = [float(c) - float(s) / 2.0 for c, s in zip(w.space_center, w.space_size)]
        min_score = -1.0

    def seeded(mod, seed):
        mod = mod.eval()
        mod.load_state_dict(synthetic.seeded_state_dict(mod, seed))
        return mod.to(dev)

    hdn = types.SimpleNamespace(max_people=K, proposal_layer=Proposal(), center_net=seeded(cnn_arch.CenterNet(J, 1), 12),
                                c2c_net=seeded(cnn_arch.C2CNet(J, 1), 14), project_layer=ProjectLayer(w.cfg(str(dev))))
    jl = types.SimpleNamespace(training=False, conv_net=seeded(cnn_arch.P2PNet(J, J), 11),
                               weight_net=seeded(cnn_arch.WeightNet(J), 15), project_layer=PI(w.cfg(str(dev))),
                               soft_argmax_layer=jln.SoftArgmaxLayer(AttrDict.wrap({"NETWORK": {"BETA": 100}})))
    hdn.project_layer.verbose = jl.project_layer.verbose = False
    for net in (hdn, jl):
        integration.set_options(net, cnn=True)

    class Net:
        training = False

        def forward(self, backbone=None, views=None, meta=None, targets=None, input_heatmaps=None, cameras=None,
                    resize_transform=None):
            if views is not None:
                input_heatmaps = torch.stack([backbone(views[:, c]) for c in range(views.shape[1])], dim=1)
            _, _, centers, _ = integration.fused_hdn_forward(hdn, input_heatmaps, meta, cameras, resize_transform)
            centers[:, :, 5:7].clamp_(0.3, 0.8)  # seeded bbox head: keep every person window non-empty
            fused, _ = jln.fused_jln_forward(jl, meta, input_heatmaps, centers, centers[:, :, 3] >= 0, cameras,
                                             resize_transform)
            return fused

    Net._fvp_original_forward = Net.forward
    Net.forward = integration.fused_fvp_forward
    model = Net()
    rn = seeded(cnn_arch.PoseResNet(50, J), 21)
    Wi, Hi = 4 * w.heatmap_size[0], 4 * w.heatmap_size[1]  # 960 x 512: the backbone's heatmaps are a quarter
    data = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (B, V, Hi, Wi, 3), dtype=np.uint8)).to(dev)
    fr = Frames(data)
    views = fr.views()
    lines = []
    for tag, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        integration.set_options(model, backbone=True, backbone_dtype=dtype)
        integration.set_options(rn, backbone=True, backbone_dtype=dtype)
        kw = dict(backbone=rn, meta=meta, cameras=cams, resize_transform=rt)
        with torch.no_grad():
            same = bool(torch.equal(model.forward(views=views, **kw), model.forward(views=fr, **kw)))
            t = timed_alternating({"tensor_views": lambda: model.forward(views=views, **kw),
                                   "frames_views": lambda: model.forward(views=fr, **kw)}, max(args.ops // 4, 5),
                                  args.repeats)
        a, c = t["tensor_views"], t["frames_views"]
        lines.append(dict(bench="pipeline", workload="c2", frames=B, views=B * V, H=Hi, W=Wi, backbone="r50 " + tag,
                          same_poses=same, **t, frames_over_tensor=round(c["median_us"] / a["median_us"], 4),
                          spread_tensor_us=round(a["max_us"] - a["min_us"], 2)))
        print(json.dumps(lines[-1]), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "frames"))
    ap.add_argument("--only", default="stem,upload,pipeline")
    ap.add_argument("--ops", type=int, default=20, help="timed calls per block (>= 20)")
    ap.add_argument("--repeats", type=int, default=5, help="blocks (>= 5)")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_frames: no HIP device (times are measured on the GPU only)")
    dev = torch.device("cuda:0")
    os.makedirs(args.out, exist_ok=True)
    for which, fn in (("stem", stem_lines), ("upload", upload_lines), ("pipeline", pipeline_lines)):
        if which not in args.only.split(","):
            continue
        with open(os.path.join(args.out, f"bench_{which}.jsonl"), "w") as f:
            for res in fn(args, dev):
                res.update(ops=args.ops, repeats=args.repeats, device=torch.cuda.get_device_name(0))
                f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
