#!/usr/bin/env python3
"""Serving latency, one frame at a time (run/service.py's use): heatmaps -> poses, and with
--views camera frames -> poses, at C3 geometry with the seeded reference architectures of
tools/bench_pipeline.py on the fvp CNNs (cnn=True).

Arms (--arms):
  a  eager, the synced JLN route (the default route: one count read per batch)
  b  eager, FvpOptions.sync_free=True (no host read, all B*K slots through P2PNet)
  c  fvp.graphs.CapturedStep of the whole forward, one replay per frame

Method: one process; every arm warmed; --frames frames per arm (>= 200) in blocks of --block
that alternate between the arms; every frame copies a new input into the same static tensor
(what a replay needs; the eager arms pay the same copy) and is timed twice: host wall clock from
before the copy to after a device synchronise, and HIP events around the same span.  Reported:
median and p10 / p90 of both, per arm.

--live N marks only the first N of the K proposal slots of each frame valid (the seeded nets
score every slot valid, which hides the padded P2PNet batch's cost: with N < K the synced route
runs 3*N planes and the sync-free routes 3*K).  Arm a alone uses nothing newer than
CapturedStep, so the same file times a checkout that predates the sync-free route.

    python tools/bench_serve.py [--batch 1] [--live 10] [--arms a,b,c] [--views] [--out profiles/serve]

Appends one JSON line per arm to <out>/serve.jsonl.
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


def pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, max(0, round(q * (len(s) - 1))))]


def stats(v):
    return {"median": round(statistics.median(v), 4), "p10": round(pct(v, 0.1), 4), "p90": round(pct(v, 0.9), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--live", type=int, default=None, help="valid proposal slots per frame (default: all K)")
    ap.add_argument("--arms", default="a,b,c")
    ap.add_argument("--frames", type=int, default=200, help="timed frames per arm")
    ap.add_argument("--block", type=int, default=20, help="frames per alternating block")
    ap.add_argument("--views", action="store_true", help="start from uint8 camera frames (bf16 PoseResNet-50)")
    ap.add_argument("--tag", default="this tree")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "serve"))
    args = ap.parse_args()
    arms = [a for a in args.arms.split(",") if a]

    import numpy as np
    import torch
    import torch.nn as nn

    import cnn_arch
    from fvp import geometry, integration, jln, synthetic
    from fvp.config import AttrDict
    from fvp.graphs import CapturedStep
    from fvp.project_individual import ProjectLayer as PI
    from fvp.project_whole import ProjectLayer
    from fvp.workloads import WORKLOADS

    if not torch.cuda.is_available():
        raise SystemExit("bench_serve: no HIP device (times are measured on the GPU only)")
    dev = torch.device("cuda:0")
    w = WORKLOADS["c3"]
    J, B, K = w.num_joints, args.batch, w.max_people
    live = K if args.live is None else args.live
    cams, seq = w.cameras()
    V = len(cams[seq])
    rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float).to(dev)
    meta = {"seq": [seq] * B}

    class Proposal(nn.Module):  # test-mode ProposalLayer constants (tools/bench_pipeline.py): every slot valid
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
            if live < K:
                centers[:, live:, 3] = -1.0
            fused, poses = jln.fused_jln_forward(jl, meta, input_heatmaps, centers, centers[:, :, 3] >= 0, cameras,
                                                 resize_transform)
            fused = torch.cat((fused, centers[:, :, 3:5].reshape(B, -1, 1, 2).repeat(1, 1, J, 1)), dim=3)
            return fused, poses

    Net._fvp_original_forward = Net.forward
    Net.forward = integration.fused_fvp_forward
    model = Net()
    kw = dict(meta=meta, cameras=cams, resize_transform=rt)
    if args.views:
        from fvp.frames import Frames

        rn = seeded(cnn_arch.PoseResNet(50, J), 21)
        for m in (model, rn):
            integration.set_options(m, backbone=True, backbone_dtype=torch.bfloat16)
        Wi, Hi = w.image_size
        pool = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (4, B, V, Hi, Wi, 3), dtype=np.uint8)).to(dev)
        static = pool[0].clone()
        fr = Frames(static)
        run = lambda: model.forward(backbone=rn, views=fr, **kw)  # noqa: E731
    else:
        pool = torch.from_numpy(synthetic.gaussian_heatmaps(w, 4 * B)).to(dev).view(4, B, V, J, *reversed(w.heatmap_size))
        static = pool[0].clone()
        run = lambda: model.forward(input_heatmaps=static, **kw)  # noqa: E731

    def route(sync_free):
        def call():
            integration.set_options(jl, sync_free=sync_free)
            return run()
        return call

    steps, notes = {}, {}
    with torch.no_grad():
        if "a" in arms:
            steps["a"] = run if arms == ["a"] else route(False)
        if "b" in arms:
            steps["b"] = route(True)
        for fn in steps.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        if "c" in arms:
            try:
                integration.set_options(jl, sync_free=True)  # the warm-up runs the route the capture records
                cap = CapturedStep(run)
                steps["c"] = cap.replay
                if "b" in steps:  # the replay computes what the eager sync-free route computes
                    static.copy_(pool[1])
                    got = [t.clone() for t in cap.replay()]
                    ref = steps["b"]()
                    torch.cuda.synchronize()
                    notes["c_equals_b"] = bool(all(torch.equal(g, r) for g, r in zip(got, ref)))
            except Exception as e:  # noqa: BLE001 -- a refused capture is a result, recorded as such
                notes["c_error"] = f"{type(e).__name__}: {e}"[:400]
        wall = {k: [] for k in steps}
        devt = {k: [] for k in steps}
        n = 0
        for _ in range((args.frames + args.block - 1) // args.block):
            for k, fn in steps.items():
                for _ in range(args.block):
                    n += 1
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record()
                    static.copy_(pool[n % 4])
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    wall[k].append((time.perf_counter() - t0) * 1e3)
                    devt[k].append(e0.elapsed_time(e1))
    os.makedirs(args.out, exist_ok=True)
    names = {"a": "eager, synced JLN", "b": "eager, sync_free=True", "c": "CapturedStep replay"}
    with open(os.path.join(args.out, "serve.jsonl"), "a") as f:
        for k in steps:
            line = dict(bench="serve", tree=args.tag, arm=k, route=names[k],
                        span="frames -> poses" if args.views else "heatmaps -> poses", workload="c3", batch=B,
                        proposals_per_frame=K, live_per_frame=live, frames=len(wall[k]), block=args.block,
                        unit="ms per batch", wall=stats(wall[k]), device=stats(devt[k]),
                        gpu=torch.cuda.get_device_name(0), **notes)
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")
        if "c_error" in notes and "c" not in steps:
            line = dict(bench="serve", tree=args.tag, arm="c", batch=B, live_per_frame=live, **notes)
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
