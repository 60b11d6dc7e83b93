#!/usr/bin/env python3
"""fp16 channels-last heatmaps against the other three input formats, same process.

For each config the four routes -- planar fp32, channels-last fp32 (both unchanged
code: the time reference), planar fp16 (pixel-pair table) and channels-last fp16
(read in place, 8 joints per 16-B lane load) -- run the same op on the same
seeded frames (fvp/synthetic.py, rounded to fp16 once and shared by all routes,
so every route computes the same cube; checked).  HIP events around blocks of
--ops calls after a warm-up, --repeats blocks; the median and the min-max spread
of the per-call time of the blocks are reported, and each ratio.

    python tools/bench_cl_half.py [--out profiles/cl_half] [--configs c2_b256,c2_b8,c3_b8,c5_b8,jln]
    rocprofv3 --pmc SQ_INSTS_VMEM_RD SQ_WAVES ... -- python tools/bench_cl_half.py --counters cl16
        (a counters-only run: 3 calls of one route's C2 B = 8 gather, nothing else)
    python tools/bench_cl_half.py --pmc-summary DIR   (DIR/<route>/**/*counter_collection.csv -> per-dispatch sums)

The ceiling is DESIGN.md §5's arithmetic (bench.tap_floor_ceiling): tap wave-loads
x 16.5 cycles over 256 CUs at 2.4 GHz, no layout pass for channels-last input.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "faster-voxelpose_amd"))

TAP_CYCLES, CUS, CLOCK_HZ = 16.5, 256, 2.4e9  # bench.TAP_CYCLES_PER_WAVELOAD, CUS, CLOCK_HZ
ROUTES = ("planar32", "cl32", "planar16", "cl16")
# (workload, frames, distinct seeded frames rendered: a large batch tiles them -- its
#  bytes are distinct memory all the same, so B = 256 stays HBM-cold)
WHOLE = {"c2_b256": ("c2", 256, 16), "c2_b8": ("c2", 8, 8), "c3_b8": ("c3", 8, 8), "c5_b8": ("c5", 8, 8)}


def lanes(J, route):
    js = min(J, 32)
    if route == "cl16":
        return 1 if js <= 8 else 2 if js <= 16 else 4
    return 1 if js <= 4 else 2 if js <= 8 else 4 if js <= 16 else 8


def tap_floor_us(n_vox, V, J, route):
    """Tap wave-loads per frame x 16.5 cycles (J <= 32: one slice).  The planar fp16
    route's pair table takes 2 row loads per voxel-camera at 4 lanes."""
    per_vc = 2 * 4 if (route == "planar16" and J <= 16) else 4 * lanes(J, route)
    wave_loads = n_vox * V * per_vc * 16 / 1024.0
    return wave_loads, wave_loads * TAP_CYCLES / (CUS * CLOCK_HZ) * 1e6


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


def inputs(w, B, distinct, dev):
    """The four formats of the same fp16-rounded frames."""
    import torch

    from fvp import synthetic
    from fvp.heatmaps import to_channels_last

    base = torch.from_numpy(synthetic.gaussian_heatmaps(w, distinct)).half()
    h16 = base.repeat((B + distinct - 1) // distinct, 1, 1, 1, 1)[:B].contiguous().to(dev)
    h32 = h16.float()
    return {"planar32": h32, "cl32": to_channels_last(h32), "planar16": h16,
            "cl16": to_channels_last(h16, dtype=torch.float16)}


def whole_config(name, args, dev):
    import torch

    from fvp import geometry
    from fvp.project_whole import ProjectLayer
    from fvp.workloads import WORKLOADS

    wname, B, distinct = WHOLE[name]
    w = WORKLOADS[wname]
    layer = ProjectLayer(w.cfg(str(dev)))
    layer.verbose = False
    cams, seq = w.cameras()
    rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float).to(dev)
    meta = {"seq": [seq] * B}
    hm = inputs(w, B, distinct, dev)
    V, J = hm["planar32"].shape[1:3]
    n_vox = w.voxels_per_axis[0] * w.voxels_per_axis[1] * w.voxels_per_axis[2]
    out = {"config": name, "workload": wname, "frames": B, "views": V, "joints": J,
           "on_the_fly": bool(layer._project_on_the_fly(V)), "routes": {}}
    ref = None
    for r in ROUTES:
        cube, xy = layer.forward_fused(hm[r], meta, cams, rt)
        if ref is None:
            ref = (cube[:2].clone(), xy[:2].clone())
        same = bool(torch.equal(cube[:2], ref[0]) and torch.equal(xy[:2], ref[1]))
        del cube, xy
        t = timed(lambda: layer.forward_fused(hm[r], meta, cams, rt), args.ops, args.repeats)
        wl, floor = tap_floor_us(n_vox, V, J, r)
        t.update(us_per_frame=round(t["median_us"] / B, 3), same_as_planar32=same,
                 tap_wave_loads_per_frame=round(wl), tap_floor_us_per_frame=round(floor, 3),
                 fraction_of_tap_floor=round(floor * B / t["median_us"], 3))
        out["routes"][r] = t
    ratios(out)
    return out


def jln_config(args, dev):
    """The JLN planes line: C3, 10 proposals x 32 frames, forward_batch (planes only, cached fine grid).
    There is no planar fp16 person kernel (a planar fp16 tensor is converted to fp32): not timed."""
    import numpy as np
    import torch

    from fvp import geometry, synthetic
    from fvp.project_individual import ProjectLayer
    from fvp.workloads import WORKLOADS

    w = WORKLOADS["c3"]
    F, P = 32, 10
    layer = ProjectLayer(w.cfg(str(dev)))
    layer.verbose = False
    cams, seq = w.cameras()
    rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float).to(dev)
    hm = inputs(w, F, F, dev)
    rng = np.random.default_rng(5)
    props = []
    for f in range(F):  # as tools/bench_jln.py
        pr = synthetic.proposals_for_frame(w, f, 4)
        extra = np.zeros((P - 4, 7), np.float32)
        extra[:, 0] = w.space_center[0] + rng.uniform(-3500, 3500, P - 4)
        extra[:, 1] = w.space_center[1] + rng.uniform(-3500, 3500, P - 4)
        extra[:, 2] = 900.0
        extra[:, 4] = 0.5
        extra[:, 5:7] = 0.5
        props.append(np.concatenate([pr, extra])[:P])
    props = torch.from_numpy(np.stack(props)).to(dev)
    mask = torch.ones((F, P), dtype=torch.bool, device=dev)
    idx = mask.nonzero()
    meta = {"seq": [seq] * F}
    out = {"config": "jln", "workload": "c3", "frames": F, "proposals": F * P, "routes": {}}
    ref = None
    for r in ("planar32", "cl32", "cl16"):
        planes = layer.forward_batch(hm[r], meta, props, mask, cams, rt, idx=idx)[0]
        if ref is None:
            ref = planes.clone()
        same = bool(torch.equal(planes, ref))
        del planes
        t = timed(lambda: layer.forward_batch(hm[r], meta, props, mask, cams, rt, idx=idx), args.ops, args.repeats)
        t.update(us_per_proposal=round(t["median_us"] / (F * P), 3), same_as_planar32=same)
        out["routes"][r] = t
    ratios(out)
    return out


def ratios(out):
    r = out["routes"]
    m = {k: v["median_us"] for k, v in r.items()}
    out["ratios"] = {f"{a}/cl16": round(m[a] / m["cl16"], 3) for a in m if a != "cl16"}
    # the bar: cl16 not slower than cl32 by more than the line's own spread (the wider of the two routes')
    spread = max(r["cl32"]["max_us"] - r["cl32"]["min_us"], r["cl16"]["max_us"] - r["cl16"]["min_us"])
    out["bar"] = {"cl16_minus_cl32_us": round(m["cl16"] - m["cl32"], 2), "spread_us": round(spread, 2),
                  "met": bool(m["cl16"] - m["cl32"] <= spread)}


def counters_run(route, dev):
    """3 calls of one route's C2 B = 8 gather for a rocprofv3 --pmc run (counters alone)."""
    import torch

    from fvp import geometry
    from fvp.project_whole import ProjectLayer
    from fvp.workloads import WORKLOADS

    w = WORKLOADS["c2"]
    layer = ProjectLayer(w.cfg(str(dev)))
    layer.verbose = False
    cams, seq = w.cameras()
    rt = torch.as_tensor(geometry.resize_transform(w.ori_image_size, w.image_size), dtype=torch.float).to(dev)
    hm = inputs(w, 8, 8, dev)[route]
    for _ in range(3):
        layer.forward_fused(hm, {"seq": [seq] * 8}, cams, rt)
    torch.cuda.synchronize()


def pmc_summary(out):
    """Per gather kernel and route: the counters of the rocprofv3 CSVs under out/<route>/, per dispatch."""
    import collections
    import csv
    import glob

    for r in ROUTES:
        acc = collections.defaultdict(lambda: collections.defaultdict(float))
        n = collections.Counter()
        for f in glob.glob(os.path.join(out, r, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                k = row["Kernel_Name"].split("(")[0]
                if "voxelize" not in k:
                    continue
                acc[k][row["Counter_Name"]] += float(row["Counter_Value"])
                n[k] += row["Counter_Name"] == "SQ_WAVES"
        for k, v in acc.items():
            print(r, k, "dispatches", n[k], {c: round(x / max(n[k], 1)) for c, x in v.items()}, "per dispatch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cl_half"))
    ap.add_argument("--configs", default="c2_b256,c2_b8,c3_b8,c5_b8,jln")
    ap.add_argument("--ops", type=int, default=20, help="timed calls per block (>= 20)")
    ap.add_argument("--repeats", type=int, default=5, help="blocks (>= 5)")
    ap.add_argument("--counters", choices=ROUTES, default=None)
    ap.add_argument("--pmc-summary", metavar="DIR", default=None)
    args = ap.parse_args()
    if args.pmc_summary:
        pmc_summary(args.pmc_summary)
        return

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_cl_half: no HIP device (times are measured on the GPU only)")
    dev = torch.device("cuda:0")
    if args.counters:
        counters_run(args.counters, dev)
        return
    os.makedirs(args.out, exist_ok=True)
    lines = []
    for name in args.configs.split(","):
        res = jln_config(args, dev) if name == "jln" else whole_config(name, args, dev)
        res.update(ops=args.ops, repeats=args.repeats, device=torch.cuda.get_device_name(0))
        print(json.dumps(res), flush=True)
        lines.append(res)
        torch.cuda.empty_cache()
    with open(os.path.join(args.out, "bench_cl_half.jsonl"), "w") as f:
        for res in lines:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
