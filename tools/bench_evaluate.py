#!/usr/bin/env python3
"""Scoring a run: fvp.evaluate (one matching launch over all frames, one copy to the host,
vectorised numpy scoring) against the per-frame host loop the reference's evaluate methods run
(tests/eval_ref.py, fed the same device tensor: one ``preds[i].cpu()`` per frame), on synthetic
runs of the real sizes:

  panoptic   N = 2,048 frames, K = 10 slots, 0-6 people of max_people 10, J = 15
  shelf      N = 301 frames (Shelf's frame range), K = 10 slots, A = 4 actors

Both sides start from the predictions on the device and end with (metric, msg) on the host;
wall clock around each call (both have host parts and end synchronised).  One warm-up of each,
then --repeats alternating repeats; the median and the min-max spread.  The two messages must be
equal (they are compared, not assumed).  Also records the evaluate time beside the forward's
time for the same N frames, from the pipeline benchmark's record (--pipeline).

    python tools/bench_evaluate.py [--out profiles/evaluate/bench_evaluate.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPELINE = os.path.join(REPO, "profiles", "round6", "final", "pipeline.jsonl")


def panoptic_run(N, K, G, J, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    count = rng.integers(0, 7, N)
    joints = rng.uniform(-3000.0, 3000.0, (N, G, 1, 3)) + rng.normal(0.0, 300.0, (N, G, J, 3))
    vis = (rng.random((N, G, J)) > 0.1).astype(np.float64)
    preds = np.zeros((N, K, J, 5), np.float32)
    pick = rng.integers(0, np.maximum(count, 1)[:, None], (N, K))
    sigma = rng.choice([10.0, 25.0, 50.0, 90.0, 400.0], (N, K, 1, 1))
    preds[..., :3] = joints[np.arange(N)[:, None], pick] + rng.normal(0.0, 1.0, (N, K, J, 3)) * sigma
    preds[..., 3] = np.where(rng.random((N, K)) < 0.5, 0.0, -1.0)[:, :, None]
    preds[..., 4] = rng.random((N, K), np.float32)[:, :, None]
    return preds, joints, vis, count.astype(np.int32)


def shelf_run(N, K, A, seed):
    import numpy as np

    import eval_ref as E

    rng = np.random.default_rng(seed)
    truth = rng.uniform(-2000.0, 2000.0, (N, A, 1, 3)) + rng.normal(0.0, 250.0, (N, A, 17, 3))
    gt = np.stack([[E.convert_pose(truth[i, a].astype(np.float32), E.SHELF) for a in range(A)] for i in range(N)])
    present = rng.random((N, A)) > 0.25
    preds = np.zeros((N, K, 17, 5), np.float32)
    pick = rng.integers(0, A, (N, K))
    sigma = rng.choice([15.0, 60.0, 110.0, 160.0, 450.0], (N, K, 1, 1))
    preds[..., :3] = truth[np.arange(N)[:, None], pick] + rng.normal(0.0, 1.0, (N, K, 17, 3)) * sigma
    flag = np.where(rng.random((N, K)) < 0.4, 0.0, -1.0)
    flag[:, 0] = 0.0
    preds[..., 3] = flag[:, :, None]
    preds[..., 4] = rng.random((N, K), np.float32)[:, :, None]
    return preds, gt, present


def forward_ms_per_frame(path):
    """ms per frame of the heatmaps -> poses forward, from the pipeline benchmark's record."""
    if not os.path.exists(path):
        return None
    with open(path) as f:
        for line in f:
            rec = json.loads(line)
            if rec.get("backbone_ms") is None and "ms_per_batch" in rec:
                return rec["ms_per_batch"] / rec["frames"]
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pipeline", default=PIPELINE, help="the pipeline benchmark's JSON lines (forward time)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "faster-voxelpose_amd"))
    sys.path.insert(0, os.path.join(REPO, "tests"))

    import numpy as np
    import torch

    import eval_ref as E
    from fvp import evaluate as V

    if not torch.cuda.is_available():
        raise SystemExit("bench_evaluate: no HIP device (the baseline's per-frame copies need one too)")
    dev = torch.device("cuda:0")
    per_frame = forward_ms_per_frame(args.pipeline)

    def measure(ours, loop):
        want, got = loop(), ours()  # the warm-up of each, and the results to compare
        torch.cuda.synchronize()
        t = {"ours": [], "loop": []}
        for _ in range(args.repeats):
            for name, fn in (("ours", ours), ("loop", loop)):
                t0 = time.perf_counter()
                fn()
                t[name].append((time.perf_counter() - t0) * 1e3)
        stat = {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3),
                    "max_ms": round(max(v), 3)} for k, v in t.items()}
        return stat, bool(float(got[0]) == float(want[0]) and got[1] == want[1])

    lines = []
    N, K, G, J = 2048, 10, 10, 15
    preds, joints, vis, count = panoptic_run(N, K, G, J, 1)
    p = torch.from_numpy(preds).to(dev)
    t0 = time.perf_counter()
    gt = V.PanopticGroundTruth.from_db([{"meta": {"num_person": int(count[i]), "joints_3d": joints[i],
                                                  "joints_3d_vis": vis[i]}} for i in range(N)]).to(dev)
    build_ms = (time.perf_counter() - t0) * 1e3
    stat, same = measure(lambda: V.panoptic(p, gt), lambda: E.panoptic(p, joints, vis, count)[:2])
    lines.append(("panoptic", dict(N=N, K=K, max_people=G, J=J, people=int(count.sum())), stat, same, build_ms))

    N, K, A = 301, 10, 4
    preds, agt, present = shelf_run(N, K, A, 2)
    p2 = torch.from_numpy(preds).to(dev)
    t0 = time.perf_counter()
    gt2 = V.ActorGroundTruth(torch.from_numpy(agt), torch.from_numpy(present.astype(np.uint8))).to(dev)
    build_ms = (time.perf_counter() - t0) * 1e3
    stat, same = measure(lambda: V.pcp(p2, gt2, V.SHELF), lambda: E.pcp(p2, agt, present, E.SHELF)[:2])
    lines.append(("shelf", dict(N=N, K=K, A=A), stat, same, build_ms))

    for name, shape, stat, same, build_ms in lines:
        ours, loop = stat["ours"]["median_ms"], stat["loop"]["median_ms"]
        forward = None if per_frame is None else round(per_frame * shape["N"], 1)
        line = {"bench": "evaluate", "dataset": name, **shape, "device": torch.cuda.get_device_name(0),
                "fvp_evaluate": stat["ours"], "host_loop": stat["loop"], "loop_over_fvp": round(loop / ours, 1),
                "same_metric_and_message": same, "ground_truth_build_ms_once": round(build_ms, 2),
                "forward_ms_same_frames": forward,
                "loop_share_of_forward_plus_loop": None if forward is None else round(loop / (forward + loop), 3),
                "fvp_share_of_forward_plus_fvp": None if forward is None else round(ours / (forward + ours), 4),
                "timing": f"host clock around each call, predictions on the device, result on the host; one "
                          f"warm-up, {args.repeats} alternating repeats; median and min-max"}
        s = json.dumps(line)
        print(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(s + "\n")


if __name__ == "__main__":
    main()
