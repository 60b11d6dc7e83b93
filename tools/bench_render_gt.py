#!/usr/bin/env python3
"""'gt' heatmap source line: fvp.heatmaps.render_poses3d (fvp_render_poses3d, one launch from
3-D poses to channels-last heatmaps) on the renderer's bench workload -- the 5 Shelf cameras,
B = 8 frames, 4 people, J = 17, heatmaps 128 x 240 -- in fp32 and fp16, against

  (a)  the route without it: the projection on the host (the numpy restatement of
       tests/render_gt_ref.py; (a_vec): a vectorised numpy projection with BLAS products, the
       cheapest host implementation), the upload of the 2-D keypoints, render_keypoints(vis).
       Wall clock around a synchronised call, because it has a host part.
  (b)  render_keypoints alone on the same keypoints already on the device
  (c)  render_poses3d
  (d)  project_poses, then render_keypoints: two launches

One process, HIP events (b, c, d), 3 warm-ups, --repeats blocks of --calls calls; the median and
the min-max spread of the blocks' per-call times.  One JSON line per dtype.

    python tools/bench_render_gt.py [--out FILE] [--save-keypoints FILE]
    python tools/bench_render_gt.py --tree OTHER_CHECKOUT --keypoints FILE   # (b) alone, on another build

The second form times (b) with another checkout's package (one that may lack the 'gt' entry points)
on the keypoints the first form saved, to show that the existing launches cost what they did.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ORI, IMAGE, HEATMAP, J, SIGMA = (1032, 776), (800, 608), (240, 128), 17, 3.0


def poses(B, P, seed):
    """[B, P, J, 3] fp64: people around the Shelf capture space's centre, most joints in most views."""
    import numpy as np

    rng = np.random.default_rng(seed)
    space_centre, space_size = np.array([450.0, -320.0, 800.0]), np.array([8000.0, 8000.0, 2000.0])
    centre = space_centre + rng.uniform(-0.15, 0.15, (B, P, 1, 3)) * space_size
    return centre + rng.normal(size=(B, P, J, 3)) * (200.0, 200.0, 400.0)


def project_vectorised(joints3d, cams, t, ori, image):
    """The host projection with numpy's own matrix products, every joint of the batch per view at once."""
    import numpy as np

    x = joints3d.reshape(-1, 3).T
    j2 = np.empty((joints3d.shape[0], cams.shape[0]) + joints3d.shape[1:3] + (2,))
    v2 = np.empty(j2.shape[:-1], np.uint8)
    for v, cam in enumerate(cams):
        xc = np.matmul(cam[0:9].reshape(3, 3), x - cam[9:12, None])
        y = xc[:2] / (xc[2] + 1e-5)
        r = np.sum(y ** 2, axis=0)
        k, p = cam[16:19], cam[19:21]
        d = 1 + k[0] * r + k[1] * r * r + k[2] * r * r * r
        u = y[0] * d + 2 * p[0] * y[0] * y[1] + p[1] * (r + 2 * y[0] * y[0])
        w = y[1] * d + 2 * p[1] * y[0] * y[1] + p[0] * (r + 2 * y[1] * y[1])
        px, py = cam[12] * u + cam[14], cam[13] * w + cam[15]
        q = np.matmul(t, np.stack([px, py, np.ones_like(px)]))
        vis = ((px >= 0) & (px <= ori[0] - 1) & (py >= 0) & (py <= ori[1] - 1)
               & ~((np.minimum(q[0], q[1]) < 0) | (q[0] >= image[0]) | (q[1] >= image[1])))
        j2[:, v] = q.T.reshape(joints3d.shape[:3] + (2,))
        v2[:, v] = vis.reshape(joints3d.shape[:3])
    return j2, v2


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--people", type=int, default=4)
    ap.add_argument("--calls", type=int, default=20, help="calls per block")
    ap.add_argument("--repeats", type=int, default=5, help="blocks")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--tree", default=REPO, help="checkout whose package is measured (default: this one)")
    ap.add_argument("--keypoints", default=None, help="time (b) alone on the keypoints in this file")
    ap.add_argument("--save-keypoints", default=None, help="write the keypoints of (b) to this file")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "faster-voxelpose_amd"))

    import numpy as np
    import torch

    from fvp.heatmaps import render_keypoints

    if not torch.cuda.is_available():
        raise SystemExit("bench_render_gt: no HIP device (nothing is measured on the host alone)")
    dev = torch.device("cuda:0")
    B, P = args.frames, args.people
    kw = dict(image_size=IMAGE, heatmap_size=HEATMAP, sigma=SIGMA)

    def blocks(fn, calls, wall=False):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        per_call = []
        for _ in range(args.repeats):
            if wall:
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                    torch.cuda.synchronize()
                per_call.append((time.perf_counter() - t0) * 1e6 / calls)
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            per_call.append(e0.elapsed_time(e1) * 1e3 / calls)
        return {"median_us": round(statistics.median(per_call), 2), "min_us": round(min(per_call), 2),
                "max_us": round(max(per_call), 2), "calls": calls, "blocks": args.repeats}

    lines = []
    if args.keypoints:  # (b) alone, on another build
        d = np.load(args.keypoints)
        j2, v2, cnt = (torch.from_numpy(d[k]).to(dev) for k in ("joints2d", "vis2d", "count"))
        for dtype in (torch.float32, torch.float16):
            lines.append({"bench": "render_gt", "tree": "." if args.tree == REPO else args.tree, "dtype": str(dtype),
                          "b_render_keypoints": blocks(lambda: render_keypoints(j2, cnt, v2, dtype=dtype, **kw),
                                                       args.calls)})
    else:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import render_gt_ref as G
        from fvp.heatmaps import project_poses, render_poses3d

        joints3d = poses(B, P, 7)
        cams, t = np.array(G.cameras64("shelf")), G.resize_transform("shelf", image_size=IMAGE)
        count = np.full((B,), P, np.int32)
        V = cams.shape[0]
        sizes = dict(ori_image_size=ORI, image_size=IMAGE)
        j3_d, cnt_d, cams_d, t_d = (torch.from_numpy(a).to(dev) for a in (joints3d, count, cams, t))
        cnt_bv = cnt_d[:, None].expand(-1, V).contiguous()
        ref_j2, ref_v2 = G.project_batch(joints3d, None, count, cams[None], None, t, ORI, IMAGE)
        vec_j2, vec_v2 = project_vectorised(joints3d, cams, t, ORI, IMAGE)
        j2_d, v2_d = project_poses(j3_d, None, cnt_d, cams_d, t_d, **sizes)
        same_projection = bool(np.array_equal(j2_d.cpu().numpy(), ref_j2)
                               and np.array_equal(v2_d.cpu().numpy(), ref_v2))
        rkw = dict(heatmap_size=HEATMAP, sigma=SIGMA, **sizes)
        if args.save_keypoints:
            os.makedirs(os.path.dirname(os.path.abspath(args.save_keypoints)), exist_ok=True)
            np.savez(args.save_keypoints, joints2d=ref_j2, vis2d=ref_v2, count=cnt_bv.cpu().numpy())

        def host_route(project, dtype):
            def fn():
                j2, v2 = project()
                return render_keypoints(torch.from_numpy(j2).to(dev), cnt_bv, torch.from_numpy(v2).to(dev),
                                        dtype=dtype, **kw)
            return fn

        for dtype in (torch.float32, torch.float16):
            one = render_poses3d(j3_d, None, cnt_d, cams_d, t_d, dtype=dtype, **rkw)
            two = render_keypoints(j2_d, cnt_bv, v2_d, dtype=dtype, **kw)
            r = {
                "a_host_restatement_upload_render": blocks(host_route(
                    lambda: G.project_batch(joints3d, None, count, cams[None], None, t, ORI, IMAGE), dtype),
                    max(1, args.calls // 4), wall=True),
                "a_vec_host_numpy_upload_render": blocks(host_route(
                    lambda: project_vectorised(joints3d, cams, t, ORI, IMAGE), dtype), args.calls, wall=True),
                "b_render_keypoints": blocks(lambda: render_keypoints(j2_d, cnt_bv, v2_d, dtype=dtype, **kw),
                                             args.calls),
                "c_render_poses3d": blocks(lambda: render_poses3d(j3_d, None, cnt_d, cams_d, t_d, dtype=dtype, **rkw),
                                           args.calls),
                "d_project_then_render": blocks(lambda: render_keypoints(
                    *_swap(project_poses(j3_d, None, cnt_d, cams_d, t_d, **sizes), cnt_bv), dtype=dtype, **kw),
                    args.calls),
            }
            m = {k: v["median_us"] for k, v in r.items()}
            lines.append({
                "bench": "render_gt", "tree": ".", "dtype": str(dtype), "B": B, "V": V, "P": P,
                "J": J, "H": HEATMAP[1], "W": HEATMAP[0], "device": torch.cuda.get_device_name(0), **r,
                "c_minus_b_us": round(m["c_render_poses3d"] - m["b_render_keypoints"], 2),
                "d_over_c": round(m["d_project_then_render"] / m["c_render_poses3d"], 3),
                "a_over_c": round(m["a_host_restatement_upload_render"] / m["c_render_poses3d"], 1),
                "a_vec_over_c": round(m["a_vec_host_numpy_upload_render"] / m["c_render_poses3d"], 1),
                "one_launch_equals_two": bool(torch.equal(one.t, two.t)),
                "device_projection_equals_restatement": same_projection,
                "vectorised_numpy_differs_from_restatement_at": int(np.count_nonzero(vec_j2 != ref_j2)),
                "visible_fraction": round(float(ref_v2.mean()), 3),
                "timing": "HIP events around blocks of calls (b, c, d); host clock around synchronised calls "
                          "(a, a_vec); 3 warm-ups; median and min-max of the blocks' per-call times",
            })
    for line in lines:
        s = json.dumps(line)
        print(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(s + "\n")


def _swap(projected, count_bv):
    """(joints2d, vis2d) -> the positional operands of render_keypoints: (joints, count, vis)."""
    return projected[0], count_bv, projected[1]


if __name__ == "__main__":
    main()
