#!/usr/bin/env python3
"""Golden vectors for fvp_project_poses / fvp_render_poses3d (fvp.heatmaps.render_poses3d).

Runs the 'gt' branch of the reference's own JointsDataset.__getitem__
(lib/dataset/JointsDataset.py:221-259) with data_augmentation = False on the
poses of tests/render_gt_ref.py (make_poses) through the two committed
calibrations, and calls its project_pose_cpu / affine_transform directly to
record the 2-D keypoints and visibility flags the branch computes on the way.
Inputs and outputs go to tests/golden/render_gt.npz (compressed).  Only
recorded data goes into the file.

    python3 -B tools/gen_render_gt_golden.py --reference <reference checkout>

(-B: no __pycache__ in the reference tree.)  The two matrix products of the
branch (np.matmul in project_point_cpu, np.dot in affine_transform) are summed
in the order the BLAS of the generating host picks; the numpy version used is recorded, and
tests/test_render_gt_golden.py pins the order the kernel assumes to these bytes.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "faster-voxelpose_amd"), os.path.join(REPO, "tools")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("FVP_REFERENCE", ""),
                    help="checkout of the reference project (its lib/ is imported)")
    args = ap.parse_args()
    ref_lib = os.path.join(args.reference, "lib")
    if not args.reference or not os.path.isdir(ref_lib):
        print("reference absent: skipped")
        return
    import render_gt_ref as G
    from gen_render_golden import reference_painter

    JointsDataset = reference_painter(ref_lib)  # (stubs cv2 / json_tricks, imports the reference's lib)
    project_pose_cpu = sys.modules["utils.cameras"].project_pose_cpu
    affine_transform = sys.modules["utils.transforms"].affine_transform

    out = {"numpy_version": np.array(np.__version__), "image_size": np.array(G.IMAGE_SIZE),
           "sigma": np.array(G.SIGMA), "n_cases": np.array(len(G.CASES))}
    for c in range(len(G.CASES)):
        case = G.built_case(c)
        name, J, hm = case["calibration"], case["J"], case["heatmap_size"]
        cams = G.camera_dicts(name)
        V = len(cams)
        ds = object.__new__(JointsDataset)
        ds.cameras = {"seq": cams}
        ds.num_views = V
        ds.ori_image_size = np.array(case["ori_image_size"])
        ds.image_size = np.array(G.IMAGE_SIZE)
        ds.heatmap_size = np.array(hm)
        ds.sigma = G.SIGMA
        ds.resize_transform = np.array(case["resize_t"])
        ds.input_heatmap_src = "gt"
        ds.data_augmentation = False
        ds.db = []
        for b in range(G.B):
            n = int(case["count"][b])
            ds.db.append({"target": None, "meta": {"joints_3d": np.array(case["joints3d"][b, :n]),
                                                   "joints_3d_vis": case["vis3d"][b, :n].astype(np.float64),
                                                   "seq": "seq"}})
        maps = np.zeros((G.B, V, J, hm[1], hm[0]), np.float32)
        joints2d = np.zeros((G.B, V, G.P, J, 2), np.float64)
        vis2d = np.zeros((G.B, V, G.P, J), np.uint8)
        for b in range(G.B):
            maps[b] = ds[b][3].numpy()
            meta = ds.db[b]["meta"]
            for v in range(V):  # the keypoints and flags of JointsDataset.py:231-254, from the reference's functions
                for n in range(len(meta["joints_3d"])):
                    pose = project_pose_cpu(meta["joints_3d"][n], cams[v])
                    vis = ((meta["joints_3d_vis"][n] > 0) & (pose[:, 0] >= 0) & (pose[:, 0] <= ds.ori_image_size[0] - 1)
                           & (pose[:, 1] >= 0) & (pose[:, 1] <= ds.ori_image_size[1] - 1))
                    for i in range(J):
                        pose[i] = affine_transform(pose[i], ds.resize_transform)
                        if np.min(pose[i]) < 0 or pose[i, 0] >= ds.image_size[0] or pose[i, 1] >= ds.image_size[1]:
                            vis[i] = False
                    joints2d[b, v, n], vis2d[b, v, n] = pose, vis
        # the recorded flags are the ones the branch painted with: repaint through the reference's painter
        for b in range(G.B):
            n = int(case["count"][b])
            for v in range(V):
                again = ds.generate_input_heatmap([joints2d[b, v, i] for i in range(n)],
                                                  joints_vis=[vis2d[b, v, i] for i in range(n)])
                assert np.array_equal(again, maps[b, v]), (c, b, v)
        for key in ("joints3d", "vis3d", "count", "cams", "resize_t"):
            out[f"c{c}_{key}"] = np.array(case[key])
        out[f"c{c}_calibration"], out[f"c{c}_zoom"] = np.array(name), np.array(case["zoom"])
        out[f"c{c}_heatmap_size"], out[f"c{c}_ori_image_size"] = np.array(hm), np.array(case["ori_image_size"])
        out[f"c{c}_joints2d"], out[f"c{c}_vis2d"], out[f"c{c}_heatmaps"] = joints2d, vis2d, maps
        print(f"case {c}: {name} J {J} heatmap {hm} zoom {case['zoom']}: {int(vis2d.sum())} visible joints, "
              f"{np.count_nonzero(maps)} painted values")
    path = os.path.join(GOLDEN, "render_gt.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, numpy {np.__version__}")


if __name__ == "__main__":
    main()
