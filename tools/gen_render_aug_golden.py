#!/usr/bin/env python3
"""Golden vectors for fvp_render_keypoints_aug / fvp_render_poses3d_aug
(fvp.heatmaps.draw_augmentation, render_keypoints(augment=), render_poses3d(augment=)).

Runs the reference's own JointsDataset.generate_input_heatmap
(lib/dataset/JointsDataset.py:368-447) with data_augmentation = True on the
people of tests/render_ref.py (the four cases of tools/gen_render_golden.py),
seeding random and np.random before every frame-view, and one case through
the 'gt' branch of JointsDataset.__getitem__ (:221-259, reached as
tools/gen_render_gt_golden.py reaches it), seeding before every frame.  Stored
in tests/golden/render_aug.npz (compressed): the inputs, the seeds, the
reference's heatmaps and the next value of each stream after the painter
returned.  Only recorded data goes into the file.

    python3 -B tools/gen_render_aug_golden.py --reference <reference checkout>

Seeds: unit k (a frame-view, or a frame of the 'gt' case) starts at FIRST_SEED + k;
for every condition of CONDITIONS the default seeds leave unmet, seeds 0, 1, 2, ...
are tried on the units in order and the first hit replaces that unit's seed.  Every
condition is asserted on what is recorded.
"""
import argparse
import os
import random
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "faster-voxelpose_amd"), os.path.join(REPO, "tools")):
    sys.path.insert(0, p)

FIRST_SEED = 100
SEARCH = 4000
GT_CASE = 0  # of tests/render_gt_ref.py CASES: Shelf, 17 joints, 48 x 32
CONDITIONS = ("scale_above_1_on_map", "unscaled", "half", "fifth", "rect_cuts", "rect_misses", "br_zero")


def conditions(joints, count, vis, image_size, heatmap_size, sigma, seed):
    """The CONDITIONS one unit meets under `seed`, from the restated draws and windows."""
    import render_aug_ref as A
    import render_ref as R

    W, H = heatmap_size
    scale, rect, detail = A.draw(joints, count, vis, image_size, heatmap_size, sigma, *A.seeded(seed))
    wins = {(v, p, j): (ul, br, n, c0) for v, p, j, ul, br, skipped, n, c0, _ in
            R.windows(joints, count, vis, image_size, heatmap_size, sigma) if not skipped}
    met = set()
    for v, p, j, scaled, second in detail:
        ul, br, n, c0 = wins[(v, p, j)]
        x0, x1 = max(0, ul[0]), min(br[0], W, ul[0] + n)
        y0, y1 = max(0, ul[1]), min(br[1], H, ul[1] + n)
        if br[0] == 0 or br[1] == 0:
            met.add("br_zero")
        if x0 >= x1 or y0 >= y1:
            continue  # paints nothing
        r0, r1, q0, q1 = (int(x) for x in rect[v, p, j])
        rows = (max(r0, y0 - ul[1]), min(r1, y1 - ul[1]))  # the rectangle within the painted part of the patch
        cols = (max(q0, x0 - ul[0]), min(q1, x1 - ul[0]))
        cuts = rows[0] < rows[1] and cols[0] < cols[1]
        met.add("rect_cuts" if cuts else "rect_misses")
        cx, cy = ul[0] + c0, ul[1] + c0
        centre_cut = r0 <= c0 < r1 and q0 <= c0 < q1
        if scale[v, p, j] > 1 and x0 <= cx < x1 and y0 <= cy < y1 and not centre_cut:
            met.add("scale_above_1_on_map")
        if not scaled and second == 1.0:
            met.add("unscaled")
        if second == 0.5:
            met.add("half")
        if second == 0.2:
            assert j in (9, 10)
            met.add("fifth")
    return met


def pick_seeds(units):
    """units: list of (joints, count, vis, image_size, heatmap_size, sigma) -> a seed per unit."""
    seeds = [FIRST_SEED + k for k in range(len(units))]
    met = set().union(*(conditions(*u, s) for u, s in zip(units, seeds)))
    taken = set()
    for cond in CONDITIONS:
        if cond in met:
            continue
        hit = next(((k, s) for s in range(SEARCH) for k, u in enumerate(units)
                    if k not in taken and cond in conditions(*u, s)), None)
        assert hit is not None, f"no seed below {SEARCH} meets {cond}"
        seeds[hit[0]] = hit[1]
        taken.add(hit[0])
        print(f"{cond}: unit {hit[0]} seeded {hit[1]}")
    met = set().union(*(conditions(*u, s) for u, s in zip(units, seeds)))
    assert met == set(CONDITIONS), sorted(set(CONDITIONS) - met)
    return seeds


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("FVP_REFERENCE", ""),
                    help="checkout of the reference project (its lib/ is imported)")
    args = ap.parse_args()
    ref_lib = os.path.join(args.reference, "lib")
    if not args.reference or not os.path.isdir(ref_lib):
        print("reference absent: skipped")
        return
    import render_aug_ref as A
    import render_gt_ref as G
    import render_ref as R
    from gen_render_golden import CASES, reference_painter

    JointsDataset = reference_painter(ref_lib)
    project_pose_cpu = sys.modules["utils.cameras"].project_pose_cpu
    affine_transform = sys.modules["utils.transforms"].affine_transform

    # -- the inputs, and the units that are seeded ------------------------------------------------
    inputs, units, owner = [], [], []
    for c, (J, hm, with_vis, seed) in enumerate(CASES):
        joints, count = R.make_people(seed, J, hm)
        vis = R.make_vis(seed, J) if with_vis else None
        inputs.append(dict(kind="pred", J=J, hm=hm, joints=joints, count=count, vis=vis))
        for b in range(R.B):
            for v in range(R.V):
                units.append((joints[b, v:v + 1], count[b, v:v + 1], None if vis is None else vis[b, v:v + 1],
                              R.IMAGE_SIZE, hm, R.SIGMA))
                owner.append((c, (b, v)))
    gt = G.built_case(GT_CASE)
    cams = G.camera_dicts(gt["calibration"])
    V, J, hm = len(cams), gt["J"], gt["heatmap_size"]
    assert tuple(G.IMAGE_SIZE) == tuple(R.IMAGE_SIZE) and G.SIGMA == R.SIGMA
    ds = object.__new__(JointsDataset)
    ds.cameras = {"seq": cams}
    ds.num_views = V
    ds.ori_image_size = np.array(gt["ori_image_size"])
    ds.image_size = np.array(G.IMAGE_SIZE)
    ds.heatmap_size = np.array(hm)
    ds.sigma = G.SIGMA
    ds.resize_transform = np.array(gt["resize_t"])
    ds.input_heatmap_src = "gt"
    ds.data_augmentation = True
    ds.db = []
    joints2d = np.zeros((G.B, V, G.P, J, 2), np.float64)
    vis2d = np.zeros((G.B, V, G.P, J), np.uint8)
    for b in range(G.B):
        n = int(gt["count"][b])
        meta = {"joints_3d": np.array(gt["joints3d"][b, :n]), "joints_3d_vis": gt["vis3d"][b, :n].astype(np.float64),
                "seq": "seq"}
        ds.db.append({"target": None, "meta": meta})
        for v in range(V):  # the keypoints and flags of JointsDataset.py:231-254, from the reference's functions
            for i in range(n):
                pose = project_pose_cpu(meta["joints_3d"][i], cams[v])
                vis = ((meta["joints_3d_vis"][i] > 0) & (pose[:, 0] >= 0) & (pose[:, 0] <= ds.ori_image_size[0] - 1)
                       & (pose[:, 1] >= 0) & (pose[:, 1] <= ds.ori_image_size[1] - 1))
                for k in range(J):
                    pose[k] = affine_transform(pose[k], ds.resize_transform)
                    if np.min(pose[k]) < 0 or pose[k, 0] >= ds.image_size[0] or pose[k, 1] >= ds.image_size[1]:
                        vis[k] = False
                joints2d[b, v, i], vis2d[b, v, i] = pose, vis
        units.append((joints2d[b], np.repeat(gt["count"][b], V), vis2d[b], G.IMAGE_SIZE, hm, G.SIGMA))
        owner.append((len(CASES), (b,)))
    inputs.append(dict(kind="gt", J=J, hm=hm, joints=joints2d, count=np.array(gt["count"]), vis=vis2d))

    # skipped joints of both kinds are in the inputs whatever the seeds
    n_vis = n_off = 0
    for u in units:
        shown = R.windows(u[0], u[1], u[2], u[3], u[4], u[5])
        n_off += sum(1 for w in shown if w[5])
        if u[2] is not None:
            n_vis += sum(int(np.count_nonzero(u[2][v, :int(u[1][v])] == 0)) for v in range(u[0].shape[0]))
    assert n_vis > 0 and n_off > 0, (n_vis, n_off)
    seeds = pick_seeds(units)

    # -- the reference's painter under those seeds ------------------------------------------------
    out = {"numpy_version": np.array(np.__version__), "image_size": np.array(R.IMAGE_SIZE),
           "sigma": np.array(R.SIGMA), "n_cases": np.array(len(inputs))}
    maps = [np.zeros(i["joints"].shape[:2] + (i["J"], i["hm"][1], i["hm"][0]), np.float32) for i in inputs]
    nxt = [np.zeros((R.B, R.V, 2) if i["kind"] == "pred" else (G.B, 2), np.float64) for i in inputs]
    sds = [np.zeros((R.B, R.V) if i["kind"] == "pred" else (G.B,), np.int64) for i in inputs]
    painter = object.__new__(JointsDataset)
    painter.image_size = np.array(R.IMAGE_SIZE)
    painter.sigma = R.SIGMA
    painter.data_augmentation = True
    largest = 0.0
    for (c, idx), unit, seed in zip(owner, units, seeds):
        random.seed(seed)
        np.random.seed(seed)
        if inputs[c]["kind"] == "gt":
            maps[c][idx[0]] = ds[idx[0]][3].numpy()
        else:
            painter.heatmap_size = np.array(inputs[c]["hm"])
            n = int(unit[1][0])
            people = [unit[0][0, p] for p in range(n)]
            people_vis = None if unit[2] is None else [unit[2][0, p] for p in range(n)]
            maps[c][idx] = painter.generate_input_heatmap(people, people_vis)
        nxt[c][idx] = (random.random(), np.random.uniform())
        sds[c][idx] = seed
        # the restated draws consumed what the reference consumed, and its heatmaps have their support
        rngs = A.seeded(seed)
        scale, rect, _ = A.draw(*unit, *rngs)
        assert np.array_equal(A.next_values(*rngs), nxt[c][idx]), (c, idx)
        mine = A.render_frame(unit[0], unit[1], unit[2], scale, rect, unit[3], unit[4], unit[5])
        theirs = maps[c][idx] if inputs[c]["kind"] == "gt" else maps[c][idx][None]
        assert np.array_equal(mine != 0, theirs != 0), (c, idx)
        largest = max(largest, float(scale.max()))
    assert 1.0 < largest < A.MAX_SCALE, largest
    for c, i in enumerate(inputs):
        out[f"c{c}_kind"], out[f"c{c}_heatmap_size"] = np.array(i["kind"]), np.array(i["hm"])
        out[f"c{c}_joints"], out[f"c{c}_count"], out[f"c{c}_heatmaps"] = i["joints"], i["count"], maps[c]
        out[f"c{c}_seeds"], out[f"c{c}_next"] = sds[c], nxt[c]
        if i["vis"] is not None:
            out[f"c{c}_vis"] = i["vis"]
        if i["kind"] == "gt":
            out[f"c{c}_gt_case"] = np.array(GT_CASE)
        print(f"case {c}: {i['kind']} J {i['J']} heatmap {i['hm']}: {np.count_nonzero(maps[c])} painted values, "
              f"{int(np.count_nonzero(maps[c] == 1.0))} at exactly 1, max {maps[c].max():.6f}")
    path = os.path.join(GOLDEN, "render_aug.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, numpy {np.__version__}, largest scale {largest:.4f}")


if __name__ == "__main__":
    main()
