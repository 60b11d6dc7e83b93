#!/usr/bin/env python3
"""Golden vectors for fvp_render_keypoints (fvp.heatmaps.render_keypoints).

Runs the reference's own JointsDataset.generate_input_heatmap
(lib/dataset/JointsDataset.py:368-447) with data_augmentation = False on the
people of tests/render_ref.py (make_people / make_vis) and stores inputs and
outputs in tests/golden/render_kp.npz (compressed).  Only recorded data goes
into the file.

    python3 -B tools/gen_render_golden.py --reference <reference checkout>

(-B: no __pycache__ in the reference tree.)  The reference computes the
patch in fp64 under numpy >= 2 (NEP 50: float32 array - float64 scalar) and
in fp32 before; the numpy version used is recorded.
"""
import argparse
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tests"))

# (J, heatmap (W, H), with vis, seed): both tile-odd shapes, both channel paddings
CASES = [(17, (48, 32), False, 1), (15, (50, 37), False, 2), (17, (50, 37), True, 3), (15, (48, 32), True, 4)]


def reference_painter(ref_lib):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))  # only get_affine_transform uses it
    jt = types.ModuleType("json_tricks")  # absent here; reads plain JSON like the standard module
    jt.load, jt.loads, jt.dump, jt.dumps = json.load, json.loads, json.dump, json.dumps
    sys.modules.setdefault("json_tricks", jt)
    sys.path.insert(0, ref_lib)
    import dataset  # noqa: F401  (dataset/__init__.py imports the dataset modules)

    return sys.modules["dataset.JointsDataset"].JointsDataset


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("FVP_REFERENCE", ""),
                    help="checkout of the reference project (its lib/ is imported)")
    args = ap.parse_args()
    ref_lib = os.path.join(args.reference, "lib")
    if not args.reference or not os.path.isdir(ref_lib):
        print("reference absent: skipped")
        return
    import render_ref as R

    JointsDataset = reference_painter(ref_lib)
    out = {"numpy_version": np.array(np.__version__), "image_size": np.array(R.IMAGE_SIZE),
           "sigma": np.array(R.SIGMA), "n_cases": np.array(len(CASES))}
    for c, (J, hm, with_vis, seed) in enumerate(CASES):
        ds = object.__new__(JointsDataset)
        ds.heatmap_size = np.array(hm)
        ds.image_size = np.array(R.IMAGE_SIZE)
        ds.sigma = R.SIGMA
        ds.data_augmentation = False
        joints, count = R.make_people(seed, J, hm)
        vis = R.make_vis(seed, J) if with_vis else None
        maps = np.zeros((R.B, R.V, J, hm[1], hm[0]), np.float32)
        for b in range(R.B):
            for v in range(R.V):
                n = int(count[b, v])
                if n == 0:  # (the reference indexes joints[0]: no people, no call)
                    continue
                people = [joints[b, v, p] for p in range(n)]
                people_vis = None if vis is None else [vis[b, v, p] for p in range(n)]
                maps[b, v] = ds.generate_input_heatmap(people, people_vis)
        out[f"c{c}_heatmap_size"] = np.array(hm)
        out[f"c{c}_joints"], out[f"c{c}_count"], out[f"c{c}_heatmaps"] = joints, count, maps
        if vis is not None:
            out[f"c{c}_vis"] = vis
        print(f"case {c}: J {J} heatmap {hm} vis {with_vis}: {np.count_nonzero(maps)} painted values, "
              f"min {maps[maps > 0].min():.3g}")
    path = os.path.join(GOLDEN, "render_kp.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, numpy {np.__version__}")


if __name__ == "__main__":
    main()
