#!/usr/bin/env python3
"""Golden vectors for fvp.evaluate (csrc/fvp_eval.hip: fvp_match_poses / fvp_match_actors).

Runs the reference's own Panoptic.evaluate, Shelf.evaluate and Campus.evaluate
(lib/dataset/panoptic.py:214-312, shelf.py:162-256, campus.py:138-230) on small
synthetic runs and stores inputs and results in tests/golden/evaluate.npz:
the inputs, the reference's (metric, msg), Panoptic's eval_list as the
reference built it (before its first sort), the records of tests/eval_ref.py,
and the numpy version.  Only recorded data goes into the file.

    python3 -B tools/gen_evaluate_golden.py --reference <reference checkout>

The dataset objects are object.__new__(cls) stubs carrying only what evaluate
reads: db / db_size for Panoptic; dataset_dir with a temporary actorsGT.mat
(scipy.io.savemat) and frame_range for Shelf and Campus.

Two assertions on every case: tests/eval_ref.py returns the reference's
(metric, msg); and every discrete decision -- an MPJPE against 25...150 and
500, each PCP left side against its right side, best against second best in
every argmin that is not an exact tie -- has a relative margin of at least
1e-9, so that a last-bit difference in a distance (np.linalg.norm goes through
BLAS) cannot flip a count.  A case that misses the margin is drawn again.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

MARGIN = 1e-9
THRESHOLDS = (25, 50, 75, 100, 125, 150, 500)


# -- inputs ------------------------------------------------------------------------------

def _people(rng, n, J):
    root = rng.uniform(-2000.0, 2000.0, (n, 1, 3))
    return root + rng.normal(0.0, 300.0, (n, J, 3))


def _near(rng, pose, sigma):
    return (pose + rng.normal(0.0, sigma, pose.shape)).astype(np.float32)


def panoptic_case(seed, empty=False):
    """N frames [K, J, 5] against up to G people; the frames of the issue's list, in order."""
    rng = np.random.default_rng(seed)
    N, K, G, J = (2, 3, 3, 15) if empty else (7, 6, 4, 15)
    joints = np.zeros((N, G, J, 3))
    vis = np.zeros((N, G, J))
    count = np.array([2, 1] if empty else [0, 2, 3, 3, 2, 4, 3])
    preds = np.zeros((N, K, J, 5), np.float32)
    preds[:, :, :, 3] = -1.0
    for i in range(N):
        joints[i, :count[i]] = _people(rng, count[i], J)
        vis[i, :count[i]] = rng.random((count[i], J)) > 0.2
        joints[i, count[i]:] = rng.normal(0.0, 1000.0, (G - count[i], J, 3))  # padding rows: never read
    if empty:
        preds[:, :, :, :3] = rng.normal(0.0, 1000.0, (N, K, J, 3))
        return preds, joints, vis, count
    sigmas = (8.0, 20.0, 35.0, 60.0, 90.0, 400.0)
    for i in range(N):
        for k in range(K):
            g = int(rng.integers(0, max(count[i], 1)))
            preds[i, k, :, :3] = _near(rng, joints[i, g] if count[i] else _people(rng, 1, J)[0], sigmas[(i + k) % 6])
            preds[i, k, :, 3] = 0.0 if rng.random() > 0.25 else -1.0
            preds[i, k, :, 4] = np.float32(rng.random())
    preds[0, :, :, 3] = 0.0      # frame 0: no people, valid predictions -> ignored
    preds[1, :, :, 3] = -1.0     # frame 1: people, no valid prediction
    vis[2, 1] = 0.0              # frame 2: a person with no visible joint -> NaN, which argmin takes
    preds[2, :3, :, 3] = 0.0
    joints[3, 1], vis[3, 1] = joints[3, 0], vis[3, 0]  # frame 3: two identical people -> the first wins
    preds[3, 0, :, :3], preds[3, 0, :, 3] = _near(rng, joints[3, 0], 15.0), 0.0
    preds[3, 1, :, :3], preds[3, 1, :, 3] = _near(rng, joints[3, 1], 30.0), 0.0
    preds[4, :, :, 3] = 0.0      # frames 4 and 5: equal scores -> the stable order decides
    preds[4, :, :, 4] = np.float32(0.5)
    preds[5, :2, :, 4] = np.float32(0.5)
    preds[5, :3, :, 3] = 0.0
    preds[5, 2, 4, 1] = np.nan   # frame 5: a NaN coordinate
    preds[6, 1, :, 3] = np.nan   # frame 6: a NaN valid flag -> not valid
    preds[6, 0, :, 3] = 0.0
    return preds, joints, vis, count


def _coco(rng, n):
    """n plausible 17-joint poses (mm): limbs a few hundred mm long."""
    root = rng.uniform(-2000.0, 2000.0, (n, 1, 3))
    return root + rng.normal(0.0, 250.0, (n, 17, 3))


def actor_case(seed, convert, limb_case=None):
    """(preds [N, K, 17, 5], actor_3d cells [A][F] in metres, frame_range, gt, present)."""
    import eval_ref as E

    rng = np.random.default_rng(seed)
    if limb_case is None:
        N, K, A, F, first = 5, 5, 4, 9, 3
    else:
        N, K, A, F, first = 1, 2, 3, 2, 1
    frame_range = list(range(first, first + N))
    present = rng.random((F, A)) > 0.3
    present[:, 3 if A > 3 else 2] = rng.random(F) > 0.7
    truth = _coco(rng, F * A).reshape(F, A, 17, 3)
    cells = np.empty((A, F), dtype=object)
    for a in range(A):
        for f in range(F):
            pose = E.convert_pose(truth[f, a].astype(np.float32), convert) / 1000.0
            cells[a, f] = pose if present[f, a] else np.zeros((1, 0))
    preds = np.zeros((N, K, 17, 5), np.float32)
    preds[:, :, :, 3] = -1.0
    sigmas = (15.0, 60.0, 110.0, 160.0, 450.0)
    for i, fi in enumerate(frame_range):
        for k in range(K):
            a = int(rng.integers(0, A))
            preds[i, k, :, :3] = _near(rng, truth[fi, a], sigmas[(i + k) % 5])
            preds[i, k, :, 3] = 0.0 if rng.random() > 0.3 else -1.0
            preds[i, k, :, 4] = np.float32(rng.random())
        preds[i, 0, :, 3] = 0.0
    if limb_case is None:
        preds[1, 2], preds[1, 2, :, 3] = preds[1, 0], 0.0   # two identical predictions -> the first wins
        preds[2, 1, :, 3] = 0.0
        preds[2, 1, 7, 2] = np.nan                          # a NaN coordinate -> a NaN mean, which argmin takes
        if convert == E.CAMPUS:
            preds[3, :, :, 3] = -1.0                        # no valid prediction: Campus skips the frame
    else:
        # one present actor, one close prediction with a few joints pushed off: the PCP shows which parts fail
        present[:, :] = False
        present[frame_range[0], 0] = True
        for a in range(A):
            for f in range(F):
                if not present[f, a]:
                    cells[a, f] = np.zeros((1, 0))
                else:
                    cells[a, f] = E.convert_pose(truth[f, a].astype(np.float32), convert) / 1000.0
        preds[0, 0, :, :3] = _near(rng, truth[frame_range[0], 0], 5.0)
        preds[0, 0, list(limb_case), :3] += np.float32(700.0)
        preds[0, 1, :, 3] = -1.0
    gt = np.zeros((N, A, 14, 3))
    pres = np.zeros((N, A), bool)
    for i, fi in enumerate(frame_range):
        for a in range(A):
            value = cells[a, fi] * 1000.0
            if len(value[0]) != 0:
                gt[i, a], pres[i, a] = value, True
    return preds, cells, frame_range, gt, pres


# -- the margin condition ----------------------------------------------------------------

def _gap(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def _argmin_margin(values):
    v = np.sort(np.asarray(values, np.float64)[~np.isnan(values)])
    return len(v) < 2 or v[1] == v[0] or _gap(v[0], v[1]) >= MARGIN  # an exact tie is one by construction


def panoptic_margins(preds, joints, vis, count):
    ok = True
    with np.errstate(invalid="ignore"):
        for i in range(len(preds)):
            for k in np.nonzero(preds[i, :, 0, 3] >= 0)[0] if count[i] else []:
                per_gt = []
                for g in range(count[i]):
                    v = vis[i, g] > 0.1
                    d = preds[i, k][v, :3] - joints[i, g][v]
                    per_gt.append(np.sqrt((d * d).sum(-1)).mean() if v.any() else np.nan)
                ok &= _argmin_margin(per_gt)
                if not np.isnan(per_gt).any():
                    ok &= all(_gap(min(per_gt), t) >= MARGIN for t in THRESHOLDS)
    return bool(ok)


def actor_margins(preds, gt, present, convert):
    import eval_ref as E

    ok = True
    with np.errstate(invalid="ignore"):
        for i in range(len(preds)):
            slots = np.nonzero(preds[i, :, 0, 3] >= 0)[0]
            if len(slots) == 0:
                continue
            poses = np.stack([E.convert_pose(preds[i, k, :, :3], convert) for k in slots])
            for a in np.nonzero(present[i])[0]:
                d = gt[i, a][None] - poses
                means = np.sqrt((d * d).sum(-1)).mean(-1)
                ok &= _argmin_margin(means)
                if np.isnan(means).any():
                    continue
                ok &= _gap(means.min(), 500.0) >= MARGIN
                for left, right in E.part_sides(poses[int(np.argmin(means))], gt[i, a]):
                    ok &= _gap(left, right) >= MARGIN
    return bool(ok)


# -- the reference's own methods ---------------------------------------------------------

def reference_panoptic(Panoptic, preds, joints, vis, count):
    import torch

    ds = object.__new__(Panoptic)
    ds.db = [{"meta": {"num_person": int(count[i]), "joints_3d": joints[i], "joints_3d_vis": vis[i]}}
             for i in range(len(count))]
    ds.db_size = len(ds.db)
    recorded = []

    def recording_ap(eval_list, total_gt, threshold):
        if not recorded:  # the list as evaluate built it, before the first in-place sort
            recorded.append([(e["mpjpe"], e["score"], e["gt_id"]) for e in eval_list])
        return Panoptic._eval_list_to_ap(eval_list, total_gt, threshold)

    ds._eval_list_to_ap = recording_ap
    import warnings

    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        metric, msg = ds.evaluate(torch.from_numpy(preds))
    return float(metric), msg, np.array(recorded[0], np.float64).reshape(-1, 3)


def reference_actors(cls, preds, cells, frame_range):
    import scipy.io as scio
    import torch

    A, F = cells.shape
    per_actor = np.empty((A, 1), dtype=object)
    for a in range(A):
        col = np.empty((F, 1), dtype=object)
        for f in range(F):
            col[f, 0] = cells[a, f]  # an absent actor's cell: 1 x 0, so len(gt[0]) == 0
        per_actor[a, 0] = col
    outer = np.empty((1, 1), dtype=object)
    outer[0, 0] = per_actor
    with tempfile.TemporaryDirectory() as tmp:
        scio.savemat(os.path.join(tmp, "actorsGT.mat"), {"actor3D": outer})
        ds = object.__new__(cls)
        ds.dataset_dir, ds.frame_range = tmp, list(frame_range)
        with np.errstate(invalid="ignore"):
            metric, msg = ds.evaluate(torch.from_numpy(preds))
        from fvp.integration import load_actor3d

        loaded = load_actor3d(os.path.join(tmp, "actorsGT.mat"))
    assert loaded.shape == cells.shape and all(
        np.array_equal(loaded[a, f].reshape(cells[a, f].shape), cells[a, f]) for a in range(A) for f in range(F)), \
        "fvp.integration.load_actor3d reads the file differently"
    return float(metric), msg


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("FVP_REFERENCE", ""),
                    help="checkout of the reference project (its lib/ is imported)")
    args = ap.parse_args()
    ref_lib = os.path.join(args.reference, "lib")
    if not args.reference or not os.path.isdir(ref_lib):
        print("reference absent: skipped")
        return
    sys.path.insert(0, os.path.join(REPO, "faster-voxelpose_amd"))
    import eval_ref as E
    from gen_render_golden import reference_painter

    reference_painter(ref_lib)  # the stub loader: imports the reference's dataset package
    Panoptic = sys.modules["dataset.panoptic"].Panoptic
    Shelf, Campus = sys.modules["dataset.shelf"].Shelf, sys.modules["dataset.campus"].Campus

    out = {"numpy_version": np.array(np.__version__)}
    names = []

    def draw(make, margins, seed):
        for attempt in range(20):
            case = make(seed + 1000 * attempt)
            if margins(case):
                return case
            print(f"  seed {seed + 1000 * attempt}: a decision within {MARGIN:g} relative; drawn again")
        raise SystemExit("no draw met the margin condition")

    for name, empty, seed in (("panoptic", False, 11), ("panoptic_empty", True, 12)):
        preds, joints, vis, count = draw(lambda s: panoptic_case(s, empty), lambda c: panoptic_margins(*c), seed)
        metric, msg, eval_list = reference_panoptic(Panoptic, preds, joints, vis, count)
        m2, msg2, items, rec = E.panoptic(preds, joints, vis, count)
        assert (float(m2), msg2) == (metric, msg), (name, m2, metric, msg2, msg)
        assert np.array_equal(np.array(items, np.float64).reshape(-1, 3), eval_list, equal_nan=True), name
        out.update({f"{name}_preds": preds, f"{name}_joints_3d": joints, f"{name}_joints_3d_vis": vis,
                    f"{name}_num_person": count.astype(np.int32), f"{name}_metric": np.array(metric),
                    f"{name}_msg": np.array(msg), f"{name}_eval_list": eval_list,
                    **{f"{name}_rec_{k}": v for k, v in rec.items()}})
        names.append(name)
        print(f"{name}: {len(eval_list)} records, metric {metric:.6f}\n  {msg!r}")

    limb_cases = ((1, 10), (5, 6, 3), (11, 12, 0), ())
    for cname, cls, convert in (("shelf", Shelf, E.SHELF), ("campus", Campus, E.CAMPUS)):
        for name, limb, seed in [(cname, None, 21 + convert)] + [
                (f"{cname}_limbs{n}", limb, 31 + 10 * convert + n) for n, limb in enumerate(limb_cases)]:
            preds, cells, frame_range, gt, present = draw(
                lambda s: actor_case(s, convert, limb), lambda c: actor_margins(c[0], c[3], c[4], convert), seed)
            metric, msg = reference_actors(cls, preds, cells, frame_range)
            m2, msg2, rec = E.pcp(preds, gt, present, convert)
            assert (float(m2), msg2) == (metric, msg), (name, m2, metric, msg2, msg)
            there = np.array([[len(cells[a, f][0]) != 0 for f in range(cells.shape[1])] for a in range(len(cells))])
            dense = np.array([[cells[a, f] if there[a, f] else np.zeros((14, 3)) for f in range(cells.shape[1])]
                              for a in range(len(cells))])
            out.update({f"{name}_preds": preds, f"{name}_gt": gt, f"{name}_present": present.astype(np.uint8),
                        f"{name}_actor3d": dense, f"{name}_actor3d_present": there.astype(np.uint8),  # the .mat, metres
                        f"{name}_frame_range": np.array(frame_range), f"{name}_convert": np.array(convert),
                        f"{name}_metric": np.array(metric), f"{name}_msg": np.array(msg),
                        **{f"{name}_rec_{k}": v for k, v in rec.items()}})
            names.append(name)
            print(f"{name}: metric {metric:.6f} parts {[f'{int(b):010b}' for b in rec['parts'].ravel()]}\n  {msg!r}")
    out["names"] = np.array(names)
    path = os.path.join(GOLDEN, "evaluate.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, numpy {np.__version__}")


if __name__ == "__main__":
    main()
