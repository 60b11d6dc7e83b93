"""Inputs shared by tests/test_evaluate_host.py and tests/test_gpu_evaluate.py:
the cases of tests/golden/evaluate.npz (tools/gen_evaluate_golden.py) and a
seeded sweep whose reference is tests/eval_ref.py."""
import os

import numpy as np

import eval_ref as E
from conftest import GOLDEN

PANOPTIC_CASES = ("panoptic", "panoptic_empty")
ACTOR_CASES = tuple(f"{d}{s}" for d in ("shelf", "campus") for s in ("", "_limbs0", "_limbs1", "_limbs2", "_limbs3"))

# Panoptic sweep (K, G, J) at N = 3 -- K * G = 130 exceeds the kernel's block of 128 -- and one run across N = 2,049
PANOPTIC_SWEEP = [(K, G, J) for K in (1, 10, 13) for G in (1, 4, 10) for J in (1, 15, 17)]
ACTOR_SWEEP = [(K, A, c) for K in (1, 10, 13) for A in (1, 4) for c in (E.SHELF, E.CAMPUS)]

_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(os.path.join(GOLDEN, "evaluate.npz")) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def panoptic_golden(name):
    g = golden()
    return tuple(g[f"{name}_{k}"] for k in ("preds", "joints_3d", "joints_3d_vis", "num_person"))


def actor_golden(name):
    g = golden()
    return g[f"{name}_preds"], g[f"{name}_gt"], g[f"{name}_present"].astype(bool), int(g[f"{name}_convert"])


def records(name, keys):
    g = golden()
    return {k: g[f"{name}_rec_{k}"] for k in keys}


def db_of(joints, vis, count):
    """A Panoptic db: what Panoptic.evaluate and PanopticGroundTruth.from_db read of it."""
    return [{"meta": {"num_person": int(count[i]), "joints_3d": joints[i], "joints_3d_vis": vis[i]}}
            for i in range(len(count))]


def actor3d_of(name):
    """The object array [A][F] (metres; 1 x 0 where absent) the golden's actorsGT.mat held."""
    g = golden()
    dense, there = g[f"{name}_actor3d"], g[f"{name}_actor3d_present"]
    cells = np.empty(there.shape, dtype=object)
    for a in range(there.shape[0]):
        for f in range(there.shape[1]):
            cells[a, f] = dense[a, f] if there[a, f] else np.zeros((1, 0))
    return cells


def write_actors_mat(path, cells):
    """actorsGT.mat with MATLAB's nesting {1x1}{A x 1}{F x 1}, as the datasets ship it."""
    import scipy.io as scio

    A, F = cells.shape
    per_actor = np.empty((A, 1), dtype=object)
    for a in range(A):
        col = np.empty((F, 1), dtype=object)
        for f in range(F):
            col[f, 0] = cells[a, f]
        per_actor[a, 0] = col
    outer = np.empty((1, 1), dtype=object)
    outer[0, 0] = per_actor
    scio.savemat(path, {"actor3D": outer})


def random_panoptic(seed, N, K, G, J, C=6):
    """preds [N, K, J, C], joints_3d, joints_3d_vis, num_person: valid and invalid slots (a NaN flag
    among them), frames without people, hidden joints and people, a repeated person, NaN coordinates."""
    rng = np.random.default_rng(seed)
    count = rng.integers(0, G + 1, N)
    count[0] = G
    joints = rng.uniform(-2000.0, 2000.0, (N, G, 1, 3)) + rng.normal(0.0, 300.0, (N, G, J, 3))
    vis = (rng.random((N, G, J)) > 0.2).astype(np.float64)
    vis[rng.random((N, G)) < 0.05] = 0.0
    if G > 1:
        joints[0, 1], vis[0, 1] = joints[0, 0], vis[0, 0]
    preds = np.zeros((N, K, J, C), np.float32)
    pick = rng.integers(0, G, (N, K))
    preds[..., :3] = joints[np.arange(N)[:, None], pick] + rng.normal(0.0, 1.0, (N, K, 1, 1)) * rng.normal(
        0.0, 80.0, (N, K, J, 3))
    flag = np.where(rng.random((N, K)) < 0.3, -1.0, rng.random((N, K))).astype(np.float32)
    flag[rng.random((N, K)) < 0.03] = np.nan
    preds[..., 3] = flag[:, :, None]
    preds[..., 4] = rng.random((N, K), np.float32)[:, :, None]
    if C > 5:
        preds[..., 5:] = 7.0
    bad = rng.random((N, K)) < 0.03
    preds[bad, J // 2, 1] = np.nan
    return preds, joints, vis, count.astype(np.int32)


def random_actors(seed, N, K, A, convert, C=6):
    """preds [N, K, 17, C], gt [N, A, 14, 3], present [N, A].  Shelf: every frame keeps a
    valid prediction (it raises on none); Campus: frame 1 has none."""
    rng = np.random.default_rng(seed)
    truth = rng.uniform(-2000.0, 2000.0, (N, A, 1, 3)) + rng.normal(0.0, 250.0, (N, A, 17, 3))
    gt = np.stack([[E.convert_pose(truth[i, a].astype(np.float32), convert) for a in range(A)] for i in range(N)])
    gt = gt + rng.normal(0.0, 20.0, gt.shape)
    present = rng.random((N, A)) > 0.3
    present[0, 0] = True
    preds = np.zeros((N, K, 17, C), np.float32)
    pick = rng.integers(0, A, (N, K))
    preds[..., :3] = truth[np.arange(N)[:, None], pick] + rng.normal(0.0, 1.0, (N, K, 1, 1)) * rng.normal(
        0.0, 120.0, (N, K, 17, 3))
    flag = np.where(rng.random((N, K)) < 0.3, -1.0, 0.0).astype(np.float32)
    flag[rng.random((N, K)) < 0.05] = np.nan
    flag[:, 0] = 0.5
    if convert == E.CAMPUS and N > 1:
        flag[1] = -1.0
    preds[..., 3] = flag[:, :, None]
    preds[..., 4] = rng.random((N, K), np.float32)[:, :, None]
    if K > 2:
        preds[0, 2] = preds[0, 0]
        preds[N - 1, 1, 9, 0] = np.nan
    if C > 5:
        preds[..., 5:] = 7.0
    return preds, gt, present
