"""The voxelize gather's case table: for every class of every place where the
launcher or the kernel decides ("Voxelize gather routes"), the
cheapest shape of a candidate list that reaches it -- found with the plan query
(fvp.ops.voxelize_plan, host only) and classified with the model of the rules
(voxelize_plan_model.py).  Coverage is the full product WITHIN a place, not
across places.  test_voxelize_cases.py checks the table on the CPU,
test_gpu_voxelize_routes.py runs it bit for bit against the oracle.
"""
import collections
import functools
import itertools

import voxelize_plan_model as M
from fvp import ops

Case = collections.namedtuple("Case", "place cls kind otf B V J bins hm gi want")  # hm = (W, H); want: "both" | "cube" | "xy"
HM = (64, 48)

# (X, Y, Z): the witnesses of the rules' corners first, then fillers
SHAPES = [(32, 128, 1), (63, 66, 1), (72, 60, 3), (17, 256, 1), (100, 63, 5), (128, 34, 7), (19, 27, 20), (65, 64, 2),
          (64, 64, 1), (64, 64, 4), (80, 80, 2), (72, 65, 5), (43, 128, 2), (12, 10, 6), (10, 9, 4), (7, 5, 3),
          (20, 20, 8), (24, 20, 12), (13, 11, 7), (64, 68, 3), (66, 64, 16), (33, 128, 32), (16, 256, 4), (40, 40, 20),
          (9, 7, 33), (5, 3, 300), (11, 13, 64), (64, 64, 20), (48, 96, 8), (17, 250, 2), (96, 66, 2), (65, 65, 1), (128, 288, 2)]


def cp_of(kind, J):
    return 0 if kind.startswith("planar") else (J + 15) // 16 * 16   # (fvp.heatmaps.to_channels_last)


def plan_of(c, aligned=True):
    st, recs = ops.voxelize_plan(c.kind, c.otf, c.B, c.V, c.J, c.hm[1], c.hm[0], *c.bins, cp=cp_of(c.kind, c.J),
                                 grid_index=c.gi, cube_aligned=aligned)
    assert st == 0, (c, st)
    return recs


def classes_of(c):
    """(branch, snap) per record of the case's plan, from the model (which the sweep holds equal to the query)."""
    out = []
    M.plan(c.kind, c.otf, c.B, c.V, c.J, c.hm[1], c.hm[0], *c.bins, cp_of(c.kind, c.J), c.gi, True, classes=out)
    return out


def cost(c):
    return c.bins[0] * c.bins[1] * c.bins[2] * c.B


def inst_of(r):
    return (r.family, r.lpv, r.pair, r.casc, r.nf)


def cfg_class(c):
    r, (branch, snap) = plan_of(c)[0], classes_of(c)[0]
    return (r.lpv, c.otf, branch, snap, M.band_class(r.cols, r.band, c.bins[0], c.bins[1]))


def stage_class(c):
    r = plan_of(c)[0]
    T = r.cols * c.bins[2]
    pitch = "tight" if r.sp == T else "pad1" if r.sp == T + 1 else "pad4"
    return (pitch, bool(r.vec_full), bool(r.vec_last), min(r.passes, 3), T % (256 // r.lpv) != 0)


def _cheapest(cands, key):
    best = {}
    for c in cands:
        k = key(c)
        if k not in best or cost(c) < cost(best[k]):
            best[k] = c
    return best


@functools.lru_cache(None)
def build():
    cases = []
    # 1. instantiation: all 40, each with a full and with a ragged last block
    small = [(8, 8, 8), (12, 10, 6), (10, 9, 4), (7, 5, 3), (13, 11, 7), (11, 7, 5), (8, 8, 1)]
    todo = [("planar_f32", J, B) for J in (4, 8, 15, 32) for B in (1,)]
    todo += [("planar_f16", 15, B) for B in (4, 2, 1)] + [("cl_f16", J, 1) for J in (8, 16, 32)]
    for (kind, J, B), otf, V in itertools.product(todo, (False, True), (5, 17)):
        found = {}
        for bins in small:
            c = Case("inst", None, kind, otf, B, V, J, bins, HM, False, "both")
            r = plan_of(c)[0]
            found.setdefault((inst_of(r), r.last_cols == r.cols), c)
        for (inst, full), c in sorted(found.items()):
            cases.append(c._replace(cls=inst + ("full" if full else "ragged",)))
    # 2. gather_cfg: branch x snap x band, at LPV 1 and 8 (channels-last fp32, J = 4 / 32), both coordinate sources
    cands = [Case("cfg", None, "cl_f32", otf, B, 5, J, bins, HM, False, "both")
             for otf, J, bins, B in itertools.product((False, True), (4, 32), SHAPES, (1, 4, 16, 64))
             if bins[0] * bins[1] * bins[2] * B <= 600000]
    for k, c in sorted(_cheapest(cands, cfg_class).items(), key=str):
        cases.append(c._replace(cls=k))
    # 3. stage and epilogue: pitch x vector epilogue (full, last) x passes x partial last pass, at LPV 4 and 8 (fp32) and 2 and 4 (fp16 in place)
    cands = [Case("stage", None, kind, False, B, 5, J, bins, HM, False, "both")
             for kind, J, bins, B in itertools.product(("cl_f32", "cl_f16"), (15, 32), SHAPES, (1, 16, 64))
             if bins[0] * bins[1] * bins[2] * B <= 600000]
    for k, c in sorted(_cheapest(cands, stage_class).items(), key=str):
        cases.append(c._replace(cls=k))
    for want in ("cube", "xy"):
        for kind in M.KINDS:
            cases.append(Case("stage", ("only", want, kind), kind, kind == "cl_f16", 2, 5, 15, (13, 11, 7), HM, False, want))
    # 4. frames: the pair table's groupings, grid_index forcing NF = 1, and calls of more than one chunk
    for B, gi, groups in [(7, False, (4, 2, 1)), (5, False, (4, 1)), (3, False, (2, 1)), (3, True, (1,))]:
        for otf in (False, True):
            cases.append(Case("frames", ("groups",) + groups + (gi,), "planar_f16", otf, B, 5, 15, (12, 10, 6), HM, gi,
                              "both"))
    cases.append(Case("frames", ("chunks", "f32", (2, 2, 1)), "planar_f32", False, 5, 16, 17, (10, 9, 4), (192, 128),
                      False, "both"))
    cases.append(Case("frames", ("chunks", "pairs", (4, 4, 1)), "planar_f16", True, 9, 16, 5, (10, 9, 4), (255, 128),
                      False, "both"))
    cases.append(Case("frames", ("chunks", "pairs bumped", (4, 4)), "planar_f16", False, 8, 16, 5, (10, 9, 4),
                      (383, 128), False, "both"))
    # the pair table at one frame per entry in several chunks (grid_index given: chunks of 4, 4, 1 frames)
    cases.append(Case("frames", ("chunks", "pairs one frame", (4, 4, 1)), "planar_f16", False, 9, 16, 5, (10, 9, 4),
                      (255, 128), True, "both"))
    # a pair-table frame above 64 MB (16 cameras of 256 x 257, one joint): the budget holds one, four do not fit
    # the cache either, so the batch runs at one frame per entry in chunks of one frame
    cases.append(Case("frames", ("chunks", "pairs big frame", (1, 1, 1)), "planar_f16", True, 3, 16, 1, (10, 9, 4),
                      (257, 256), False, "both"))
    # 33 joints in several chunks: the 32-joint slice one 63 MB frame at a time, then the 1-joint slice's nine
    # frames of 7.9 MB in one chunk -- more than the first slice's chunk, which is what sizes the workspace
    cases.append(Case("frames", ("chunks", "f32 sliced", (1,) * 9 + (9,)), "planar_f32", False, 9, 16, 33, (10, 9, 4),
                      (241, 128), False, "both"))
    # 5. joint slices: the last slice at another LPV than the first, every entry kind, both coordinate sources
    for kind, J, otf in itertools.product(M.KINDS, (33, 40), (False, True)):
        cases.append(Case("slices", (kind, J, otf), kind, otf, 2, 5, J, (10, 9, 4), HM, False, "both"))
    # 6. cameras: odd / even, not a multiple of 2 * LPV, around the 16-camera blocks, three complete blocks (parked sums)
    for kind, J, V, otf in itertools.product(("planar_f32", "cl_f16"), (15,), (3, 6, 16, 17, 32, 33, 48), (False, True)):
        cases.append(Case("cams", (kind, V, otf), kind, otf, 1, V, J, (10, 9, 4), HM, False, "both"))
    return tuple(cases)


@functools.lru_cache(None)
def cameras(V, two):
    """The camera sets of the cases: V cameras of a ring of max(V, 5) + 1 as sequence "a", and -- for the cases
    with a grid_index -- the ring's next V as sequence "b"."""
    from fvp.workloads import ring_cameras

    cams, seq = ring_cameras(max(V, 5) + 1)
    ring = cams[seq]
    out = {"a": ring[:V]}
    if two:
        out["b"] = ring[1:V + 1]
    return out


def workload(bins, J, hm_size):
    import dataclasses

    from fvp.workloads import WORKLOADS

    return dataclasses.replace(WORKLOADS["c5"], voxels_per_axis=bins, num_joints=J, heatmap_size=hm_size)


@functools.lru_cache(None)
def sample_grid(V, seq, bins, hm_size):
    """The oracle's sample grid [V, N, 2] of a camera set and grid, read-only: shared by the cases that use it."""
    import numpy as np

    from fvp import geometry
    from oracle import fvp_oracle as O

    w = workload(bins, 1, hm_size)
    rt = geometry.resize_transform(w.ori_image_size, w.image_size).astype(np.float32)
    grid = O.compute_grid(w.space_size, w.space_center, bins)
    sg = np.stack([O.project_grid(grid, c, w.ori_image_size, w.image_size, hm_size, rt)
                   for c in cameras(V, seq == "b")[seq]])
    sg.setflags(write=False)
    return sg


def case_id(c):
    return f"{c.place}-{c.kind}-{'otf' if c.otf else 'grid'}-B{c.B}V{c.V}J{c.J}-{'x'.join(map(str, c.bins))}-" \
           f"{c.hm[0]}x{c.hm[1]}{'-gi' if c.gi else ''}{'-' + c.want if c.want != 'both' else ''}"
