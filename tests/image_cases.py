"""The case table of the heatmap sizes and image borders ("Heatmap sizes and
image borders"): every pair-table layout kernel at every width class, frame grouping and
source alignment the choice allows, the fp32 / fp16 -> fp32 layout at ragged sizes, every
entry kind that takes a packed grid on a planted grid (image_ref.planted_grid: all 25 tap
classes, corners included), the on-the-fly kinds on a portrait image (every x class comes
from projection), fvp_voxel_columns in all 8 instantiations, and the four per-person kinds
at two sizes (person_cases(), at the end).  Coverage is complete
WITHIN a place, not across places.  test_image_cases.py checks the table on the CPU,
test_gpu_image_routes.py runs it bit for bit against the oracle.
"""
import collections
import functools
import itertools

import numpy as np

import image_ref as R
import voxelize_cases as VC
from fvp import ops

# hm = (W, H); src: "planted" | "portrait"; amod: heatmap address mod 16 (planar fp16 sources carved out of a
# larger buffer); strides (columns): "planar" | "cl"
Case = collections.namedtuple("Case", "place cls kind otf B V J bins hm gi want src amod strides")

GRIDS = ((10, 9, 4), (12, 10, 6), (8, 8, 8), (7, 5, 3))
PORTRAIT = (512, 960)      # image_size: the letter-box moves to y, so x leaves the image
SPACE_SCALE = 2.5
WIDTHS = (2, 3, 6, 8, 10, 12, 14, 16, 61, 64, 130, 508, 510)
AMODS = (0, 2, 4, 8)
PLANTED_SIZES = ((64, 48), (61, 33), (10, 6), (2, 2), (130, 10))
PORTRAIT_SIZES = ((48, 64), (33, 61), (6, 10))
COLUMN_VIEWS = (1, 4, 5, 8, 9, 16, 17, 33)


def _case(place, cls, kind, B, V, J, bins, hm, otf=False, gi=False, src=None, amod=0, strides="planar"):
    return Case(place, cls, kind, otf, B, V, J, bins, hm, gi, "both", src or ("portrait" if otf else "planted"), amod,
                strides)


def grid_for(hm, i=0):
    """A small grid that holds the planted samples of the size: (7, 5, 3) where an axis of 2 or 3 pixels leaves
    room (fewer reachable classes), else the i-th of the other three."""
    need = R.MIN_SPECIALS + R.PER_PAIR * len(R.axis_candidates(hm[0])) * len(R.axis_candidates(hm[1]))
    return GRIDS[3] if need <= 7 * 5 * 3 else GRIDS[i % 3]


def layout_of(c):
    """The pair-table layout kernel of a one-chunk planar fp16 case (the query; B frames per entry)."""
    return ops.pair_layout_kind(c.B, c.hm[0], c.amod)


@functools.lru_cache(None)
def build():
    cases = []
    # 1. pair layout: every (NF, W, address class), each on the kernel the choice gives it; H through 2, 3, 33;
    #    wide heatmaps at V = 1, H = 2
    for i, (nf, W, a) in enumerate(itertools.product((4, 2, 1), WIDTHS, AMODS)):
        k = R.pair_layout_model(nf, W, a)
        wide = W >= 128
        H = 2 if wide else (2, 3, 33)[i % 3]
        J = 16 if (W, nf) == (130, 4) else 15
        cases.append(_case("pairs", (R.LAYOUT_NAMES[k], nf, W, a), "planar_f16", nf, 1 if wide else 2, J,
                           grid_for((W, H)), (W, H), amod=a))
    # 2. pair joints: ragged joint quads and zero joints on each kernel at NF = 4
    for (k, W, a), J in itertools.product(((R.VEC8, 16, 0), (R.ROWS, 10, 0), (R.ENTRY, 61, 0)), (1, 3, 4, 5, 8, 13, 16)):
        cases.append(_case("joints", (R.LAYOUT_NAMES[k], J), "planar_f16", 4, 2, J, grid_for((W, 3)), (W, 3), amod=a))
    # 3. fp32 and fp16 -> fp32 channels-last layout: LPV 1, 2, 4, 8 from fp32, 8 from fp16, ragged sizes
    for i, ((kind, J), hm) in enumerate(itertools.product(
            (("planar_f32", 3), ("planar_f32", 7), ("planar_f32", 13), ("planar_f32", 29), ("planar_f16", 17),
             ("planar_f16", 32)), ((61, 33), (45, 31), (2, 2), (10, 6)))):
        cases.append(_case("layout", (kind, J, hm), kind, 1, 3, J, grid_for(hm, i), hm))
    for kind in ("planar_f32", "planar_f16"):   # a last slice of one joint: Jst != J on an odd H * W
        cases.append(_case("layout", (kind, 33, (45, 31)), kind, 1, 3, 33, grid_for((45, 31)), (45, 31)))
    # 4. borders on a cached (planted) grid: every entry kind x every size x V = 5, 17
    kinds = [("planar_f32", 1, J) for J in (4, 8, 15, 32)] + [("planar_f16", B, 15) for B in (4, 2, 1)] + \
            [("cl_f32", 1, 15)] + [("cl_f16", 1, J) for J in (8, 16, 32)]
    for i, ((kind, B, J), hm, V) in enumerate(itertools.product(kinds, PLANTED_SIZES, (5, 17))):
        cases.append(_case("border", (kind, B, J, V, hm), kind, B, V, J, grid_for(hm, i), hm))
    # 5. borders from projection: the _cams kinds on the portrait image
    for (ki, (kind, B)), (si, hm) in itertools.product(
            enumerate((("planar_f32", 1), ("planar_f16", 2), ("cl_f32", 1), ("cl_f16", 1))), enumerate(PORTRAIT_SIZES)):
        V = (5, 17)[(ki + si) % 2]
        cases.append(_case("border_otf", (kind, V, hm), kind, B, V, 15, (10, 9, 4), hm, otf=True))
    # 6. columns: (fp32, fp16) x (grid, on the fly) x V; planar and channels-last strides alternating so that
    #    each of the 8 instantiations meets both; one grid_index case per coordinate source
    for (hi, half), (oi, otf), (vi, V) in itertools.product(enumerate((False, True)), enumerate((False, True)),
                                                             enumerate(COLUMN_VIEWS)):
        hm = (PORTRAIT_SIZES if otf else PLANTED_SIZES[:4])[(vi + hi) % (3 if otf else 4)]
        if otf and V == 1:
            hm = PORTRAIT_SIZES[2]   # one camera: only the smallest size has 8 samples at x0 == W - 1
        strides = ("planar", "cl")[(vi // 2 + vi + hi) % 2]
        kind = ("cl_" if strides == "cl" else "planar_") + ("f16" if half else "f32")
        cases.append(_case("columns", (half, otf, V > 16, V, strides), kind, 2, V, 5,
                           (12, 10, 6) if otf else grid_for(hm, vi), hm, otf=otf, strides=strides))
    for otf in (False, True):
        hm = (33, 61) if otf else (61, 33)
        cases.append(_case("columns", ("grid_index", otf), "planar_f32", 3, 5, 5, (12, 10, 6) if otf else (10, 9, 4), hm,
                           otf=otf, gi=True))
    return tuple(cases)


def case_id(c):
    return f"{c.place}-{c.kind}-{'otf' if c.otf else 'grid'}-B{c.B}V{c.V}J{c.J}-{'x'.join(map(str, c.bins))}-" \
           f"{c.hm[0]}x{c.hm[1]}{'-gi' if c.gi else ''}{'-a%d' % c.amod if c.amod else ''}" \
           f"{'-cl' if c.place == 'columns' and c.strides == 'cl' else ''}"


def plan_of(c):
    return VC.plan_of(c)


def workload(c):
    """C5's geometry at the case's grid, joints and heatmap size; the projected cases on the portrait image
    with the space scaled (the voxels then project across the left and right image borders)."""
    import dataclasses

    w = VC.workload(c.bins, c.J, c.hm)
    if c.src == "portrait":
        w = dataclasses.replace(w, image_size=PORTRAIT, space_size=tuple(SPACE_SCALE * s for s in w.space_size))
    return w


@functools.lru_cache(None)
def _planted(V, N, hm, seed):
    sg = R.planted_grid(V, N, hm[0], hm[1], seed)
    sg.setflags(write=False)
    return sg


@functools.lru_cache(None)
def _projected(V, seq, bins, hm):
    from fvp import geometry
    from oracle import fvp_oracle as O

    w = workload(_case("", None, "planar_f32", 1, V, 1, bins, hm, otf=True))
    rt = geometry.resize_transform(w.ori_image_size, w.image_size).astype(np.float32)
    grid = O.compute_grid(w.space_size, w.space_center, bins)
    sg = np.stack([O.project_grid(grid, cam, w.ori_image_size, w.image_size, hm, rt)
                   for cam in VC.cameras(V, seq == "b")[seq]])
    sg.setflags(write=False)
    return sg


def sample_grid(c, seq="a"):
    """The case's sample grid [V, N, 2] of sequence "a" (or "b", the cases with a grid_index), read-only."""
    if c.src == "portrait":
        return _projected(c.V, seq, c.bins, c.hm)
    X, Y, Z = c.bins
    return _planted(c.V, X * Y * Z, c.hm, 1 if seq == "a" else 2)


def seqs_of(c):
    return [("b" if c.gi and b % 2 else "a") for b in range(c.B)]


@functools.lru_cache(None)
def _heatmaps(half, B, V, J, hm):
    import torch

    g = torch.Generator().manual_seed(1000 * V + 10 * J + B + 7 * hm[0])
    t = torch.rand((B, V, J, hm[1], hm[0]), generator=g)   # every frame differs
    return t.half() if half else t


def heatmaps(c):
    """[B, V, J, H, W] torch.rand, fp16 for the fp16 kinds (the oracle sees .half().float())."""
    return _heatmaps(c.kind.endswith("f16"), c.B, c.V, c.J, c.hm)


@functools.lru_cache(None)
def _oracle(half, B, V, J, bins, hm, src, gi):
    from oracle import fvp_oracle as O

    c = _case("", None, "planar_f16" if half else "planar_f32", B, V, J, bins, hm, otf=src == "portrait", gi=gi, src=src)
    h = heatmaps(c).float().numpy()
    out = np.stack([O.voxelize(h[b], sample_grid(c, s)).reshape(J, *bins) for b, s in enumerate(seqs_of(c))])
    out.setflags(write=False)
    return out


def oracle_cube(c):
    """oracle.fvp_oracle.voxelize of every frame, [B, J, X, Y, Z], read-only, once per set of inputs."""
    return _oracle(c.kind.endswith("f16"), c.B, c.V, c.J, c.bins, c.hm, c.src, c.gi)


def flat_of(c):
    """Columns: every index of the map once per frame (each frame in another order), then -1 and X * Y."""
    X, Y, _ = c.bins
    rng = np.random.default_rng(c.V)
    return np.stack([np.concatenate([rng.permutation(X * Y), [-1, X * Y]]) for _ in range(c.B)]).astype(np.int64)


# ---------------------------------------------------------------------------
# the per-person gather at other heatmap sizes: the cached kinds sample a planted fine grid, the on-the-fly
# kind projects the fine grid of a scaled space onto the portrait image
PERSON_KINDS = ("planar", "cams", "cl", "cl_f16")
PERSON_SIZES = ((61, 33), (10, 6))
PERSON_BINS, PERSON_P, PERSON_J, PERSON_V = (8, 8, 8), 4, 15, 5
# window corners (centers_tl) on the fine grid of 15^3: the cached kinds' four windows cover fine x < 8 entirely
# (the planted slots are the first ones, x-major); the projected kind's windows are spread over the space
PERSON_CTL = {False: ((0, 0, 0), (0, 7, 0), (0, 0, 7), (0, 7, 7)), True: ((0, 0, 0), (7, 7, 0), (0, 7, 7), (7, 0, 7))}


@functools.lru_cache(None)
def person_cases():
    import person_cases as PC

    out = []
    for kind, hm in itertools.product(PERSON_KINDS, PERSON_SIZES):
        otf = kind == "cams"
        out.append(PC.Case("person", (kind, hm), kind, otf, 1, PERSON_V, PERSON_J, PERSON_BINS,
                           (hm[1], hm[0]) if otf else hm, PERSON_P, "both", None))
    return tuple(out)


def person_id(c):
    return f"person-{c.kind}-{c.hm[0]}x{c.hm[1]}"


def person_workload(c):
    """(workload, person volume size): 2 m of space and 1 m volumes as the person route table; the projected
    kind on the portrait image with C5's space scaled and volumes of half the space (a fine grid of 15^3)."""
    import dataclasses

    import person_cases as PC
    from fvp.workloads import WORKLOADS

    w = dataclasses.replace(PC.workload(c.bins, c.J, (1000.0,) * 3), heatmap_size=c.hm)
    if c.otf:
        space = tuple(SPACE_SCALE * s for s in WORKLOADS["c5"].space_size)
        w = dataclasses.replace(w, image_size=PORTRAIT, space_size=space, ind_space_size=tuple(s / 2 for s in space))
    return w, tuple(w.ind_space_size)


@functools.lru_cache(None)
def person_individual(c):
    from oracle import fvp_oracle as O

    w, ind = person_workload(c)
    return O.Individual(w.space_size, w.space_center, ind, c.bins)


@functools.lru_cache(None)
def _person_fine(otf, V, hm):
    import person_cases as PC
    from fvp import geometry
    from oracle import fvp_oracle as O

    c = PC.Case("person", None, "cams" if otf else "planar", otf, 1, V, 1, PERSON_BINS, hm, PERSON_P, "both", None)
    o = person_individual(c)
    n = int(np.prod(o.fine_bins))
    if otf:
        w, _ = person_workload(c)
        rt = geometry.resize_transform(w.ori_image_size, w.image_size).astype(np.float32)
        grid = o.fine_grid()
        sg = np.stack([O.project_grid(grid, cam, w.ori_image_size, w.image_size, hm, rt)
                       for cam in VC.cameras(V, False)["a"]])
    else:
        sg = R.planted_grid(V, n, hm[0], hm[1], 3)
    sg.setflags(write=False)
    return sg


def person_fine_grid(c):
    """The fine sample grid [V, FX * FY * FZ, 2] of a person case, read-only."""
    return _person_fine(c.otf, c.V, c.hm)


def person_proposals(c):
    """[P, 7]: windows at PERSON_CTL with bbox entries 1 (no margin), each the whole 8^3 volume."""
    import person_cases as PC

    o = person_individual(c)
    rows = np.zeros((c.P, 7), np.float32)
    for i, ctl in enumerate(PERSON_CTL[c.otf]):
        rows[i, :3], rows[i, 4], rows[i, 5:7] = PC._centre(o, ctl), 0.9, 1.0
    return rows


@functools.lru_cache(None)
def _person_heatmaps(half, V, J, hm):
    import torch

    g = torch.Generator().manual_seed(31 * V + J + 7 * hm[0])
    t = torch.rand((1, V, J, hm[1], hm[0]), generator=g)
    return t.half() if half else t


def person_heatmaps(c):
    return _person_heatmaps(c.kind == "cl_f16", c.V, c.J, c.hm)


@functools.lru_cache(None)
def _person_reference(half, otf, V, J, hm):
    import person_cases as PC
    from oracle import fvp_oracle as O

    c = PC.Case("person", None, "cl_f16" if half else "cams" if otf else "planar", otf, 1, V, J, PERSON_BINS, hm,
                PERSON_P, "both", None)
    o = person_individual(c._replace(J=1))
    vol = O.voxelize(person_heatmaps(c)[0].float().numpy(), np.array(person_fine_grid(c))).reshape(J, *o.fine_bins)
    cubes, offset = PC._cut(o, vol, person_proposals(c), c.bins)
    cubes.setflags(write=False)
    return cubes, offset


def person_reference(c):
    """person_cases.sliced_reference on the case's own fine grid: the whole fine grid voxelized by the oracle,
    each proposal's window (Individual.windows) cut out of it.  (cubes [P, J, 8, 8, 8], offset [P, 3])."""
    return _person_reference(c.kind == "cl_f16", c.otf, c.V, c.J, c.hm)


def person_window_samples(c):
    """[V, M, 2]: the fine-grid samples inside the case's windows, each fine voxel once."""
    o = person_individual(c)
    _, _, start, end = o.windows(person_proposals(c))
    inside = np.zeros(tuple(o.fine_bins), bool)
    for s, e in zip(start, end):
        inside[s[0]:e[0], s[1]:e[1], s[2]:e[2]] = True
    return np.array(person_fine_grid(c))[:, inside.reshape(-1)]
