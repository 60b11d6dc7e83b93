"""The per-person gather's case table: for every class of every place where the
launcher or the kernel decides ("Person gather routes"), a small case
that reaches it.  Each case's class is read back from the plan query
(fvp.ops.person_plan, host only: the decision function the launcher calls), so
the table cannot claim a route it does not take.  Coverage is complete WITHIN a
place, not across places.  test_person_cases.py checks the table, the inputs and
the references on the CPU; test_gpu_person_routes.py runs every case bit for bit
against oracle.fvp_oracle.Individual.person_cubes / max_planes.

All cases share one geometry: the c5 workload with a capture space of 2 m^3 at
the Panoptic centre, person volumes of 1 m^3 (1.5 m for the 65 / 72 deep cubes),
64 x 48 heatmaps and the camera ring of voxelize_cases.cameras.
"""
import collections
import functools
import itertools

import numpy as np

import voxelize_cases as VC
from fvp import ops

# kind: fvp.ops.PERSON_KINDS; hm = (W, H); want: "cubes" | "planes" | "both"; frames: frame_of as a tuple, or None
Case = collections.namedtuple("Case", "place cls kind otf B V J bins hm P want frames")
HM = (64, 48)
SPACE = (2000.0, 2000.0, 2000.0)
ERR_SHAPE = 1002
MAX_JOINTS = 1024  # FVP_MAX_JOINTS
F32 = np.float32


def is_half(c):
    return c.kind == "cl_f16"


def ind_size(c):
    """ind_space_size: 1 m, or 1.5 m for the deep cubic volumes (the fine grid stays near 86^3 .. 96^3)."""
    return (1500.0,) * 3 if c.bins[0] == c.bins[1] == c.bins[2] and c.bins[0] in (65, 72) else (1000.0,) * 3


def cp_of(c):
    """Channels per pixel of the channels-last kinds (fvp.heatmaps.to_channels_last: J rounded up to 16); the
    'padded' slices case carries a whole unused 16-channel group more, filled with junk."""
    if not c.kind.startswith("cl"):
        return 0
    return (c.J + 15) // 16 * 16 + (16 if c.cls and "padded" in c.cls else 0)


def error_of(c):
    return c.cls[1] if c.cls and c.cls[0] == "error" else 0


def plan_of(c):
    ind = individual(c.bins, ind_size(c))
    return ops.person_plan(c.kind, c.B, c.V, c.J, c.hm[1], c.hm[0], c.bins, ind.fine_bins, c.P,
                           want_cubes=c.want != "planes", want_planes=c.want != "cubes", cp=cp_of(c))


def inst_of(r):
    return (r.jpl, r.lpv, r.otf, r.casc)


# ---------------------------------------------------------------------------
# a model of the plan rules, written from the launcher's description, to hold fvp_person_plan to
def model_plan(kind, cp, B, V, J, H, W, bins, fine, P, want_planes, aligned=True):
    """(status, [(j0, jc, lpv, jpl, otf, casc, xsplit, zsplit, xy_direct, blocks, threads, pix_bytes, layout,
    zeroed_planes), ...]) of a per-person call."""
    half, cl, otf = kind == "cl_f16", kind in ("cl", "cl_f16"), kind == "cams"
    lpv32 = lambda j: 1 if j <= 4 else 2 if j <= 8 else 4 if j <= 16 else 8   # a lane holds 4 fp32 joints ...
    lpv16 = lambda j: 1 if j <= 8 else 2 if j <= 16 else 4                     # ... or 8 fp16 joints
    if half and (cp <= 0 or cp % 8 or cp < J or J > MAX_JOINTS or not aligned):
        return ERR_SHAPE, []
    if kind == "cl" and cp <= 0:
        return ERR_SHAPE, []
    if P <= 0:
        return 0, []
    if B <= 0 or not 0 < V <= 255 or not 0 < J <= MAX_JOINTS or H < 2 or W < 2 or (otf and V > 64):
        return ERR_SHAPE, []
    if any(not 0 < s <= 4096 for s in bins) or any(f <= 1 for f in fine):
        return ERR_SHAPE, []
    if want_planes and not bins[0] == bins[1] == bins[2]:
        return ERR_SHAPE, []
    if not otf and fine[0] * fine[1] * fine[2] * (V + V % 2) * 8 > 0xfffff000:
        return ERR_SHAPE, []
    last = J - (J - 1) // 32 * 32   # joints of the last slice
    if half and H * W * cp * 2 > 0x7fffffff:
        return ERR_SHAPE, []
    if kind == "cl" and (cp % 4 or cp < J - last + 4 * lpv32(last) or H * W * cp * 4 > 0x7fffffff):
        return ERR_SHAPE, []
    rows = P * bins[1]
    xsplit = 1 if rows >= 4096 else 2 if rows >= 1024 else 4
    zsplit = -(-bins[2] // 64)
    direct = int(want_planes and xsplit == 1 and zsplit == 1 and bins[0] <= 64 and (half or J <= 16))
    recs = []
    for j0 in range(0, J, 32):
        jc = min(32, J - j0)
        lpv = lpv16(jc) if half else lpv32(jc)
        pix = 2 * cp if half else 4 * (cp if cl else 4 * lpv)
        recs.append((j0, jc, lpv, 8 if half else 4, int(otf), int(V > 16), xsplit, zsplit, direct,
                     (P * bins[1] * xsplit * zsplit) & 0xffffffff, 64 * lpv, pix, int(not cl),
                     0 if not want_planes else 3 if xsplit > 1 else 2))
    return 0, recs


# ---------------------------------------------------------------------------
@functools.lru_cache(None)
def build():
    cases = []

    def add(place, cls, kind, V, J, S, P, want, B=1, frames=None):
        bins = (S,) * 3 if isinstance(S, int) else tuple(S)
        c = Case(place, cls, kind, kind == "cams", B, V, J, bins, HM, P, want, frames)
        if cls is None:
            st, recs = plan_of(c)
            assert st == 0, (c, st)
            r = recs[0]
            c = c._replace(cls=inst_of(r) + (r.xsplit, r.zsplit, r.xy_direct))
        cases.append(c)

    # 1. inst: all 22 instantiations x {cubes, planes}; S = 8, P = 8 (xsplit 4); every J leaves a ragged last joint group
    for want, V in itertools.product(("cubes", "planes"), (5, 17)):
        for i, J in enumerate((3, 7, 15, 30)):
            add("inst", None, "cams", V, J, 8, 8, want)                                   # OTF: planar input
            add("inst", None, ("planar", "cl")[(i + (V > 16) + (want == "planes")) % 2], V, J, 8, 8, want)
        for J in (5, 15, 30):
            add("inst", None, "cl_f16", V, J, 8, 8, want)
    # 2. split: xsplit 1 / 2 / 4 x want, four gather kinds; then the x ranges that do not divide, the empty parts
    #    and the last x slot of the LDS table
    for (kind, J), P, want in itertools.product((("planar", 15), ("cl", 30), ("cl_f16", 15), ("cams", 15)),
                                                (8, 128, 512), ("cubes", "planes", "both")):
        add("split", None, kind, 5, J, 8, P, want)
    for S in (7, 3, 2):
        add("split", None, "planar", 5, 15, S, 8, "both")
    add("split", None, "planar", 2, 4, 64, 64, "planes")
    # 3. depth: zsplit > 1
    for S, J, want in itertools.product((65, 72), (3, 15), ("planes", "both")):
        add("depth", None, "planar", 2, J, S, 3, want)
    add("depth", None, "planar", 5, 15, (5, 3, 130), 8, "cubes")
    add("depth", None, "cams", 5, 15, (9, 5, 3), 8, "cubes")
    add("depth", ("error", ERR_SHAPE), "planar", 5, 15, (5, 3, 130), 8, "both")
    add("depth", ("error", ERR_SHAPE), "cl_f16", 5, 15, (9, 5, 3), 8, "planes")
    # 4. slices: more than 32 joints, every entry kind; channels-last fp32 also with cp > J and junk in the padding
    for J, kind in itertools.product((33, 40, min(64, MAX_JOINTS)), ops.PERSON_KINDS):
        add("slices", ("slices", kind, J), kind, 5, J, 8, 8, "both")
    add("slices", ("slices", "cl", 40, "padded"), "cl", 5, 40, 8, 8, "both")
    # 5. cams: camera counts around the pairs of a lane, the 2 * LPV cameras of a load and the 16-camera blocks
    for V, kind in itertools.product((1, 2, 3, 6, 16, 17, 32, 33, 48), ("planar", "cams", "cl_f16")):
        add("cams", None, kind, V, 15, 8, 8, "both")
    for V, J in itertools.product((3, 17, 33), (3, 30)):
        add("cams", None, "planar", V, J, 8, 8, "both")
    add("cams", ("error", ERR_SHAPE), "cams", 65, 15, 8, 8, "both")
    # 6. frames: three frames with frame_of out of order, and frame_of = None
    order = (2, 0, 1, 2, 2, 0, 1, 1)
    for kind in ("planar", "cl", "cl_f16"):
        add("frames", ("frames", kind, "order"), kind, 5, 15, 8, 8, "both", B=3, frames=order)
        add("frames", ("frames", kind, "none"), kind, 5, 15, 8, 8, "both", B=1, frames=None)
    # 7. window: rounding ties and one-voxel / border windows on every axis (proposals by search, window_proposals)
    for kind in ("planar", "cams"):
        add("window", ("window", kind), kind, 5, 4, 8, len(WINDOW_KINDS) * 3 + 6, "both")
    return tuple(cases)


def case_id(c):
    fr = "" if c.place != "frames" else "-order" if c.frames else "-noframes"
    return f"{c.place}-{c.kind}-B{c.B}V{c.V}J{c.J}-{'x'.join(map(str, c.bins))}-P{c.P}-{c.want}" \
           f"{'-padded' if 'padded' in c.cls else ''}{fr}{'-error' if error_of(c) else ''}"


# ---------------------------------------------------------------------------
# geometry and the oracle's objects
class _Individual:
    """oracle.fvp_oracle.Individual for any person volume: the oracle's constructor also builds the JLN's centre
    grid, which exists for cubic volumes only.  Constants as there (project_individual.py:43-85; for cubic
    volumes test_person_cases.py holds them equal to the oracle's); windows and person_cubes are the oracle's."""

    def __init__(self, whole_size, whole_center, ind_size, ind_bins):
        import torch

        self.wc = torch.tensor(list(map(float, whole_center)))
        self.ws = torch.tensor(list(map(float, whole_size)))
        self.isz = torch.tensor(list(map(float, ind_size)))
        self.vpa = torch.tensor(list(map(int, ind_bins)), dtype=torch.int32)
        self.fine = (self.ws / self.isz * (self.vpa - 1)).int() + 1
        self.scale = (self.fine.float() - 1) / self.ws
        self.bias = -self.isz / 2.0 / self.ws * (self.fine - 1) - self.scale * (self.wc - self.ws / 2.0)
        self.fine_bins = self.fine.numpy().astype(np.int64)


def workload(bins, J, ind):
    import dataclasses

    from fvp.workloads import WORKLOADS

    return dataclasses.replace(WORKLOADS["c5"], space_size=SPACE, ind_space_size=ind, ind_voxels_per_axis=bins,
                               num_joints=J, heatmap_size=HM)


@functools.lru_cache(None)
def individual(bins, ind):
    from oracle import fvp_oracle as O

    w = workload(bins, 1, ind)
    if bins[0] == bins[1] == bins[2]:
        return O.Individual(w.space_size, w.space_center, ind, bins)
    o = _Individual(w.space_size, w.space_center, ind, bins)
    for name in ("fine_grid", "windows", "person_cubes"):
        setattr(o, name, getattr(O.Individual, name).__get__(o))
    return o


@functools.lru_cache(None)
def fine_sample_grid(V, bins, ind):
    """The oracle's fine sample grid [V, FX, FY, FZ, 2] of the case's cameras, read-only."""
    from fvp import geometry
    from oracle import fvp_oracle as O

    w = workload(bins, 1, ind)
    o = individual(bins, ind)
    rt = geometry.resize_transform(w.ori_image_size, w.image_size).astype(F32)
    grid = o.fine_grid()
    sg = np.stack([O.project_grid(grid, c, w.ori_image_size, w.image_size, HM, rt) for c in VC.cameras(V, False)["a"]])
    sg = sg.reshape(V, *o.fine_bins, 2)
    sg.setflags(write=False)
    return sg


# ---------------------------------------------------------------------------
# proposals
def _centre(o, ctl):
    """A proposal centre whose window's top-left fine voxel (centers_tl) is `ctl`."""
    sc, bi = o.scale.numpy().astype(np.float64), o.bias.numpy().astype(np.float64)
    return ((np.asarray(ctl, np.float64) - bi) / sc).astype(F32)


def _tie(o, axis, k):
    """A centre coordinate x with fl(fl(x * scale) + bias) == k + 0.5 exactly in fp32, by search around the
    real solution; None if none within 4096 ulps."""
    sc, bi = F32(o.scale[axis].item()), F32(o.bias[axis].item())
    x0 = F32((np.float64(k) + 0.5 - np.float64(bi)) / np.float64(sc))
    for away in (F32(np.inf), F32(-np.inf)):
        x = x0
        for _ in range(4096):
            if F32(F32(x * sc) + bi) == F32(k + 0.5):
                return x
            x = np.nextafter(x, away)
    return None


WINDOW_KINDS = ("tie even", "tie odd", "one voxel low", "end at fine", "one voxel high")


def window_proposals(c):
    """Per axis: a centre whose pc * scale + bias is exactly k + 0.5 for an even and for an odd k (round half
    to even), ctl == -S + 1 (start == end - 1 at the low border), end == fine exactly, and ctl == fine - 1
    (start == end - 1 at the high border); the other two axes inside.  Returns (rows [3 * 5, 7], ties) with
    ties = [(row, axis, k), ...]."""
    o = individual(c.bins, ind_size(c))
    rng = np.random.default_rng(77)
    S, F = np.array(c.bins), o.fine_bins
    rows, ties = [], []
    for a in range(3):
        for kind in WINDOW_KINDS:
            ctl = rng.integers(0, F - S + 1)
            row = np.zeros(7, F32)
            row[4], row[5:7] = 0.9, 1.0
            if kind.startswith("tie"):
                want_even = kind == "tie even"
                found = None
                for k in range(int(F[a] - S[a]) + 1):
                    if (k % 2 == 0) == want_even and _tie(o, a, k) is not None:
                        found = (k, _tie(o, a, k))
                        break
                assert found is not None, (c, a, kind)
                row[:3] = _centre(o, ctl)
                row[a] = found[1]
                ties.append((len(rows), a, found[0]))
            else:
                ctl[a] = {"one voxel low": -S[a] + 1, "end at fine": F[a] - S[a], "one voxel high": F[a] - 1}[kind]
                row[:3] = _centre(o, ctl)
            rows.append(row)
    return np.stack(rows), ties


def proposals(c):
    """[P, 7] rows (x, y, z, -, score, bbox w, bbox h) of a case: a full window, one clipped at the low border of
    an axis (ctl < 0), one clipped at the high border, one skipped (start >= end), one with both bbox entries
    > 1 (negative margin -> 0), one whose margins alone empty the window, the rest uniform over the space with
    bbox entries uniform in [-0.2, 1.2].  With fewer than six proposals (the deep cubes: three) the classes
    share proposals: full with bbox > 1, clipped low on x and high on y, emptied by its margins."""
    o = individual(c.bins, ind_size(c))
    S, F = np.array(c.bins), o.fine_bins
    rng = np.random.default_rng(1000 * c.V + 10 * c.J + c.P + 7 * c.bins[2])
    inside = lambda: rng.integers(0, F - S + 1)

    def row(ctl, bbox):
        r = np.zeros(7, F32)
        r[:3], r[4], r[5:7] = _centre(o, ctl), 0.9, bbox
        return r

    def low():
        ctl = inside()
        a = int(rng.integers(0, 3))
        ctl[a] = -int(rng.integers(1, S[a]))
        return ctl

    def high():
        ctl = inside()
        a = int(rng.integers(0, 3))
        ctl[a] = F[a] - S[a] + int(rng.integers(1, S[a]))
        return ctl

    if c.P < 6:
        both = inside()
        both[0], both[1] = -int(rng.integers(1, S[0])), F[1] - S[1] + int(rng.integers(1, S[1]))
        rows = [row(inside(), (1.1, 1.2)), row(both, (1.0, 1.0)), row(inside(), (-1.0, -1.0))]
    else:
        skipped, a = inside(), int(rng.integers(0, 3))
        skipped[a] = -S[a] if rng.integers(0, 2) else F[a]   # the window ends at voxel 0, or starts at fine
        rows = [row(inside(), (1.0, 1.0)), row(low(), (1.0, 1.0)), row(high(), (1.0, 1.0)), row(skipped, (1.0, 1.0)),
                row(inside(), (1.1, 1.2)), row(inside(), (-1.0, -1.0))]
    if c.place == "window":
        rows += list(window_proposals(c)[0])
    w = workload(c.bins, 1, ind_size(c))
    while len(rows) < c.P:
        r = np.zeros(7, F32)
        r[:3] = np.array(w.space_center) + rng.uniform(-0.5, 0.5, 3) * np.array(SPACE)
        r[4], r[5:7] = 0.9, rng.uniform(-0.2, 1.2, 2)
        rows.append(r)
    assert len(rows) == c.P, (c, len(rows))
    return np.stack(rows).astype(F32)


def classes(c, props=None):
    """Per proposal: 'skipped', else 'full' (the window is the whole cube) or 'clipped', with ' low' / ' high'
    for the borders it is clipped at."""
    o = individual(c.bins, ind_size(c))
    ctl, _, start, end = o.windows(proposals(c) if props is None else props)
    S, F = np.array(c.bins), o.fine_bins
    out = []
    for i in range(len(ctl)):
        if np.any(start[i] >= end[i]):
            out.append("skipped")
            continue
        full = np.array_equal(start[i], ctl[i]) and np.array_equal(end[i], ctl[i] + S)
        out.append(("full" if full else "clipped") + (" low" if np.any(ctl[i] < 0) else "") +
                   (" high" if np.any(ctl[i] + S > F) else ""))
    return out


# ---------------------------------------------------------------------------
# inputs and references, shared by the cases with the same inputs (the kinds, wants and coordinate sources of a shape)
@functools.lru_cache(None)
def _heatmaps(half, B, V, J):
    import torch

    g = torch.Generator().manual_seed(1000 * V + 10 * J + B)
    hm = torch.rand((B, V, J, HM[1], HM[0]), generator=g)   # every frame differs: a wrong frame_of shows
    return hm.half() if half else hm


def heatmaps(c):
    """[B, V, J, H, W] torch.rand, fp16 for the fp16 kind (the reference sees .half().float())."""
    return _heatmaps(is_half(c), c.B, c.V, c.J)


def frame_of(c):
    return None if c.frames is None else np.array([c.frames[i % len(c.frames)] for i in range(c.P)], np.int32)


def _cut(o, vol, props, bins):
    """Each proposal's window of the whole fine volume [J, FX, FY, FZ], in a zero cube."""
    ctl, offset, start, end = o.windows(props)
    cubes = np.zeros((len(props), vol.shape[0]) + tuple(bins), F32)
    for i in range(len(props)):
        s, e = start[i], end[i]
        if np.any(s >= e):
            continue
        o0, o1 = s - ctl[i], e - ctl[i]
        cubes[i, :, o0[0]:o1[0], o0[1]:o1[1], o0[2]:o1[2]] = vol[:, s[0]:e[0], s[1]:e[1], s[2]:e[2]]
    return cubes, offset


def sliced_reference(c, rows=None):
    """person_cubes for many proposals: the whole fine grid voxelized once per frame (oracle.voxelize: the same
    per-voxel arithmetic as person_cubes, independent of the window), each proposal's window
    (Individual.windows) cut out of it.  test_person_cases.py holds it equal to person_cubes bit for bit."""
    from oracle import fvp_oracle as O

    o = individual(c.bins, ind_size(c))
    sg = fine_sample_grid(c.V, c.bins, ind_size(c))
    hm = heatmaps(c).float().numpy()
    props, fo = proposals(c), frame_of(c)
    rows = np.arange(c.P) if rows is None else np.asarray(rows)
    cubes = np.zeros((len(rows), c.J) + tuple(c.bins), F32)
    offset = np.zeros((len(rows), 3), F32)
    for b in range(c.B):
        sel = np.nonzero((fo[rows] if fo is not None else np.zeros(len(rows), int)) == b)[0]
        if len(sel) == 0:
            continue
        vol = O.voxelize(hm[b], sg.reshape(c.V, -1, 2)).reshape(c.J, *o.fine_bins)
        cubes[sel], offset[sel] = _cut(o, vol, props[rows[sel]], c.bins)
    return cubes, offset


def direct_reference(c, rows=None):
    """Individual.person_cubes, frame by frame."""
    o = individual(c.bins, ind_size(c))
    sg = fine_sample_grid(c.V, c.bins, ind_size(c))
    hm = heatmaps(c).float().numpy()
    props, fo = proposals(c), frame_of(c)
    rows = np.arange(c.P) if rows is None else np.asarray(rows)
    cubes = np.zeros((len(rows), c.J) + tuple(c.bins), F32)
    offset = np.zeros((len(rows), 3), F32)
    for b in range(c.B):
        sel = np.nonzero((fo[rows] if fo is not None else np.zeros(len(rows), int)) == b)[0]
        if len(sel):
            cubes[sel], offset[sel] = o.person_cubes(hm[b], sg, props[rows[sel]])
    return cubes, offset


SLICED_ABOVE = 16  # proposals: beyond, person_cubes costs minutes (P V J S^3) and the sliced reference stands in


def uses_sliced(c):
    """Whether the case's reference is the sliced stand-in (the window cases, 21 proposals, keep person_cubes:
    every searched row is then the oracle's own)."""
    return c.P > SLICED_ABOVE and c.place != "window"


@functools.lru_cache(None)
def _reference(c):
    cubes, offset = (sliced_reference if uses_sliced(c) else direct_reference)(c)
    cubes.setflags(write=False)
    offset.setflags(write=False)
    return cubes, offset


def reference(c):
    """(cubes [P, J, SX, SY, SZ], offset [P, 3]) of the case, read-only, computed once per set of inputs."""
    return _reference(c._replace(place="window" if c.place == "window" else "", cls=(), otf=False, want="",
                                 kind="cl_f16" if is_half(c) else "planar"))


def in_window_mask(c):
    """[P, SX, SY, SZ] bool: the voxels inside the windows of the proposals that are not skipped."""
    o = individual(c.bins, ind_size(c))
    ctl, _, start, end = o.windows(proposals(c))
    m = np.zeros((c.P,) + tuple(c.bins), bool)
    for i in range(c.P):
        s, e = start[i], end[i]
        if np.any(s >= e):
            continue
        o0, o1 = s - ctl[i], e - ctl[i]
        m[i, o0[0]:o1[0], o0[1]:o1[1], o0[2]:o1[2]] = True
    return m


def fill_of(c):
    """(share of nonzero in-window voxels, least share of distinct in-window values of a joint, any value at 1).
    Distinct values are counted within one proposal's window: the windows of a case overlap in the fine grid
    (512 proposals share 15^3 fine voxels), so across proposals values repeat by construction."""
    cubes, _ = reference(c)
    m = in_window_mask(c)
    nz = n = 0
    distinct, at_one = 1.0, False
    for i in np.nonzero(m.any(axis=(1, 2, 3)))[0]:
        vals = cubes[i][:, m[i]]   # [J, voxels of the window]
        nz, n = nz + np.count_nonzero(vals), n + vals.size
        distinct = min(distinct, min(len(np.unique(vals[j])) for j in range(c.J)) / vals.shape[1])
        at_one |= bool((vals >= 1).any())
    return nz / max(n, 1), distinct, at_one


# ---------------------------------------------------------------------------
def nan_max(a, axis):
    """max along `axis` with NaN winning (torch.max; the kernels' nanmax), as an explicit numpy loop."""
    a = np.moveaxis(np.asarray(a, F32), axis, 0)
    m = a[0].copy()
    for t in range(1, a.shape[0]):
        v = a[t]
        take = np.isnan(v) | (~np.isnan(m) & (v > m))
        m = np.where(take, v, m)
    return m


def zero_sign_defined(a, axis):
    """Cells whose maximum along `axis` is a zero of a defined sign: no NaN in the line and all its zero-valued
    elements share one sign (then every visiting order gives that zero; with both signs in the line the result
    depends on the order torch.max or a kernel visits them)."""
    a = np.asarray(a, F32)
    zero = a == 0
    neg = zero & np.signbit(a)
    mixed = neg.any(axis=axis) & (zero & ~neg).any(axis=axis)
    with np.errstate(invalid="ignore"):
        return ~np.isnan(a).any(axis=axis) & (np.nanmax(np.where(np.isnan(a), -np.inf, a), axis=axis) == 0) & ~mixed


def zero_sign_defined_planes(cubes):
    """zero_sign_defined in the layout of nan_max_planes."""
    return np.concatenate([zero_sign_defined(cubes, 4), zero_sign_defined(cubes, 3), zero_sign_defined(cubes, 2)], axis=0)


def nan_max_planes(cubes):
    """oracle.max_planes with NaN winning: cat([max z, max y, max x]) of [P, J, S, S, S]."""
    return np.concatenate([nan_max(cubes, 4), nan_max(cubes, 3), nan_max(cubes, 2)], axis=0)
