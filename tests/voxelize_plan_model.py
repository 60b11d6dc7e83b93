"""A plain-Python restatement of the voxelize gather's launch rules
(csrc/fvp_voxelize.hip), written from its comments and constants, for
test_voxelize_plan_model.py to hold fvp_voxelize_plan to.

plan(...) returns (status, [record, ...]) with the fields of
fvp.ops.GatherLaunch in order, and fills `trace` -- the values every threshold
comparison saw -- so a sweep can show that both sides of each were reached.
plan(..., classes=[]) and band_class(...) name the gather_cfg class of a record
(branch, snap, band), which the case table (voxelize_cases.py) is organised by.
"""
import collections

OK, ERR_SHAPE = 0, 1002
MAX_JOINTS, MAX_VIEWS, CAM_STRIDE = 1024, 255, 24
BAND_ROWS, JOINT_SLICE, PAIR_FRAMES = 16, 32, 4
MB = 1 << 20
KINDS = ("planar_f32", "planar_f16", "cl_f32", "cl_f16")

Cfg = collections.namedtuple("Cfg", "cols band col_blocks sp lds status branch snap")


def lanes_per_voxel(J):
    """fp32 channels-last table: 4 joints per lane."""
    return 1 if J <= 4 else 2 if J <= 8 else 4 if J <= 16 else 8


def lanes_per_voxel_h(J):
    """fp16 channels-last pixels read in place: 8 joints per lane."""
    return 1 if J <= 8 else 2 if J <= 16 else 4


def use_pairs(J, half):
    return half and J <= 16


def frame_bytes(V, J, H, W, half):
    if use_pairs(J, half):
        return V * H * (W + 1) * 64           # pixel-pair entries of 64 B
    return V * H * W * 4 * lanes_per_voxel(J) * 4


def chunk_frames(B, V, J, H, W, half, trace=None):
    per = frame_bytes(V, J, H, W, half)
    pairs = use_pairs(J, half)
    c = (128 * MB if pairs else 120 * MB) // max(per, 1)
    if trace is not None:
        trace["budget_pairs" if pairs else "budget_f32"].add(min(c, 2))   # 0, 1, 2+: frames the budget holds
    if pairs and c < PAIR_FRAMES:
        bump = PAIR_FRAMES * per <= 256 * MB
        if trace is not None:
            trace["pair_bump"].add(bump)
        if bump:
            c = PAIR_FRAMES
    return min(max(c, 1), B)


def cols_per_block(Z):
    return 1 if Z >= 256 else 256 // Z if Z >= 32 else 160 // Z


def stage_pitch(L, cols, Z, trace=None):
    """L: 16-B units per stage column (LPV * JPL / 4)."""
    T = cols * Z
    pad = 1 if T % 4 else 4
    padded, tight = 16 * L * (T + pad), 16 * L * T
    if trace is not None:
        for v in (padded, tight):
            if abs(v - 20480) <= 64:
                trace["stage_20480"].add(v > 20480)
    return T if padded > 20480 and tight <= 20480 else T + pad


def gather_cfg(LPV, OTF, JPL, frames, NF, V, X, Y, Z, trace=None):
    big = X * Y >= 4096
    kinds = []

    def snap(c):
        if not big:
            kinds.append("small")
            return c
        cc = c
        while cc > 1 and Y % cc:
            cc -= 1
        if trace is not None:
            trace["snap_half"].add((2 * cc - c > 0) - (2 * cc - c < 0))   # 2cc < c, = c, > c
        kinds.append("unchanged" if cc == c else "snapped" if 2 * cc >= c else "rejected")
        return cc if 2 * cc >= c else c

    def blocks(c):
        return frames // NF * ((X * Y + c - 1) // c)

    otf_vox = 128 if NF >= 4 else 256
    cols = snap((1 if Z >= otf_vox else otf_vox // Z) if OTF else cols_per_block(Z))
    branch = "throughput"
    if trace is not None:
        trace["xy"].add(X * Y)
        trace["blocks_1024"].add(blocks(cols))
        trace["z"].add(Z)
    if blocks(cols) < 1024:
        cols = snap(max(1, (256 // LPV) // Z))
        branch = "one"
        if trace is not None:
            trace["blocks_2048"].add(blocks(cols))
        if blocks(cols) > 2048:
            cols = snap(max(1, 2 * (256 // LPV) // Z))
            branch = "two"
    band = BAND_ROWS if big and Y % cols == 0 and X > BAND_ROWS else 0
    col_blocks = (X * Y + cols - 1) // cols
    sp = stage_pitch(LPV * JPL // 4, cols, Z, trace)
    lds = NF * JPL * LPV * sp * 4
    if OTF:
        lds = (lds // 4 + 3) // 4 * 4 * 4 + (V + (V & 1)) * CAM_STRIDE * 4
    if trace is not None:
        trace["lds_160k"].add(lds > 160 * 1024)
    return Cfg(cols, band, col_blocks, sp, lds, ERR_SHAPE if lds > 160 * 1024 else OK, branch, kinds[-1])


def stage_vec(T, sp, Z, N, cube16):
    return T % 4 == 0 and sp % 4 == 0 and Z % 4 == 0 and N % 4 == 0 and cube16


def _record(j0, LPV, JPL, pair, otf, casc, NF, f0, nb, c, Jslice, X, Y, Z, cube16, tab, status):
    vpp = 256 // LPV
    N = X * Y * Z
    last = X * Y - (c.col_blocks - 1) * c.cols
    family = (4 if otf else 3) if JPL == 8 else (2 if otf else 1)
    return (j0, family, LPV, JPL, int(pair), int(casc), NF, f0, nb, c.cols, c.band, c.col_blocks, c.sp, c.lds,
            -(-c.cols * Z // vpp), int(stage_vec(c.cols * Z, c.sp, Z, N, cube16)),
            int(stage_vec(last * Z, c.sp, Z, N, cube16)), status, nb // NF * c.col_blocks, last, -(-last * Z // vpp),
            tab, int(otf), Jslice)


def plan(kind, otf, B, V, J, H, W, X, Y, Z, cp=0, grid_index=False, cube_aligned=True, trace=None, classes=None):
    """(status, records).  classes (a list, optional) receives (branch, snap) per record."""
    half = kind in ("planar_f16", "cl_f16")
    if (B <= 0 or V <= 0 or V > MAX_VIEWS or J <= 0 or J > MAX_JOINTS or H < 2 or W < 2 or X <= 0 or Y <= 0 or Z <= 0
            or X * Y * Z * (V + (V & 1)) * 8 > 0xfffff000):
        return ERR_SHAPE, []
    if kind == "cl_f16" and (cp <= 0 or cp % 8 or cp < J or H * W * cp * 2 > 0x7fffffff):
        return ERR_SHAPE, []
    if kind == "cl_f32":
        jl = (J - 1) // JOINT_SLICE * JOINT_SLICE
        if cp % 4 or cp < jl + 4 * lanes_per_voxel(J - jl) or H * W * cp * 4 > 0x7fffffff:
            return ERR_SHAPE, []
    if kind.startswith("planar") and frame_bytes(1, min(J, JOINT_SLICE), H, W, half) > 0x7fffffff:
        return ERR_SHAPE, []
    if trace is not None:
        trace["v"].add(V)
        trace["j"].add(J)
    casc = V > 16
    N = X * Y * Z
    recs = []

    def note(c):
        if classes is not None:
            classes.append((c.branch, c.snap))

    for j0 in range(0, J, JOINT_SLICE):
        Js = min(JOINT_SLICE, J - j0)
        # the slice's cube starts j0 * N floats in: 16-B aligned with the cube if that is a multiple of 4
        cube16 = cube_aligned and (j0 * N) % 4 == 0 or (not cube_aligned and (1 + j0 * N) % 4 == 0)
        if kind.startswith("cl"):
            JPL = 8 if half else 4
            LPV = lanes_per_voxel_h(Js) if half else lanes_per_voxel(Js)
            c = gather_cfg(LPV, otf, JPL, B, 1, V, X, Y, Z, trace)
            note(c)
            recs.append(_record(j0, LPV, JPL, False, otf, casc, 1, 0, B, c, Js, X, Y, Z, cube16, 0, c.status))
            if c.status != OK:
                return c.status, recs
            continue
        pair = use_pairs(J, half)           # (the whole call's joints: J <= 16 is never sliced)
        LPV = 4 if pair else lanes_per_voxel(Js)

        def run_chunks(first, last, NF):
            n = last - first
            chunk = max(NF, chunk_frames(n, V, Js, H, W, half, trace) // NF * NF)
            c = gather_cfg(LPV, otf, 4, min(chunk, n), NF, V, X, Y, Z, trace)
            note(c)
            if c.status != OK:
                recs.append(_record(j0, LPV, 4, pair, otf, casc, NF, first, min(chunk, n), c, Js, X, Y, Z, cube16, 0,
                                    c.status))
                return c.status
            for f0 in range(first, last, chunk):
                nb = min(chunk, last - f0)
                if f0 > first:
                    note(c)
                recs.append(_record(j0, LPV, 4, pair, otf, casc, NF, f0, nb, c, Js, X, Y, Z, cube16,
                                    nb * frame_bytes(V, Js, H, W, pair), OK))   # (the copy made: pairs or fp32)
            return OK

        st, done, whole = OK, 0, True
        if pair:
            cf = chunk_frames(B, V, Js, H, W, True, trace)
            if not grid_index and cf >= PAIR_FRAMES:
                done = B // PAIR_FRAMES * PAIR_FRAMES
                st = run_chunks(0, done, PAIR_FRAMES)
                whole = False
            if st == OK and done < B and not grid_index and cf >= 2 and B - done >= 2:
                even = done + (B - done) // 2 * 2
                st = run_chunks(done, even, 2)
                done, whole = even, False
            if st == OK and done < B and not whole:
                st = run_chunks(done, B, 1)
        if whole:
            st = run_chunks(0, B, 1)
        if st != OK:
            return st, recs
    return OK, recs


def new_trace():
    return collections.defaultdict(set)


def band_class(rec_cols, band, X, Y):
    """0: not banded; 'exact': X a multiple of the band; 'short': a short last band
    with at least two column groups per x-row (where a wrong row count shows)."""
    if not band:
        return 0
    if X % band == 0:
        return "exact"
    return "short" if Y // rec_cols >= 2 else "short1"
