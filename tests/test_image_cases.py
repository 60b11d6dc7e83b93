"""CPU: the case table of the heatmap sizes and image borders (image_cases.py) reaches every
class it names, each case's pair-table layout kernel from the query (fvp_pair_layout_kind)
is the one the model (image_ref.pair_layout_model) gives and the one the case stands for,
the planted grids hit every reachable one of the 25 tap classes, the projected grids every x
class projection can give, no case is trivially passable, and the numpy table builders
decode back to their heatmaps."""
import collections
import itertools

import numpy as np
import pytest

import image_cases as IC
import image_ref as R
from fvp import ops

MAX_CASES = 370
FILL, DISTINCT = 0.60, 0.50   # lower than the route tables' 0.90: these inputs are off-image on purpose


def test_table_size_and_ids():
    cases = IC.build()
    assert len(cases) <= MAX_CASES
    ids = [IC.case_id(c) for c in cases]
    assert len(set(ids)) == len(ids)
    counts = collections.Counter(c.place for c in cases)
    print(len(cases), dict(counts))
    assert set(counts) == {"pairs", "joints", "layout", "border", "border_otf", "columns"}
    assert all(c.bins in IC.GRIDS for c in cases)


def test_model_equals_query_on_a_sweep():
    """Every (NF, W <= 1100, address mod 16), at two address magnitudes."""
    n = 0
    for nf, W, a in itertools.product((1, 2, 4), range(2, 1101), range(16)):
        for base in (0, 0x7F0000001000):
            assert ops.pair_layout_kind(nf, W, base + a) == R.pair_layout_model(nf, W, base + a), (nf, W, a)
            n += 1
    assert n == 3 * 1099 * 16 * 2
    assert ops.pair_layout_kind(3, 64, 0) == -1 and ops.pair_layout_kind(4, 1, 0) == -1
    # the witnesses the table is built around
    assert R.pair_layout_model(4, 508, 4) == R.ROWS and 4 * 16 * (508 // 2 + 2) * 4 == 65536
    assert R.pair_layout_model(4, 510, 4) == R.ENTRY and R.pair_layout_model(2, 510, 4) == R.ROWS
    assert R.pair_layout_model(4, 8, 0) == R.VEC8 and R.pair_layout_model(1, 10, 0) == R.ENTRY
    assert 4 * 16 * (130 // 2) > 256 * 16   # W = 130, NF = 4, J = 16: a second trip of pairs_rows_kernel's load loop


def test_pair_layout_classes():
    """Every (NF, W, address class) is a case on the kernel the choice gives it; each case's kernel
    from the query equals the model and is the one its class names; its plan is one launch of B frames per
    entry over the whole batch."""
    cases = [c for c in IC.build() if c.place in ("pairs", "joints")]
    for c in cases:
        k = IC.layout_of(c)
        assert k == R.pair_layout_model(c.B, c.hm[0], c.amod) and R.LAYOUT_NAMES[k] == c.cls[0], c
        recs = IC.plan_of(c)
        assert len(recs) == 1 and (recs[0].pair, recs[0].nf, recs[0].nb) == (1, c.B, c.B), (c, recs)
        assert recs[0].tab_bytes == c.B * c.V * c.hm[1] * (c.hm[0] + 1) * 64
    assert {c.cls for c in cases if c.place == "pairs"} == {
        (R.LAYOUT_NAMES[R.pair_layout_model(nf, W, a)], nf, W, a)
        for nf, W, a in itertools.product((4, 2, 1), IC.WIDTHS, IC.AMODS)}
    assert {c.cls[0] for c in cases} == set(R.LAYOUT_NAMES)
    by = {c.cls: c for c in cases if c.place == "pairs"}
    assert any(k[:3] == ("rows", 4, 508) for k in by) and any(k[:3] == ("entry", 4, 510) for k in by)
    assert not any(k[:3] == ("rows", 4, 510) for k in by)
    assert any(k[:3] == ("vec8", 4, 8) for k in by)
    assert {c.J for c in cases if c.cls[:3] == ("rows", 4, 130)} == {16}
    assert {c.hm[1] for c in cases if c.place == "pairs"} == {2, 3, 33}
    assert all((c.V, c.hm[1], c.bins) == (1, 2, (7, 5, 3)) for c in cases if c.hm[0] >= 128)
    assert {c.cls for c in cases if c.place == "joints"} == {
        (k, J) for k in R.LAYOUT_NAMES for J in (1, 3, 4, 5, 8, 13, 16)}
    assert all(c.B == 4 for c in cases if c.place == "joints")


def test_layout_border_and_columns_classes():
    cases = IC.build()
    lay = [c for c in cases if c.place == "layout"]
    inst = set()
    for c in lay:
        recs = IC.plan_of(c)
        assert all(r.pair == 0 and r.nf == 1 and r.nb == 1 and r.tab_bytes > 0 for r in recs), (c, recs)
        inst |= {(r.lpv, c.kind, c.hm) for r in recs}
        assert [r.j0 for r in recs] == ([0, 32] if c.J == 33 else [0])
    sizes = {(61, 33), (45, 31), (2, 2), (10, 6)}
    assert {(l, k, s) for l in (1, 2, 4, 8) for s in sizes for k in ("planar_f32",)} | \
        {(8, "planar_f16", s) for s in sizes} | {(1, "planar_f16", (45, 31))} == inst
    assert any(c.V * c.hm[0] * c.hm[1] * r.lpv % 256 for c in lay for r in IC.plan_of(c))
    assert any(c.J == 33 and (c.hm[0] * c.hm[1]) % 2 for c in lay)

    bor = [c for c in cases if c.place == "border"]
    kinds = set()
    for c in bor:
        r = IC.plan_of(c)[0]
        kinds.add((c.kind, r.lpv, r.nf))
    assert kinds == {("planar_f32", l, 1) for l in (1, 2, 4, 8)} | {("planar_f16", 4, n) for n in (4, 2, 1)} | \
        {("cl_f32", 4, 1)} | {("cl_f16", l, 1) for l in (1, 2, 4)}
    assert {(c.kind, c.B, c.J, c.hm, c.V) for c in bor} == {
        (k, b, j, s, V) for (k, b, j) in {(c.kind, c.B, c.J) for c in bor} for s in IC.PLANTED_SIZES for V in (5, 17)}
    assert len({(c.kind, c.B, c.J) for c in bor}) == 11
    assert any(c.hm[0] >= 128 and float(R.sample_px(-1.1, c.hm[0])) < -4 for c in bor)   # below tap_origin's clamp

    otf = [c for c in cases if c.place == "border_otf"]
    assert {(c.kind, c.hm) for c in otf} == {(k, s) for k in ("planar_f32", "planar_f16", "cl_f32", "cl_f16")
                                             for s in IC.PORTRAIT_SIZES}
    assert all(IC.plan_of(c)[0].otf == 1 for c in otf)

    col = [c for c in cases if c.place == "columns" and c.cls[0] != "grid_index"]
    assert {c.cls[:4] for c in col} == {(h, o, V > 16, V) for h in (False, True) for o in (False, True)
                                        for V in IC.COLUMN_VIEWS}
    assert {(c.cls[0], c.cls[1], c.cls[2], c.cls[4]) for c in col} == set(
        itertools.product((False, True), (False, True), (False, True), ("planar", "cl")))
    assert {c.cls for c in cases if c.place == "columns" and c.cls[0] == "grid_index"} == {
        ("grid_index", False), ("grid_index", True)}
    for c in col:
        flat = IC.flat_of(c)
        X, Y, _ = c.bins
        assert all(sorted(f[:-2]) == list(range(X * Y)) and tuple(f[-2:]) == (-1, X * Y) for f in flat)


def test_tap_classes_of_the_planted_grids():
    """Every reachable one of the 25 (x class, y class) pairs at least 4 times per camera; what cannot be
    reached within [-2, 2] is exactly: t < -1 and t > n - 1 on an axis of 2 pixels, t < -1 on an axis of 3."""
    assert R.unreachable(2) == ["below", "beyond"] and R.unreachable(3) == ["below"]
    assert all(R.unreachable(n) == [] for n in (4, 6, 10, 33, 48, 61, 64, 130, 510))
    seen = set()
    for c in IC.build():
        if c.src != "planted":
            continue
        for seq in set(IC.seqs_of(c)):
            sg = IC.sample_grid(c, seq)
            key = (c.V, sg.shape[1], c.hm, seq)
            if key in seen:
                continue
            seen.add(key)
            assert np.isfinite(sg).all() and np.abs(sg).max() <= 2
            tc = R.tap_classes(sg, *c.hm)
            rx = [i for i in range(5) if R.CLASS_NAMES[i] not in R.unreachable(c.hm[0])]
            ry = [i for i in range(5) if R.CLASS_NAMES[i] not in R.unreachable(c.hm[1])]
            assert tc[:, rx][:, :, ry].min() >= R.PER_PAIR, (key, tc.min(axis=0))
            assert tc.sum() == tc[:, rx][:, :, ry].sum()
            pts = {tuple(p) for p in sg[0].tolist()}   # the exact border and padding coordinates
            for p in R.SPECIALS[:R.MIN_SPECIALS]:
                assert tuple(np.float32(p).tolist()) in pts, (key, p)
    assert len(seen) >= 40
    # fractional parts at a border tap: 0, .25, .5 and the largest fp32 below the next integer
    for n in (10, 33, 64):
        fr = [float(R.sample_px(g, n)) - (n - 1) for g in R.axis_candidates(n)[R.LAST]]
        assert fr[0] == 0 and abs(fr[1] - 0.25) < 1e-4 and abs(fr[2] - 0.5) < 1e-4 and 1 - 1e-4 < fr[3] < 1
        g = R.axis_candidates(n)[R.LAST][3]
        assert R.axis_class(np.nextafter(g, np.float32(9)), n) == R.BEYOND   # the largest: the next fp32 is past it
    # g == -1 and g == +1 exactly: ix == 0 and ix == n - 1
    for n in (2, 3, 10, 61, 64, 130, 510):
        assert float(R.sample_px(-1.0, n)) == 0 and float(R.sample_px(1.0, n)) == n - 1


# What projection reaches (oracle.fvp_oracle.project_grid on the portrait image): never t < -1 -- pixel
# coordinates are clipped at -1 before the resize transform, which lands in t == -1 -- and at 6 pixels the
# clip at the other side (pixel 1920 -> 6.0 before the division by W - 1) rounds into t == W - 1.
PROJECTED_X = {48: {"minus1", "inside", "last", "beyond"}, 33: {"minus1", "inside", "last", "beyond"},
               6: {"minus1", "inside", "last"}}


def test_tap_classes_of_the_projected_grids():
    """Every x class projection can give has at least 8 samples per case; corners (both axes off the image)
    are unreachable by projection (y is letter-boxed on the portrait image): asserted, the planted cases have
    them."""
    n = 0
    for c in IC.build():
        if c.src != "portrait":
            continue
        n += 1
        tc = sum(R.tap_classes(IC.sample_grid(c, s), *c.hm) for s in set(IC.seqs_of(c))).sum(axis=0)
        x = tc.sum(axis=1)
        assert {R.CLASS_NAMES[i] for i in range(5) if x[i]} == PROJECTED_X[c.hm[0]], (c, x)
        assert all(x[i] >= 8 for i in range(5) if x[i]), (c, x)
        assert tc[:, [R.BELOW, R.MINUS1, R.LAST, R.BEYOND]].sum() == 0, (c, tc)   # y stays inside: no corner
    assert n >= 12 + 16


def test_no_case_is_trivially_passable():
    worst = {}
    for c in IC.build():
        ref = IC.oracle_cube(c)
        N = ref[0, 0].size
        fill = min(np.count_nonzero(ref[b]) / ref[b].size for b in range(c.B))
        distinct = min(len(np.unique(ref[b, j])) / N for b in range(c.B) for j in range(c.J))
        w = worst.get(c.place, (1.0, 1.0))
        worst[c.place] = (min(w[0], fill), min(w[1], distinct))
        assert fill >= FILL and distinct >= DISTINCT, (IC.case_id(c), fill, distinct)
    print({k: (round(a, 3), round(b, 3)) for k, (a, b) in worst.items()})


def test_table_builders_decode_back():
    rng = np.random.default_rng(5)
    for (nb, V, J, H, W), nf in itertools.product(((4, 2, 5, 3, 6), (4, 1, 16, 2, 9), (4, 3, 1, 2, 2)), (1, 2, 4)):
        hm = rng.integers(1, 0x7BFF, (nb, V, J, H, W)).astype(np.uint16)
        tab = R.pair_table(hm, nf)
        assert tab.shape == (nb // nf, V, H, W + 1, nf, 4, 2, 4) and tab.nbytes == nb * V * H * (W + 1) * 64
        back, ok = R.pair_table_decode(tab, J)
        assert ok and np.array_equal(back, hm)
        # lane q of frame f of entry (y, e): 16 B = joints 4q .. 4q + 3 of pixel e - 1, then of pixel e
        e, f, q = W // 2, nf - 1, 0
        lane = tab[0, V - 1, H - 1, e, f, q]
        for k in range(min(4, J)):
            assert lane[0, k] == hm[f, V - 1, k, H - 1, e - 1] and lane[1, k] == hm[f, V - 1, k, H - 1, e]
    for (nb, V, Jst, H, W), (j0, J, lpv) in itertools.product(((2, 3, 33, 3, 5), (1, 2, 40, 2, 2)),
                                                              ((0, 32, 8), (32, 1, 1), (3, 13, 4), (0, 7, 2))):
        hm = rng.random((nb, V, Jst, H, W)).astype(np.float32) + 0.5
        tab = R.cl_table(hm, j0, J, lpv)
        assert tab.shape == (nb, V, H * W, lpv, 4)
        back, ok = R.cl_table_decode(tab, J, H, W)
        assert ok and np.array_equal(back, hm[:, :, j0:j0 + J])
        assert tab[nb - 1, V - 1, H * W - 1].reshape(-1)[J - 1] == hm[nb - 1, V - 1, j0 + J - 1, H - 1, W - 1]


def test_fp32_table_is_never_grouped():
    """Pinned by name: heatmaps_to_cl_kernel's `NF > 1` branch (fvp_layout.h) is unreachable -- only the pair
    table groups frames (run_frames), so every non-pair launch of the plan sweep has nf == 1.  The branch stays."""
    import ctypes

    from fvp import _lib
    from test_voxelize_plan_model import _sets
    import voxelize_plan_model as M

    lib = _lib.load()
    nfld = len(ops.GatherLaunch._fields)
    cap = 256
    buf = (ctypes.c_longlong * (cap * nfld))()
    n = ctypes.c_int(0)
    launches = 0
    for kind, otf, B, V, J, H, W, X, Y, Z, cp, gi, al in _sets():
        lib.fvp_voxelize_plan(M.KINDS.index(kind), int(otf), cp, B, V, J, H, W, X, Y, Z, int(gi), int(al), buf, cap,
                              ctypes.byref(n))
        for i in range(min(n.value, cap)):
            pair, nf = buf[i * nfld + 4], buf[i * nfld + 6]
            launches += not pair
            assert pair or nf == 1, (kind, otf, B, V, J, H, W)
    assert launches >= 100000


def test_person_cases():
    """The four per-person entry kinds at two heatmap sizes, at most 12 cases: the cached kinds' windows hold
    every one of the 25 tap classes at least 4 times per camera, the projected kind's every x class projection
    gives at least 8 times; every window is the whole 8^3 volume; the construction person_cases.sliced_reference
    uses (the fine grid voxelized once, the windows cut out) equals the oracle's person_cubes on a case."""
    import person_cases as PC
    from oracle import fvp_oracle as O

    cases = IC.person_cases()
    assert len(cases) <= 12 and len({IC.person_id(c) for c in cases}) == len(cases)
    assert {(c.kind, tuple(sorted(c.hm))) for c in cases} == {(k, tuple(sorted(s))) for k in PC.ops.PERSON_KINDS
                                                              for s in IC.PERSON_SIZES}
    for c in cases:
        assert (c.bins, c.P, c.J) == ((8, 8, 8), 4, 15)
        o = IC.person_individual(c)
        ctl, _, start, end = o.windows(IC.person_proposals(c))
        assert ctl.tolist() == [list(t) for t in IC.PERSON_CTL[c.otf]] and (end - start == 8).all()
        tc = R.tap_classes(IC.person_window_samples(c), *c.hm)
        if c.otf:
            x = tc.sum(axis=(0, 2))
            assert {R.CLASS_NAMES[i] for i in range(5) if x[i]} == PROJECTED_X[c.hm[0]], (c, x)
            assert all(x[i] >= 8 for i in range(5) if x[i]), (c, x)
        else:
            assert tc.min() >= R.PER_PAIR, (c, tc.min(axis=0))
        cubes, _ = IC.person_reference(c)
        fill = np.count_nonzero(cubes) / cubes.size
        distinct = min(len(np.unique(cubes[p, j])) for p in range(c.P) for j in range(c.J)) / cubes[0, 0].size
        assert fill >= FILL and distinct >= DISTINCT, (c, fill, distinct)
    c = cases[0]
    sg = np.array(IC.person_fine_grid(c)).reshape(c.V, *IC.person_individual(c).fine_bins, 2)
    direct, off = IC.person_individual(c).person_cubes(IC.person_heatmaps(c)[0].numpy()[:, :2], sg, IC.person_proposals(c))
    cubes, offset = IC.person_reference(c)
    assert np.array_equal(direct, cubes[:, :2]) and np.array_equal(off, offset)
