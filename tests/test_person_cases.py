"""CPU: the per-person gather's case table (person_cases.py) covers what it claims, its
inputs can show a fault, its stand-in reference is the oracle's, and fvp_person_plan -- the
decision function the launcher calls -- equals a Python model of the rules.  The GPU run
of the table is test_gpu_person_routes.py."""
import itertools

import numpy as np
import pytest
import torch

import person_cases as PC
from fvp import ops
from oracle import fvp_oracle as O

FILL = 0.90  # least share of nonzero in-window voxels, and of distinct in-window values per joint: a condition on
#              the inputs (a case that misses it gets other inputs), not a tolerance
CASES = PC.build()
RUN = [c for c in CASES if not PC.error_of(c)]


def _inputs_of(c):
    return c._replace(place="window" if c.place == "window" else "", cls=(), otf=False, want="",
                      kind="cl_f16" if PC.is_half(c) else "planar")


INPUTS = list(dict.fromkeys(_inputs_of(c) for c in RUN))   # the distinct (heatmaps, proposals) sets of the table


def _input_id(c):
    return f"{'f16' if PC.is_half(c) else 'f32'}-B{c.B}V{c.V}J{c.J}-{'x'.join(map(str, c.bins))}-P{c.P}" \
           f"{'-order' if c.frames else ''}{'-window' if c.place else ''}"


def test_table_covers_every_class():
    inst, split, direct, zs = set(), set(), set(), set()
    for c in CASES:
        st, recs = PC.plan_of(c)
        assert st == PC.error_of(c), (c, st)
        if st:
            assert recs == []
            continue
        r = recs[0]
        assert all((q.xsplit, q.zsplit, q.xy_direct, q.blocks, q.zeroed_planes, q.casc, q.otf, q.jpl, q.layout) ==
                   (r.xsplit, r.zsplit, r.xy_direct, r.blocks, r.zeroed_planes, r.casc, r.otf, r.jpl, r.layout)
                   for q in recs), recs
        assert r.zeroed_planes == (0 if c.want == "cubes" else 3 if r.xsplit > 1 else 2)
        assert r.layout == int(c.kind in ("planar", "cams")) and r.otf == int(c.otf) and r.casc == int(c.V > 16)
        if c.place == "inst":
            assert c.cls == PC.inst_of(r) + (4, 1, 0) and len(recs) == 1
            inst.add((PC.inst_of(r), c.want))
        if c.place == "split":
            split.add((r.xsplit, c.want))
            if r.xsplit == 1 and c.want != "cubes":   # 8 lanes per voxel (fp32, 17 .. 32 joints) keep the atomics
                assert r.xy_direct == int(not (c.kind == "cl" and c.J == 30)), c
        direct.add(r.xy_direct)
        zs.add(r.zsplit)
        if c.place == "slices":
            assert [q.j0 for q in recs] == list(range(0, c.J, 32))
            if c.J in (33, 40):
                assert recs[0].lpv != recs[-1].lpv, recs
        if c.place == "depth":
            assert r.zsplit == -(-c.bins[2] // 64) and (r.zsplit > 1 or c.bins == (9, 5, 3)), c
    want_inst = {((4, lpv, otf, casc), w) for lpv in (1, 2, 4, 8) for otf in (0, 1) for casc in (0, 1)
                 for w in ("cubes", "planes")}
    want_inst |= {((8, lpv, 0, casc), w) for lpv in (1, 2, 4) for casc in (0, 1) for w in ("cubes", "planes")}
    assert inst == want_inst and len(want_inst) == 44
    assert split == set(itertools.product((1, 2, 4), ("cubes", "planes", "both")))
    assert direct == {0, 1} and zs == {1, 2, 3}
    assert {c.place for c in CASES} == {"inst", "split", "depth", "slices", "cams", "frames", "window"}
    # the planar and the channels-last input both feed the cached-grid fp32 kernel
    assert {c.kind for c in CASES if c.place == "inst"} == set(ops.PERSON_KINDS)
    # x ranges that do not divide, parts with an empty x range, and the last x slot of the LDS table
    shapes = {(c.bins[0], PC.plan_of(c)[1][0].xsplit) for c in RUN if c.place == "split"}
    assert {(7, 4), (3, 4), (2, 4), (64, 1), (8, 1), (8, 2), (8, 4)} <= shapes
    assert len({PC.case_id(c) for c in CASES}) == len(CASES)


def test_plan_model_equals_the_query():
    """person_cases.model_plan == fvp_person_plan over a sweep of P, S, J, V, kind and want, with values either
    side of 1024 and 4096 rows, 64 deep, 4 / 8 / 16 / 32 joints, 16 and 64 cameras, and the argument errors."""
    n = 0
    seen = set()
    Ps = (0, 1, 8, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 513)
    Ss = (1, 2, 7, 8, 32, 63, 64, 65, 128, 129, 4096, 4097)
    Js = (1, 4, 5, 8, 9, 16, 17, 32, 33, 40, 64, 65, 1024, 1025)
    Vs = (1, 2, 16, 17, 64, 65, 255, 256)
    rng = np.random.default_rng(5)
    points = list(itertools.product(ops.PERSON_KINDS, Ps, Ss, (4, 16, 33), (5, 17), (False, True)))
    points += list(itertools.product(ops.PERSON_KINDS, (8, 64), (8, 64), Js, Vs, (False, True)))
    for kind, P, S, J, V, planes in points:
        bins = (S, S, S) if rng.integers(0, 8) else (S, max(1, S - 1), S)
        fine = tuple(2 * b - 1 for b in bins) if rng.integers(0, 16) else (1, 5, 5)
        cp = 0 if kind in ("planar", "cams") else int(rng.choice([(J + 15) // 16 * 16, (J + 7) // 8 * 8,
                                                                  (J + 3) // 4 * 4, J, 0, 12, 32]))
        aligned = bool(rng.integers(0, 8))
        B = 1 if rng.integers(0, 16) else 0
        H, W = (48, 64) if rng.integers(0, 16) else (1, 64)
        st, recs = ops.person_plan(kind, B, V, J, H, W, bins, fine, P, want_cubes=not planes or bool(rng.integers(0, 2)),
                                   want_planes=planes, cp=cp, aligned=aligned)
        mst, mrecs = PC.model_plan(kind, cp, B, V, J, H, W, bins, fine, P, planes, aligned)
        assert (st, [tuple(r) for r in recs]) == (mst, mrecs), (kind, P, bins, fine, J, V, planes, cp, aligned, B, H)
        n += 1
        if recs:
            seen.add((recs[0].xsplit, min(recs[0].zsplit, 3), recs[0].xy_direct, recs[0].lpv, recs[0].casc))
        seen.add(st)
    assert n >= 3000 and {0, PC.ERR_SHAPE} <= seen
    assert {k[0] for k in seen if isinstance(k, tuple)} == {1, 2, 4} and {k[2] for k in seen if isinstance(k, tuple)} == {0, 1}
    # the packed fine grid beyond 32-bit byte offsets, and pixels beyond 2 GB
    big = (1024, 1024, 512)
    for kind in ops.PERSON_KINDS:
        got = ops.person_plan(kind, 1, 8, 15, 48, 64, (8, 8, 8), big, 8, cp=16)
        assert (got[0], [tuple(r) for r in got[1]]) == PC.model_plan(kind, 16, 1, 8, 15, 48, 64, (8, 8, 8), big, 8, False)
        assert (got[0] == 0) == (kind == "cams")
    assert ops.person_plan("cl", 1, 5, 15, 16384, 16384, (8,) * 3, (15,) * 3, 8, cp=16)[0] == PC.ERR_SHAPE
    assert PC.model_plan("cl", 16, 1, 5, 15, 16384, 16384, (8,) * 3, (15,) * 3, 8, False)[0] == PC.ERR_SHAPE


def test_individual_constants_are_the_oracles():
    """The constants person_cases builds for the non-cubic volumes are the oracle's (held on cubic ones)."""
    for bins, ind in (((8,) * 3, (1000.0,) * 3), ((65,) * 3, (1500.0,) * 3), ((7,) * 3, (1000.0,) * 3)):
        w = PC.workload(bins, 1, ind)
        a, b = PC._Individual(w.space_size, w.space_center, ind, bins), O.Individual(w.space_size, w.space_center, ind, bins)
        for name in ("wc", "ws", "isz", "vpa", "fine", "scale", "bias"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert np.array_equal(a.fine_bins, b.fine_bins)
    assert tuple(PC.individual((8,) * 3, (1000.0,) * 3).fine_bins) == (15, 15, 15)
    assert tuple(PC.individual((5, 3, 130), (1000.0,) * 3).fine_bins) == (9, 5, 259)


@pytest.mark.parametrize("c", INPUTS, ids=_input_id)
def test_inputs_can_show_a_fault(c):
    """Per set of inputs, from the reference alone: at least 0.90 of the voxels inside the windows of the
    proposals that are not skipped are nonzero, per joint at least 0.90 of a window's values are distinct, none
    is saturated at 1, and the proposals hold a full, a low-clipped, a high-clipped and a skipped window."""
    fill, distinct, at_one = PC.fill_of(c)
    print(f"fill {fill:.3f} distinct {distinct:.3f}")
    assert fill >= FILL and distinct >= FILL and not at_one, (fill, distinct, at_one)
    cl = PC.classes(c)
    assert "skipped" in cl and any(k.startswith("full") for k in cl), cl
    assert any(k.startswith("clipped") and " low" in k for k in cl) and \
        any(k.startswith("clipped") and " high" in k for k in cl), cl
    props = PC.proposals(c)
    assert props.shape == (c.P, 7) and np.isfinite(props).all()
    planted = 0 if c.P < 6 else 4   # the row with both bbox entries above 1: negative margin -> 0, a full window
    assert props[planted, 5] > 1 and props[planted, 6] > 1 and cl[planted] == "full", (props[planted], cl[planted])
    ctl, _, start, end = PC.individual(c.bins, PC.ind_size(c)).windows(props)
    o = PC.individual(c.bins, PC.ind_size(c))
    inside = np.all((ctl >= 0) & (ctl + np.array(c.bins) <= o.fine_bins), axis=1)
    assert any(inside[i] and cl[i] == "skipped" for i in range(c.P)), "no window emptied by its margins alone"
    cubes, _ = PC.reference(c)
    assert not cubes[~PC.in_window_mask(c)[:, None].repeat(c.J, 1)].any()


def test_window_cases_have_their_ties():
    for c in (c for c in CASES if c.place == "window"):
        o = PC.individual(c.bins, PC.ind_size(c))
        rows, ties = PC.window_proposals(c)
        props = PC.proposals(c)
        assert np.array_equal(props[6:6 + len(rows)], rows)
        ctl, _, start, end = o.windows(rows)
        S, F = np.array(c.bins), o.fine_bins
        assert sorted((a, k % 2) for _, a, k in ties) == [(a, par) for a in range(3) for par in (0, 1)]
        for i, a, k in ties:
            sc, bi = np.float32(o.scale[a].item()), np.float32(o.bias[a].item())
            assert np.float32(np.float32(rows[i, a] * sc) + bi) == np.float32(k + 0.5)
            t = torch.tensor(rows[i, a]) * o.scale[a] + o.bias[a]           # the oracle's own arithmetic
            assert t.item() == k + 0.5 and ctl[i, a] == (k if k % 2 == 0 else k + 1)   # round half to even
        for a in range(3):
            assert any(ctl[i, a] == -S[a] + 1 and end[i, a] - start[i, a] == 1 for i in range(len(rows)))
            assert any(ctl[i, a] == F[a] - 1 and end[i, a] - start[i, a] == 1 for i in range(len(rows)))
            assert any(ctl[i, a] + S[a] == F[a] == end[i, a] for i in range(len(rows)))


@pytest.mark.parametrize("c", INPUTS, ids=_input_id)
def test_sliced_reference_is_person_cubes(c):
    """The stand-in for many proposals (the fine grid voxelized once, windows cut out) equals
    Individual.person_cubes bit for bit: for every case whose reference is person_cubes itself (at most 16
    proposals, and the window cases) on all rows, and for 16 proposals sampled from each larger one."""
    cubes, offset = PC.reference(c)
    if not PC.uses_sliced(c):
        got, off = PC.sliced_reference(c)
        rows = np.arange(c.P)
    else:
        rows = np.sort(np.random.default_rng(c.P).choice(c.P, 16, replace=False))
        got, off = PC.direct_reference(c, rows)
    assert np.array_equal(got, cubes[rows]) and np.array_equal(off, offset[rows])
    assert got.any()


def test_nan_max_is_torch_max():
    """person_cases.nan_max (NaN wins, the first of equal values is kept) against torch.max on the CPU, on signed
    values with infinities, both zeros and NaN, bit for bit -- including the sign of a zero maximum wherever it
    is defined (person_cases.zero_sign_defined: all zeros of the line share one sign).  Only where a line holds
    both +0 and -0 as its maximum does torch's choice depend on the order it visits them (vectorised or not):
    those cells alone are compared with ==."""
    rng = np.random.default_rng(3)
    for S in (1, 2, 3, 7, 33, 65):
        a = rng.standard_normal((2, 3, S, S, S)).astype(np.float32)
        flat = a.reshape(-1)
        idx = rng.choice(flat.size, min(flat.size, 40), replace=False)
        flat[idx] = np.resize(np.array([-np.inf, np.inf, -0.0, 0.0, np.nan], np.float32), len(idx))
        if S >= 3:   # zero maxima of a defined sign (all -0.0; -0.0 above negatives; +0.0 alone) and of both signs
            a[0, 0, 0, :, :] = -1 - rng.random((S, S)).astype(np.float32)
            a[0, 0, 0, 0, :] = -0.0
            a[0, 0, 0, 1, 0] = -0.0
            a[0, 0, 0, 2, 1] = 0.0
            a[0, 0, 0, 1, 2], a[0, 0, 0, 2, 2] = 0.0, -0.0
        for axis in (2, 3, 4):
            ref = torch.max(torch.from_numpy(a), dim=axis)[0].numpy()
            got = PC.nan_max(a, axis)
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            ok = ~np.isnan(ref)
            assert np.array_equal(got[ok], ref[ok])
            exact = ok & ((ref != 0) | PC.zero_sign_defined(a, axis))
            assert np.array_equal(got[exact].view(np.uint32), ref[exact].view(np.uint32))
            if S >= 3:
                assert (exact & (ref == 0) & np.signbit(ref)).any() or axis == 2, "no -0.0 maximum of a defined sign"
                assert (ok & ~exact).any() or axis != 3, "no zero maximum of both signs"
    c = np.zeros((1, 1, 2, 2, 2), np.float32)
    assert np.array_equal(PC.nan_max_planes(c), O.max_planes(c))
