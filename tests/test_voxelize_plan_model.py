"""CPU: fvp_voxelize_plan -- the voxelize launcher's own walk, recording instead of
launching -- against the independent restatement of its rules in
voxelize_plan_model.py, over a few hundred thousand argument sets, with both
sides of every threshold reached, and the branches no argument set reaches pinned."""
import itertools
import random

import pytest

import voxelize_plan_model as M
from fvp import _lib, ops

SMALL_HW = (48, 64)  # (H, W)


def _sets():
    """The sweep: a dense random sample of the argument space plus directed sets around every threshold."""
    rnd = random.Random(20240611)
    zs = [1, 2, 3, 4, 5, 7, 8, 12, 16, 20, 31, 32, 33, 63, 64, 100, 127, 128, 129, 255, 256, 257]
    js = [1, 4, 5, 8, 9, 15, 16, 17, 32, 33, 40, 64, 65]
    vs = [1, 2, 3, 5, 8, 15, 16, 17, 31, 32, 33, 48]
    bs = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 24, 25]
    big_xy = [(63, 65), (64, 64), (65, 63), (4095, 1), (1, 4096), (80, 80), (128, 128), (160, 160), (72, 60), (17, 256),
              (100, 63), (128, 34), (32, 128), (63, 66), (65, 64), (43, 128), (273, 15), (91, 45), (64, 65), (17, 241)]
    hws = [SMALL_HW] * 6 + [(128, 240), (128, 192), (128, 255), (128, 383), (256, 480), (512, 960)]
    for _ in range(260000):
        kind = rnd.choice(M.KINDS)
        X, Y = (rnd.randint(1, 96), rnd.randint(1, 96)) if rnd.random() < 0.6 else rnd.choice(big_xy)
        J = rnd.choice(js)
        cp = 0 if kind.startswith("planar") else (J + 7) // 8 * 8 + rnd.choice([0, 0, 8])
        H, W = rnd.choice(hws)
        yield (kind, rnd.random() < 0.5, rnd.choice(bs), rnd.choice(vs), J, H, W, X, Y, rnd.choice(zs), cp,
               rnd.random() < 0.2, rnd.random() < 0.8)
    # directed: X*Y at 4095 / 4096, the block-count thresholds, tall columns up to the LDS limit, the chunk budgets
    for kind, otf, (X, Y), Z, J in itertools.product(M.KINDS, (False, True), [(4095, 1), (1, 4095), (64, 64), (65, 63)],
                                                     (1, 20, 64), (4, 15, 32)):
        yield (kind, otf, 1, 5, J, *SMALL_HW, X, Y, Z, 32, False, True)
    for kind, otf, XY, B, Z, J in itertools.product(M.KINDS, (False, True), (1023, 1024, 2048, 2049), (1, 2, 8),
                                                    (1, 33, 64, 128, 256), (4, 8, 16, 32)):
        for X, Y in ((XY, 1), (1, XY)) + (((XY // 31, 31),) if XY % 31 == 0 else ((XY // 32, 32),) if XY % 32 == 0
                                          else ()):
            yield (kind, otf, B, 5, J, *SMALL_HW, X, Y, Z, 32, False, True)
    for kind, otf, Z, B, J in itertools.product(M.KINDS, (False, True), (320, 639, 640, 641, 1279, 1280, 1281, 2560, 5000),
                                                (1, 2, 4, 8), (8, 15, 17, 32)):
        yield (kind, otf, B, 17, J, *SMALL_HW, 3, 5, Z, 32, False, True)
    for kind, (H, W), V, B, J, gi in itertools.product(("planar_f32", "planar_f16"),
                                                       [(128, 192), (128, 255), (128, 383), (128, 511), (128, 512),
                                                        (128, 1023), (128, 1024), (256, 1024), (512, 1919), (512, 1920)],
                                                       (16, 17), (1, 2, 3, 5, 7, 8, 9, 16), (5, 15, 17, 33), (False, True)):
        yield (kind, False, B, V, J, H, W, 20, 20, 8, 0, gi, True)
    for bad in [("planar_f32", False, 0, 5, 15, 48, 64, 8, 8, 4, 0, False, True),
                ("planar_f32", False, 1, 256, 15, 48, 64, 8, 8, 4, 0, False, True),
                ("planar_f32", False, 1, 5, 1025, 48, 64, 8, 8, 4, 0, False, True),
                ("planar_f32", False, 1, 5, 15, 1, 64, 8, 8, 4, 0, False, True),
                ("planar_f32", False, 1, 32, 15, 48, 64, 1024, 1024, 512, 0, False, True),
                ("cl_f32", False, 1, 5, 15, 48, 64, 8, 8, 4, 12, False, True),
                ("cl_f32", True, 1, 5, 33, 48, 64, 8, 8, 4, 32, False, True),
                ("cl_f16", False, 1, 5, 15, 48, 64, 8, 8, 4, 12, False, True),
                ("cl_f16", True, 1, 5, 17, 48, 64, 8, 8, 4, 16, False, True)]:
        yield bad


@pytest.fixture(scope="module")
def sweep():
    """One pass over the sweep: the mismatches, the trace of every comparison, and what the plans contained."""
    import ctypes

    lib = _lib.load()
    nf = len(ops.GatherLaunch._fields)
    cap = 256
    buf = (ctypes.c_longlong * (cap * nf))()
    n = ctypes.c_int(0)
    trace = M.new_trace()
    seen = {"sets": 0, "bad": [], "first_nf": set(), "groupings": set(), "status": set(), "launches": 0,
            "inst": set(), "ws_short": [], "branch_lpv": set()}
    for a in _sets():
        kind, otf, B, V, J, H, W, X, Y, Z, cp, gi, al = a
        st = lib.fvp_voxelize_plan(M.KINDS.index(kind), int(otf), cp, B, V, J, H, W, X, Y, Z, int(gi), int(al), buf, cap,
                                   ctypes.byref(n))
        assert n.value <= cap, a
        got = [tuple(buf[i * nf:(i + 1) * nf]) for i in range(n.value)]
        classes = []
        want_st, want = M.plan(kind, otf, B, V, J, H, W, X, Y, Z, cp, gi, al, trace, classes)
        assert len(classes) == len(want)
        seen["branch_lpv"].update((branch, r[2]) for (branch, _), r in zip(classes, want))
        seen["sets"] += 1
        seen["status"].add(st)
        seen["launches"] += len(got)
        if (st, got) != (want_st, want):
            seen["bad"].append((a, st, got, want_st, want))
            continue
        for r in map(ops.GatherLaunch._make, got):
            seen["inst"].add((r.family, r.lpv, r.pair, r.casc, r.nf))
        if kind == "planar_f16" and J <= 16 and got:
            seen["groupings"].add((min(B, 4), bool(gi), tuple(dict.fromkeys(r[6] for r in got))))
        if kind.startswith("planar") and st == 0:
            ws = (lib.fvp_voxelize_f16_workspace_bytes if kind == "planar_f16" else lib.fvp_voxelize_workspace_bytes)(
                B, V, J, H, W)
            if max(r[21] for r in got) > ws:
                seen["ws_short"].append((a, ws, max(r[21] for r in got)))
    return trace, seen


def test_query_equals_model_over_the_sweep(sweep):
    trace, seen = sweep
    assert seen["sets"] >= 250000 and seen["launches"] >= 300000
    assert not seen["bad"], f"{len(seen['bad'])} mismatches, first: {seen['bad'][0]}"
    assert seen["status"] == {0, 1002}


def test_all_40_instantiations_occur(sweep):
    """(family, LPV, PAIR, CASC, NF): 16 fp32-table kernels (2 families x LPV 1/2/4/8 x CASC), 12 pair-table
    (2 families x NF 1/2/4 x CASC), 12 fp16-in-place (2 families x LPV 1/2/4 x CASC)."""
    inst = sweep[1]["inst"]
    want = {(f, l, 0, c, 1) for f in (1, 2) for l in (1, 2, 4, 8) for c in (0, 1)}
    want |= {(f, 4, 1, c, n) for f in (1, 2) for n in (1, 2, 4) for c in (0, 1)}
    want |= {(f, l, 0, c, 1) for f in (3, 4) for l in (1, 2, 4) for c in (0, 1)}
    assert len(want) == 40 and inst == want


def test_both_sides_of_every_threshold(sweep):
    trace, _ = sweep
    assert {4095, 4096} <= trace["xy"]
    assert {1023, 1024} <= trace["blocks_1024"] and {2048, 2049} <= trace["blocks_2048"]
    assert {31, 32, 255, 256} <= trace["z"]
    assert trace["snap_half"] == {-1, 0, 1}            # 2 * cc < c, == c, > c
    assert trace["stage_20480"] == {False, True}       # within 64 B of the threshold, either side
    assert trace["lds_160k"] == {False, True}
    assert {16, 17} <= trace["v"]
    assert {4, 5, 8, 9, 16, 17, 32, 33} <= trace["j"]
    assert trace["budget_f32"] == {0, 1, 2} and trace["budget_pairs"] == {0, 1, 2}
    assert trace["pair_bump"] == {False, True}


def test_stage_pitch_at_exactly_20480_bytes():
    """padded == 20480 keeps the pad, tight == 20480 drops it (C4: 8 columns of 32, LPV 4 -> 16 x 4 x 320 = 20480)."""
    assert M.stage_pitch(4, 79, 4) == 320 and M.stage_pitch(4, 8, 40) == 320 and M.stage_pitch(4, 80, 4) == 320
    assert M.stage_pitch(4, 78, 4) == 316 and M.stage_pitch(4, 81, 4) == 328


def test_unreachable_pair_grouping(sweep):
    """run_frames' pair branch `workspace holds >= 2 but < 4 frames` only ever sees B = 2 or 3: chunk_frames
    returns (before the clip to B) 1 or >= 4 for pairs, since 128 MB / per >= 2 implies 4 * per <= 256 MB.
    So a batch of 4 or more frames never starts with pairs of frames: it starts at NF = 4, or -- a frame
    beyond 128 MB, or grid_index given -- runs frame by frame."""
    groupings = sweep[1]["groupings"]
    assert {g for g in groupings if g[0] == 4 and not g[1]} == {(4, False, t) for t in
                                                                [(4,), (4, 2), (4, 1), (4, 2, 1), (1,)]}
    assert {g[2] for g in groupings if g[1]} == {(1,)}                      # grid_index: NF = 1
    assert {g[2] for g in groupings if g[0] in (2, 3) and not g[1]} == {(2,), (2, 1), (1,)}
    for per in range(1, 300):  # the arithmetic, in MB
        c = 128 // per
        assert not (2 <= c < 4) or 4 * per <= 256


def test_two_passes_never_at_one_lane_per_voxel(sweep):
    """gather_cfg's two-pass branch needs more than 2048 one-pass blocks after fewer than 1024 throughput blocks.
    At one lane per voxel a one-pass block holds 256 / Z columns and a throughput block at least half as many
    (160 / Z or 256 / Z, 128 / Z on the fly at 4 frames per entry -- which is never at one lane), so there are
    at most about twice as many one-pass blocks: no launch of the sweep takes two passes at LPV 1, every other
    (branch, LPV) occurs.  The branch stays in the code."""
    got = sweep[1]["branch_lpv"]
    assert got == {(b, l) for b in ("throughput", "one", "two") for l in (1, 2, 4, 8)} - {("two", 1)}


def test_every_launch_fits_the_workspace(sweep):
    """What a gather launch reads of the workspace (and its layout pass wrote) is within
    fvp_voxelize*_workspace_bytes for the call."""
    short = sweep[1]["ws_short"]
    assert not short, f"{len(short)} calls overrun their workspace, first: {short[0]}"
