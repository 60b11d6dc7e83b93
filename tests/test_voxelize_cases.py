"""CPU: the voxelize case table (voxelize_cases.py) reaches every class it names,
every case's plan is the class it stands for, the block walk of every case
(voxelize_walk.py) writes each cube and xy element exactly once inside the
packed grid, and each planted fault breaks the walk on a named case."""
import collections

import numpy as np
import pytest

import voxelize_cases as VC
import voxelize_plan_model as M
import voxelize_walk as WK

MAX_CASES = 260          # the table's stated size
MAX_SMALL_COST = 600000  # voxels x frames of every case


def test_table_size_and_ids():
    cases = VC.build()
    assert len(cases) <= MAX_CASES
    ids = [VC.case_id(c) + str(c.cls) for c in cases]
    assert len(set(ids)) == len(ids)
    assert all(VC.cost(c) <= MAX_SMALL_COST for c in cases)
    counts = collections.Counter(c.place for c in cases)
    print(dict(counts))
    assert set(counts) == {"inst", "cfg", "stage", "frames", "slices", "cams"}


def test_every_instantiation_full_and_ragged():
    got = {c.cls for c in VC.build() if c.place == "inst"}
    want = {(f, l, 0, k, 1) for f in (1, 2) for l in (1, 2, 4, 8) for k in (0, 1)}
    want |= {(f, 4, 1, k, n) for f in (1, 2) for n in (1, 2, 4) for k in (0, 1)}
    want |= {(f, l, 0, k, 1) for f in (3, 4) for l in (1, 2, 4) for k in (0, 1)}
    assert len(want) == 40
    assert got == {i + (e,) for i in want for e in ("full", "ragged")}
    for c in VC.build():
        if c.place == "inst":
            r = VC.plan_of(c)[0]
            assert VC.inst_of(r) == c.cls[:5] and (r.last_cols == r.cols) == (c.cls[5] == "full")


# gather_cfg: what the rules allow.  A small grid (X * Y < 4096) is never snapped or banded; a rejected snap
# leaves Y % cols != 0, hence no band; on a big grid an unchanged or snapped column group is banded whenever
# X > 16.
def _cfg_allowed(snap, band, X):
    if snap in ("small", "rejected") or X <= M.BAND_ROWS:
        return band == 0
    return band in ("exact", "short", "short1")


def test_gather_cfg_product():
    got = collections.defaultdict(set)
    for c in VC.build():
        if c.place == "cfg":
            assert VC.cfg_class(c) == c.cls
            lpv, otf, branch, snap, band = c.cls
            assert _cfg_allowed(snap, band, c.bins[0])
            got[(lpv, otf)].add((branch, snap, band))
    assert set(got) == {(1, False), (1, True), (8, False), (8, True)}
    need = {(b, s, d) for b in ("throughput", "one", "two") for s in ("small", "rejected") for d in (0,)}
    need |= {(b, s, d) for b in ("throughput", "one", "two") for s in ("unchanged", "snapped") for d in ("exact", "short")}
    missing = {k: sorted(need - v) for k, v in got.items() if need - v}
    print({k: len(v) for k, v in got.items()}, "missing:", missing)
    assert missing == {k: sorted(v) for k, v in UNREACHABLE_CFG.items()}


# At one lane per voxel the two-pass branch cannot be reached: it needs more than 2048 one-pass blocks of 256
# voxels (over 524,288 voxels x frames) after fewer than 1024 throughput blocks of at most 256 voxels (under
# 262,144).  Pinned by name; the branch stays in gather_cfg.
_TWO = {("two", s, d) for s, d in [("small", 0), ("rejected", 0), ("unchanged", "exact"), ("unchanged", "short"),
                                   ("snapped", "exact"), ("snapped", "short")]}
UNREACHABLE_CFG = {(1, False): _TWO, (1, True): _TWO}


def test_named_witnesses_are_what_the_issue_says():
    def first(kind, J, bins, B=1, otf=False):
        c = VC.Case("w", None, kind, otf, B, 5, J, bins, VC.HM, False, "both")
        return VC.plan_of(c)[0], VC.cfg_class(c)

    r, k = first("cl_f32", 4, (32, 128, 1))
    assert k[2:] == ("one", "snapped", "exact") or k[3:] == ("snapped", "exact"), k
    r, k = first("cl_f32", 4, (63, 66, 1))
    assert k[3:] == ("rejected", 0) and r.last_cols < r.cols, (r, k)
    r, k = first("cl_f32", 32, (72, 60, 3))
    assert r.cols == 10 and k[4] == "short", (r, k)
    r, k = first("cl_f32", 32, (17, 256, 1))
    assert k[4] == "short", (r, k)
    r, k = first("cl_f32", 32, (100, 63, 5))
    assert k[2:] == ("two", "snapped", "short"), (r, k)
    r, k = first("cl_f32", 32, (128, 34, 7))
    assert k[2:] == ("two", "rejected", 0) and r.last_cols < r.cols, (r, k)
    r, k = first("cl_f32", 32, (19, 27, 20), B=4)
    assert k[2:] == ("two", "small", 0), (r, k)


def test_stage_frames_slices_cameras_classes():
    cases = VC.build()
    st = {c.cls for c in cases if c.place == "stage" and c.cls[0] != "only"}
    for c in cases:
        if c.place == "stage" and c.cls[0] != "only":
            assert VC.stage_class(c) == c.cls
    assert {s[0] for s in st} == {"pad1", "pad4", "tight"}
    # the vector epilogue needs Z % 4 == 0, which makes every block's voxel count a multiple of 4: the full
    # blocks and the last block of a launch always take the same epilogue (no "vector, then scalar last block")
    assert {(s[1], s[2]) for s in st} == {(True, True), (False, False)}
    assert all(r.vec_full == r.vec_last for c in cases for r in VC.plan_of(c))
    assert {(s[3], s[4]) for s in st} == {(p, q) for p in (1, 2, 3) for q in (False, True)}
    assert {(s[0], s[1]) for s in st} == {(p, v) for p in ("pad4", "tight") for v in (False, True)} | {("pad1", False)}
    assert {c.cls[1:] for c in cases if c.place == "stage" and c.cls[0] == "only"} == {
        (w, k) for w in ("cube", "xy") for k in M.KINDS}
    for c in cases:
        recs = VC.plan_of(c)
        if c.place == "frames" and c.cls[0] == "groups":
            assert tuple(dict.fromkeys(r.nf for r in recs)) == c.cls[1:-1], (c, recs)
        if c.place == "frames" and c.cls[0] == "chunks":
            assert tuple(r.nb for r in recs) == c.cls[2], (c, recs)
            for j0 in sorted({r.j0 for r in recs}):   # each joint slice walks the batch from frame 0
                sl = [r for r in recs if r.j0 == j0]
                assert [r.f0 for r in sl] == [sum(q.nb for q in sl[:i]) for i in range(len(sl))] and \
                    sum(r.nb for r in sl) == c.B, (c, recs)
            assert sum(r.f0 > 0 and r.nf == recs[0].nf for r in recs) >= 1   # a second chunk of one run_chunks call
        if c.place == "slices":
            assert [r.j0 for r in recs] == [0, 32] and recs[0].lpv > recs[1].lpv, (c, recs)
            assert (recs[0].lpv, recs[1].lpv) == ((4, 1) if c.kind == "cl_f16" else (8, 1 if c.J == 33 else 2))
        if c.place == "cams":
            assert recs[0].casc == (c.V > 16)
    cams = {c.cls for c in cases if c.place == "cams"}
    assert {v for _, v, _ in cams} == {3, 6, 16, 17, 32, 33, 48}
    assert ("cl_f16", 48, False) in cams   # the parked-sum kernel over three complete 16-camera blocks


FILL = 0.90


def test_oracle_cubes_are_filled_and_distinct():
    """What keeps a pass of the kernel from being empty and a moved voxel from hiding: on every camera set and
    grid of the table the oracle cube of uniform random heatmaps has at least 90 % nonzero voxels and at least
    90 % distinct values per joint (two joints of one frame here; the GPU test asserts it on each case's own
    frames).  If a camera set cannot meet it at some shape, change the camera set, not the bound."""
    import torch

    from oracle import fvp_oracle as O

    seen, worst = set(), (1.0, 1.0, None)
    for c in VC.build():
        for seq in ("a", "b") if c.gi else ("a",):
            key = (c.V, seq, c.bins, c.hm)
            if key in seen:
                continue
            seen.add(key)
            g = torch.Generator().manual_seed(len(seen))
            hm = torch.rand((c.V, 2, c.hm[1], c.hm[0]), generator=g).numpy()
            ref = O.voxelize(hm, VC.sample_grid(c.V, seq, c.bins, c.hm))
            fill = np.count_nonzero(ref) / ref.size
            distinct = min(len(np.unique(r)) for r in ref) / ref[0].size
            worst = min(worst, (fill, distinct, key), key=lambda t: min(t[:2]))
            assert fill >= FILL and distinct >= FILL, (key, fill, distinct)
    print(len(seen), "camera set x grid combinations; worst", worst)


@pytest.fixture(scope="module")
def walks():
    """(case, record) of every launch of the table whose walk is distinct."""
    out = {}
    for c in VC.build():
        for r in VC.plan_of(c):
            key = (c.bins, r.lpv, r.cols, r.band, r.col_blocks, r.nb // r.nf)
            out.setdefault(key, (c, r))
    return list(out.values())


def _unsnapped(c, r):
    """The column group gather_cfg wanted before the snap (a divisor search upwards from the launched one)."""
    X, Y, Z = c.bins
    for want in range(r.cols + 1, 2 * r.cols + 1):
        cc = want
        while cc > 1 and Y % cc:
            cc -= 1
        if cc == r.cols:
            return want
    return r.cols


def test_walk_covers_every_case_exactly_once(walks):
    assert len(walks) >= 60
    for c, r in walks:
        assert WK.check(*c.bins, r.lpv, r.cols, r.band, r.col_blocks, r.nb // r.nf) == [], (c, r)


@pytest.mark.parametrize("fault", WK.FAULTS)
def test_planted_fault_breaks_a_named_case(walks, fault):
    hit = [VC.case_id(c) for c, r in walks
           if WK.check(*c.bins, r.lpv, r.cols, r.band, r.col_blocks, r.nb // r.nf, unsnapped=_unsnapped(c, r), fault=fault)]
    print(fault, len(hit), hit[:3])
    assert hit, f"no case of the table sees the planted fault {fault}"
