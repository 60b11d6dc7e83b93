"""tests/cnn_edge_ref.py on the CPU, over the cases of tests/cnn_edge_cases.py: a float32 (or
bf16-operand) evaluation of each operation meets its criterion, the cap holds on every case
of the bf16 kernels, every planted fault leaves the criterion on the cases it shows on, and
the eight entry points refuse bad arguments on the host, before any HIP call.

Measured here (pytest -s prints them; numbers to read the GPU ratios against, not
tolerances).  Largest err / tol of the clean fp32 evaluations: stem7_f32 0.040, front7_f32
0.014, 1x1 head 0.218 (Cin 16: the shortest chain, where the epilogue's roundings weigh
most), fused tail 0.034.  bf16 kernels: no element outside its interval; largest wide share
stem7_bf16 0.031, front7_bf16 0.089 (the cap is 0.30).  Smallest err / tol a planted fault
reaches over the cases it shows on (fp32 kernels; inf: a NaN left): tap 1.6e3, seam 6.3e3,
wrap / plane / swap / row / ho inf; 1x1 head wrow 296, pixel inf; fused tail skip1 136 (outside
tol on 0.97 of a case's elements at least), class 1.0e4 (0.15), noskip 1.2e4 (1.00).  bf16
kernels, smallest count of elements outside their interval: stem7_bf16 tap 10,400, wrap 64,
plane 64, swap 1,024, seam 80, row 64, ho 64, rtz 7,920; front7_bf16 tap 431, wrap 16, plane
16, swap 256, seam 133, row 16, rtz 151.
"""
import ctypes

import numpy as np
import pytest

import cnn_edge_cases as C
import cnn_edge_ref as E

NULL, SHAPE = 1001, 1002
P = 4096  # a non-NULL, 16-B aligned stand-in: every call below returns before any launch


def _worst(r):
    return float(np.max(r))


@pytest.mark.parametrize("name", sorted(E.KERNELS))
def test_7x7_emulation_meets_the_criterion_and_faults_leave_it(name):
    k = E.KERNELS[name]
    cases = C.cases7(name)
    clean, share, planted, bad = 0.0, 0.0, {}, []
    for c in cases:
        d = C.data7(c)
        args = (k, d["x"], d["w"], d["scale"], d["shift"])

        def judge(got):
            """fp32: the largest err / tol; bf16: the count of elements outside their interval."""
            if k.bf16:
                return int(np.count_nonzero(~E.inside(got, d["pre"], d["tol"])))
            return _worst(E.ratio(got, d["ref"], d["tol"]))

        r = judge(E.emulate7(*args))
        clean, share = max(clean, r), max(share, d["share"])
        if (r > 0) if k.bf16 else not (r <= 1.0):
            bad.append(f"{C.id7(c)}: the clean evaluation misses the criterion ({r:.3g})")
        if d["share"] > E.CAP:
            bad.append(f"{C.id7(c)}: wide share {d['share']:.3f} above the cap")
        for f in E.faults7(k, c.N, c.C, c.H, c.W):
            fr = judge(E.emulate7(*args, fault=f))
            planted[f] = min(planted.get(f, np.inf), fr)
            if (fr == 0) if k.bf16 else not (fr > 1.0):
                bad.append(f"{C.id7(c)}: fault {f} stays inside the criterion ({fr:.3g})")
    what = "elements outside" if k.bf16 else "err / tol"
    print(f"{name}: clean {what} {clean:.3g}, largest wide share {share:.3f}; smallest {what} per fault: "
          + ", ".join(f"{f} {v:.3g}" for f, v in sorted(planted.items())))
    want = set(E.FAULTS7) - (set() if k.stride == 2 else {"ho"}) - (set() if k.bf16 else {"rtz"})
    assert set(planted) == want, want - set(planted)
    assert not bad, "\n".join(bad)


def test_7x7_cases_cover_the_listed_shapes():
    for name, k in E.KERNELS.items():
        cases = C.cases7(name)
        assert len(set(cases)) == len(cases)
        assert name == "front7_bf16" or C.walk_base7(name) in cases  # (one tile per block: no walk)
        cs = {c.C for c in cases}
        if k.stride == 2:
            assert cs == ({1, 2, 3, 4} if k.bf16 else {1, 2, 3})
            assert {(c.N, c.C, c.H, c.W) for c in cases} >= {(1, 3, 1, 1), (2, 1, 2, 3), (3, 3, 17, 131)}
            grid = {(ch, h, w) for ch in cs for h in (15, 16, 17) for w in (63, 64, 65)}
            assert {(c.C, c.H, c.W) for c in cases} >= grid
            assert E.tiles7(k, 17, 131) == (2, 3) and E.tiles7(k, 16, 64) == (1, 1) and E.tiles7(k, 17, 65) == (2, 2)
        else:
            assert cs == {1, 3, 4, 5, 8, 9, 15, 16}
            assert {(c.N, c.C, c.H, c.W) for c in cases} >= {(1, 1, 1, 1), (3, 5, 5, 3), (3, 15, 9, 49)}
            assert {(c.H, c.W) for c in cases} >= {(h, w) for h in (8, 9) for w in (16, 17, 32, 33)}
            grids = {E.tiles7(k, c.H, c.W) for c in cases if c.N == 3}
            assert any(ty > 1 and tx > 1 and ty != tx for ty, tx in grids), grids
        assert all(d["x"][:, :, [0, -1]].all() and d["x"][..., [0, -1]].all()
                   for d in map(C.data7, cases) if k.stride == 2), "image borders must be non-zero"


@pytest.mark.parametrize("cin", C.CIN1)
def test_1x1_emulation_inside_the_bound_and_faults_outside(cin):
    clean, planted, bad = 0.0, {}, []
    for i, c in enumerate(C.cases1(cin)):
        conv, layer = C.packed1(c.Cin, c.Cout)
        rows = C.rows1(100 * cin + i, c.N, c.H, c.W, c.pitch)
        w = conv.weight.detach().numpy()[:, :, 0, 0]
        scale, shift = layer.scale[:c.Cout].numpy(), layer.shift[:c.Cout].numpy()
        assert not layer.wpack[0, c.Cin:].any() and np.array_equal(layer.wpack[0, :c.Cin, :c.Cout].numpy(), w.T)
        ref, tol = E.ref1x1(C.nchw(rows, 0, c.Cin), w, scale, shift, c.relu)
        args = (rows, 0, c.Cin, w, scale, shift, c.relu)
        r = _worst(E.ratio(E.emulate1x1(*args), ref, tol))
        clean = max(clean, r)
        if not r <= 1.0:
            bad.append(f"{c}: emulation at {r:.3g} x tol")
        # (a ReLU can cut the few outputs of a one-pixel case with and without the extra row)
        shows = c.Cin < 4 * E.t4_of(c.Cin) and (not c.relu or c.N * c.H * c.W * c.Cout >= 16)
        faults = (["wrow"] if shows else []) + (["pixel"] if c.N > 1 else [])
        for f in faults:
            fr = _worst(E.ratio(E.emulate1x1(*args, fault=f), ref, tol))
            planted[f] = min(planted.get(f, np.inf), fr)
            if not fr > 1.0:
                bad.append(f"{c}: fault {f} stays inside tol ({fr:.3g})")
    print(f"1x1 head Cin {cin} (t4 {E.t4_of(cin)}): clean err / tol {clean:.3g}; smallest per fault: "
          + ", ".join(f"{f} {v:.3g}" for f, v in sorted(planted.items())))
    assert set(planted) == ({"pixel"} if cin in (16, 32, 64) else set(E.FAULTS1X1))
    assert not bad, "\n".join(bad)


def test_1x1_cases_cover_the_listed_shapes():
    assert {E.t4_of(c) for c in C.CIN1} == {4, 8, 16}
    for cin in C.CIN1:
        cases = C.cases1(cin)
        assert {c.Cout for c in cases} == {1, 15, 33, 64} and {c.relu for c in cases} == {0, 1}
        assert {c.N * c.H * c.W for c in cases if c.N == 1} == {1, 255, 256, 257}
        assert any(c.N == 3 and (c.H * c.W) % 256 and c.N * c.H * c.W > 256 for c in cases)
        assert {c.pitch > 4 * E.t4_of(cin) for c in cases} == {False, True} and all(c.pitch % 4 == 0 for c in cases)
    off = C.cases_off()
    assert {c.c0 for c in off} == {16, 36} and {E.t4_of(c.Cin) for c in off} == {4, 8, 16}
    assert all(c.c0 % 4 == 0 and c.c0 + 4 * E.t4_of(c.Cin) <= c.Cp and c.c0 + c.Cin <= c.C <= c.Cp for c in off)


def test_tail_emulation_inside_the_bound_and_faults_outside():
    """The float32 two-stage evaluation stays inside the two-stage bound on every case; the
    skip left out of one channel, swapped parity classes and a head that reads y before the
    skip leave it on every case (printed: on which share of a case's elements at least)."""
    clean, planted, outside, bad = 0.0, {}, {}, []
    for c in C.cases_tail():
        d = C.data_tail(c)
        args = C.tail_args(d)
        r = _worst(E.ratio(E.emulate_tail(*args), d["ref"], d["tol"]))
        clean = max(clean, r)
        if not r <= 1.0:
            bad.append(f"{C.id_tail(c)}: emulation at {r:.3g} x tol")
        for f in E.FAULTS_TAIL:
            fr = E.ratio(E.emulate_tail(*args, fault=f), d["ref"], d["tol"])
            planted[f] = min(planted.get(f, np.inf), _worst(fr))
            outside[f] = min(outside.get(f, 1.0), float(np.mean(fr > 1.0)))
            if not _worst(fr) > 1.0:
                bad.append(f"{C.id_tail(c)}: fault {f} stays inside tol ({_worst(fr):.3g})")
    print(f"fused tail: clean err / tol {clean:.3g}; smallest per fault (share of elements outside): "
          + ", ".join(f"{f} {v:.3g} ({outside[f]:.2f})" for f, v in sorted(planted.items())))
    assert not bad, "\n".join(bad)


def test_tail_cases_cover_the_listed_shapes():
    cases = C.cases_tail()
    assert {(c.Cpi, c.Cs) for c in cases} == {(a, b) for a in (16, 48, 64, 80, 128) for b in (1, 20, 29, 32)}
    assert {c.J for c in cases} == {1, 15, 16} and {c.W for c in cases} == {32, 96} and {c.H for c in cases} == {1, 3}
    assert all(c.N == 2 and c.Cps in (-(-c.Cs // 4) * 4, 32) for c in cases)
    for cs in (1, 20):  # both pitch rules where they differ
        assert {c.Cps for c in cases if c.Cs == cs} == {-(-cs // 4) * 4, 32}
    a, b = C.walk_bases_tail()  # one K step with clamped loads; the first K step loaded per item
    assert (a.Cpi, b.Cpi) == (16, 80) and all(c.N == 2 and c.W % 32 == 0 for c in (a, b))


def test_tail_packer_gives_the_kernel_32_scales():
    """up2_head_nchw reads the folded BN of all 32 y channels: the packer hands it 32, zero past
    Cout, whatever Cpo the deconvolution layer has (16 where Cout <= 16)."""
    for c in C.cases_tail():
        f = C.data_tail(c)["f"]
        wd, layer, wh, J, scale, shift = f.tail
        assert scale.numel() == shift.numel() == 32 and J == c.J
        assert np.array_equal(scale[:c.Cs].numpy(), layer.scale[:c.Cs].numpy()) and not scale[c.Cs:].any()
        assert np.array_equal(shift[:c.Cs].numpy(), layer.shift[:c.Cs].numpy()) and not shift[c.Cs:].any()
        assert tuple(wd.shape) == (c.Cpi // 16, 4, 128, 4) and tuple(wh.shape) == (2, 4, 16, 4)


# ---- host-side refusals ------------------------------------------------------------------
def _lib():
    from fvp import _lib as L

    return L.load()


def _nulls(fn, args, ptrs):
    """Every pointer argument (positions `ptrs`) NULL in turn -> FVP_ERR_NULL."""
    for i in ptrs:
        a = list(args)
        a[i] = None
        assert fn(*a) == NULL, (fn.__name__, i)


def _shape(fn, args, **changes):
    a = list(args)
    for i, v in changes.items():
        a[int(i[1:])] = v
    return fn(*a)


@pytest.mark.parametrize("name, cmax", [("fvp_conv_stem7_f32", 3), ("fvp_conv_stem7_bf16", 4),
                                        ("fvp_conv_front7_f32", 16), ("fvp_conv_front7_bf16", 16)])
def test_7x7_entry_points_refuse_bad_arguments_without_gpu(name, cmax):
    fn = getattr(_lib(), name)
    good = [P, 2, cmax, 17, 65, P, P, P, P, None]  # (x, N, C, H, W, wpack, scale, shift, out, stream)
    _nulls(fn, good, (0, 5, 6, 7, 8))
    for ch in ({"a1": 0}, {"a2": 0}, {"a2": cmax + 1}, {"a3": 0}, {"a4": 0}, {"a3": -1}, {"a4": -5}):
        assert _shape(fn, good, **ch) == SHAPE, (name, ch)
    if name == "fvp_conv_stem7_f32":  # its 16-B LDS copies and stores
        for i in (5, 6, 7, 8):
            assert _shape(fn, good, **{f"a{i}": P + 4}) == SHAPE, i
    # more tiles than INT_MAX
    assert _shape(fn, good, a1=1 << 30, a3=1024, a4=1024) == SHAPE


@pytest.mark.parametrize("name", ["fvp_conv_stem7_u8_f32", "fvp_conv_stem7_u8_bf16"])
def test_u8_stems_refuse_bad_arguments_without_gpu(name):
    from fvp._lib import FrameSpec

    fn = getattr(_lib(), name)
    f3 = ctypes.c_float * 3

    def spec(**kw):
        f = dict(H=16, W=32, VR=1, VC=1, frame_stride=16 * 32 * 3, vr_stride=0, vc_stride=0, row_stride=32 * 3,
                 pix_stride=3, swap_rb=0)
        f.update(kw)
        return ctypes.byref(FrameSpec(mean=f3(0.485, 0.456, 0.406), std=f3(0.229, 0.224, 0.225), **f))

    good = [P, 1, spec(), P, P, P, P, None]  # (frames, B, spec, wpack, scale, shift, out, stream)
    _nulls(fn, good, (0, 2, 3, 4, 5, 6))
    for ch in ({"a1": 0}, {"a2": spec(H=0)}, {"a2": spec(W=0)}, {"a2": spec(pix_stride=2)}, {"a3": P + 8},
               {"a6": P + 8}):
        assert _shape(fn, good, **ch) == SHAPE, (name, list(ch))


def test_conv1x1_nchw_refuses_bad_arguments_without_gpu():
    fn = _lib().fvp_conv1x1_nchw
    # (in, N, H, W, Cpi, Cin, w, ldw, Cout, scale, shift, relu, out, stream)
    good = [P, 1, 7, 13, 32, 17, P, 128, 33, P, P, 0, P, None]
    _nulls(fn, good, (0, 6, 9, 10, 12))
    for ch in ({"a8": 65}, {"a8": 0}, {"a4": 34}, {"a4": 68, "a5": 65}, {"a4": 128, "a5": 65}, {"a4": 28},
               {"a4": 16}, {"a4": 48, "a5": 33}, {"a0": P + 4}, {"a0": P + 8}, {"a7": 32}, {"a1": 0}, {"a2": 0},
               {"a3": 0}, {"a5": 0}, {"a4": 16, "a5": 17}):
        assert _shape(fn, good, **ch) == SHAPE, ch
    # 4 t4 <= Cpi at each instantiation's edge: Cin 16 reads 16, 17 reads 32, 33 reads 64
    for cpi, cin in ((12, 12), (28, 20), (60, 40)):
        assert _shape(fn, good, a4=cpi, a5=cin) == SHAPE, (cpi, cin)


def test_up2_head_nchw_refuses_bad_arguments_without_gpu():
    fn = _lib().fvp_up2_head_nchw
    # (in, N, H, W, Cpi, wd, scale, shift, skip, Cps, Cs, wh, hscale, hshift, J, out, stream)
    good = [P, 2, 3, 96, 80, P, P, P, P, 32, 29, P, P, P, 16, P, None]
    _nulls(fn, good, (0, 5, 6, 7, 8, 11, 12, 13, 15))
    for ch in ({"a3": 95}, {"a3": 48}, {"a3": 0}, {"a4": 72}, {"a4": 8}, {"a4": 144}, {"a4": 0}, {"a10": 33, "a9": 36},
               {"a10": 0}, {"a9": 28}, {"a9": 30}, {"a9": 34}, {"a14": 17}, {"a14": 0}, {"a0": P + 4}, {"a0": P + 8},
               {"a8": P + 4}, {"a8": P + 8}, {"a1": 0}, {"a2": 0}):
        assert _shape(fn, good, **ch) == SHAPE, ch
