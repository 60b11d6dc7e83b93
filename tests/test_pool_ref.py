"""tests/pool_ref.py on the CPU, over the cases of tests/pool_cases.py: the pool reference equals
torch's CPU max_pool2d bit for bit on every case (NaN by position; bf16 through .float() and back),
every planted fault differs from the reference on at least one case (pytest -s prints the first such
case and how many there are), the table reaches what its docstring lists, and the entry points refuse
bad arguments on the host, before any HIP call.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_cases as C
import pool_ref as R

NULL, SHAPE = 1001, 1002
P = 4096  # a non-NULL, 16-B aligned stand-in: every call below returns before any launch


def _ref(c, fault=None):
    return R.pool(C.data(c), c.k, c.s, c.p, 8 if c.bf16 else 4, fault)


def test_reference_equals_torch_max_pool2d_on_every_case():
    bad = []
    for c in C.pools():
        x = torch.from_numpy(C.data(c))
        if c.bf16:
            assert R.same(x.bfloat16().float().numpy(), x.numpy()), "the inputs must be exact in bf16"
        ref = R.pool(x.numpy(), c.k, c.s, c.p)
        for name, xin in (("contiguous", x.permute(0, 3, 1, 2).contiguous()), ("channels-last", x.permute(0, 3, 1, 2))):
            t = F.max_pool2d(xin, c.k, c.s, c.p).permute(0, 2, 3, 1).contiguous()
            if c.bf16:
                t = t.bfloat16().float()
            if not R.same(ref, t.numpy()):
                bad.append(f"{C.pool_id(c)} ({name})")
    assert not bad, "\n".join(bad)


def test_every_planted_pool_fault_is_caught():
    seen = {f: [] for f in R.FAULTS}
    for c in C.pools():
        ref = _ref(c)
        for f in R.FAULTS:
            if not R.same(ref, _ref(c, f)):
                seen[f].append(C.pool_id(c))
    for f, ids in seen.items():
        print(f"{f}: differs on {len(ids)} cases, the first {ids[0] if ids else None}")
    assert all(seen.values()), [f for f, ids in seen.items() if not ids]
    # both pool families and both precisions tell the faults that can show in them
    for pad in (False, True):
        for bf16 in (False, True):
            tag = f"{'pad' if pad else 'pool'}-{'bf16' if bf16 else 'f32'}-"
            want = set(R.FAULTS) - (set() if pad else {"zero_pad", "s_for_k"})
            got = {f for f, ids in seen.items() if any(i.startswith(tag) for i in ids)}
            assert want <= got, (tag, want - got)


def test_pool_table_reaches_what_it_lists():
    cases = C.pools()
    assert len(set(cases)) == len(cases)
    for bf16 in (False, True):
        un = C.unpadded(bf16)
        assert {c.C for c in un} == ({8, 24} if bf16 else {4, 20})
        for k in C.KHKW:
            shapes = {(c.N, c.H, c.W) for c in un if c.k == k}
            assert shapes >= {(1,) + k, (3, 5, 7), (2, 6, 4)} and ((2, 1, 9) in shapes) == (k[0] == 1)
            assert any(C.threads(c) > 256 and C.threads(c) % 256 for c in un if c.k == k), k
        pd = [c for c in C.padded(bf16) if c.N < C.GRID_Y]
        assert {c.C for c in pd} >= ({8, 24} if bf16 else {4, 20}) and {c.N for c in pd} >= {1, 3}
        for k, s, p in C.KSP:
            sizes = {(c.H, c.W) for c in pd if (c.k[0], c.s[0], c.p[0]) == (k, s, p)}
            assert sizes >= {hw for hw in C.SIZES if min(hw) + 2 * p >= k}, (k, s, p)
    f32 = C.padded(False)
    assert {(c.H % 2, c.W % 2) for c in f32 if C.fast(c)} == {(0, 0), (1, 1), (0, 1)}  # even sizes too
    assert any(C.fast(c) and c.N * C.out_hw(c)[0] == C.GRID_Y for c in f32)
    assert any(not C.fast(c) and c.k == (3, 3) and c.s == (2, 2) and c.N * C.out_hw(c)[0] == C.GRID_Y + 1 for c in f32)
    assert any(C.fast(c) and C.out_hw(c)[1] * c.C // 4 > 256 for c in f32)
    # the inputs: zeros in both orders and a NaN at either end of the first window, which is a border
    # window; +inf and NaN in what floor mode drops, and none of it in the result
    for c in cases:
        x, taps = C.data(c), C.first_window(c)
        if len(taps) >= 2:
            a, b = taps[0], taps[-1]
            sign = lambda v: bool(np.signbit(v).all()) and bool((v == 0).all())  # noqa: E731
            assert not sign(x[:, a[0], a[1], 0]) and sign(x[:, b[0], b[1], 0])
            assert sign(x[:, a[0], a[1], 1]) and not sign(x[:, b[0], b[1], 1])
            assert np.isnan(x[:, a[0], a[1], 2]).all() and np.isnan(x[:, b[0], b[1], 3]).all()
            ref = _ref(c)
            assert not np.signbit(ref[:, 0, 0, 0]).any() and np.signbit(ref[:, 0, 0, 1]).all()
            assert (ref[:, 0, 0, :2] == 0).all() and np.isnan(ref[:, 0, 0, 2:4]).all()
        dy, dx = C.dropped(c)
        if dy < c.H or dx < c.W:
            assert not np.isfinite(x[:, dy:]).any() and not np.isfinite(x[:, :, dx:]).any()
    odd = [c for c in cases if C.dropped(c)[0] < c.H and C.dropped(c)[1] < c.W]
    assert {(c.pad, c.bf16) for c in odd} == {(a, b) for a in (False, True) for b in (False, True)}
    assert sum(bool((C.data(c)[..., 0] >= 0).any()) for c in cases if c.k != (1, 1)) > 0
    neg = [c for c in cases if not (np.nan_to_num(C.data(c), nan=-1.0, posinf=-1.0) > 0).any()]
    assert len(neg) > len(cases) // 2  # most cases hold nothing above zero


def test_layout_and_copy_references_and_their_planted_faults():
    pre = C.PREFILL_BITS
    seen = {}
    for c in C.to_nhwc_cases():
        x = C.bits((c.N, c.C, c.H, c.W), *c)
        ref = R.nchw_to_nhwc(x, c.Cp, pre)
        want = torch.zeros((c.N, c.H, c.W, c.Cp), dtype=torch.int32)
        want[..., :c.C] = torch.from_numpy(x).permute(0, 2, 3, 1)
        assert np.array_equal(ref, want.numpy()) and not ref[..., c.C:].any()
        for f in R.LAYOUT_FAULTS:
            if not np.array_equal(ref, R.nchw_to_nhwc(x, c.Cp, pre, f)):
                seen.setdefault(("to_nhwc", f), []).append(tuple(c))
    for c in C.to_nchw_cases():
        x = C.bits((c.N, c.H, c.W, c.Cp), *c)
        ref = R.nhwc_to_nchw(x, c.C, pre)
        assert np.array_equal(ref, torch.from_numpy(x)[..., :c.C].permute(0, 3, 1, 2).contiguous().numpy())
        for f in ("pitch", "tail"):
            if not np.array_equal(ref, R.nhwc_to_nchw(x, c.C, pre, f)):
                seen.setdefault(("to_nchw", f), []).append(tuple(c))
    for nb in C.COPY_BYTES:
        x = C.bits((nb // 4,), "copy", nb)
        assert np.array_equal(R.copy_f4(x, pre), x)
        if not np.array_equal(x, R.copy_f4(x, pre, "tail")):
            seen.setdefault(("copy", "tail"), []).append(nb)
    for k, v in sorted(seen.items()):
        print(f"{k[0]} {k[1]}: differs on {len(v)} cases, the first {v[0]}")
    assert set(seen) == {("to_nhwc", f) for f in R.LAYOUT_FAULTS} | {("to_nchw", "pitch"), ("to_nchw", "tail"),
                                                                     ("copy", "tail")}
    assert seen[("copy", "tail")] == [16, 16 * 255, 16 * 257]
    # every listed pitch, pixel count and batch size
    a, b = C.to_nhwc_cases(), C.to_nchw_cases()
    assert {(c.C, c.Cp) for c in a} == set(C.TO_NHWC_CCP) and {c.H * c.W for c in a} == {1, 15, 64, 65}
    assert {(c.C, c.Cp) for c in b} == set(C.TO_NCHW_CCP) and {c.H * c.W for c in b} == {1, 63, 64, 65, 129}
    assert {c.N for c in a} == {c.N for c in b} == {1, 3}
    assert {c.Cp for c in a if c.Cp in (4, 8, 16, 32)} == {4, 8, 16, 32} and {c.Cp for c in a} > {4, 8, 16, 32}
    assert {(c.Cp % 4 == 0 and c.C <= 128) for c in b} == {False, True}
    assert [(f.c0, f.c0 % 4 == 0) for f in C.FROM] == [(1, False), (4, True)]
    assert all(f.c0 + f.C <= f.Cp for f in C.FROM)


# ---- host-side refusals ------------------------------------------------------------------
def _lib():
    from fvp import _lib as L

    return L.load()


def _with(fn, args, **changes):
    a = list(args)
    for i, v in changes.items():
        a[int(i[1:])] = v
    return fn(*a)


@pytest.mark.parametrize("name, quantum", [("fvp_maxpool_pad_nhwc", 4), ("fvp_maxpool_pad_nhwc_bf16", 8)])
def test_padded_pools_refuse_bad_arguments_without_gpu(name, quantum):
    fn = getattr(_lib(), name)
    good = [P, 2, 5, 7, 24, 3, 2, 1, P, None]  # (in, N, H, W, C, K, S, P, out, stream)
    assert _with(fn, good, a0=None) == NULL and _with(fn, good, a8=None) == NULL
    for ch in ({"a4": 24 + quantum // 2}, {"a4": 0}, {"a1": 0}, {"a2": 0}, {"a3": 0}, {"a5": 0}, {"a6": 0},
               {"a7": -1}, {"a7": 2}, {"a5": 2, "a7": 2}, {"a2": 1, "a5": 4, "a7": 1}, {"a3": 2, "a5": 5, "a7": 1}):
        assert _with(fn, good, **ch) == SHAPE, (name, ch)
    for i in (0, 8):  # 16-B loads and stores
        for off in (4, 8, 2):
            assert _with(fn, good, **{f"a{i}": P + off}) == SHAPE, (name, i, off)


@pytest.mark.parametrize("name, quantum", [("fvp_maxpool_nhwc", 4), ("fvp_maxpool_nhwc_bf16", 8)])
def test_unpadded_pools_refuse_bad_arguments_without_gpu(name, quantum):
    fn = getattr(_lib(), name)
    good = [P, 2, 5, 7, 24, 2, 2, P, None]  # (in, N, H, W, C, KH, KW, out, stream)
    assert _with(fn, good, a0=None) == NULL and _with(fn, good, a7=None) == NULL
    for ch in ({"a4": 24 + quantum // 2}, {"a4": 0}, {"a1": 0}, {"a5": 0}, {"a6": 0}, {"a5": 3}, {"a6": 3},
               {"a2": 1}, {"a3": 1}, {"a2": 0, "a5": 1}):
        assert _with(fn, good, **ch) == SHAPE, (name, ch)
    for i in (0, 7):
        for off in (4, 8, 2):
            assert _with(fn, good, **{f"a{i}": P + off}) == SHAPE, (name, i, off)


def test_maxpool2_layouts_and_copy_refuse_bad_arguments_without_gpu():
    lib = _lib()
    good = [P, 2, 5, 7, 24, P, None]  # fvp_maxpool2_nhwc(in, N, H, W, C, out, stream)
    assert _with(lib.fvp_maxpool2_nhwc, good, a0=None) == NULL and _with(lib.fvp_maxpool2_nhwc, good, a5=None) == NULL
    for ch in ({"a4": 22}, {"a2": 1}, {"a3": 1}, {"a1": 0}, {"a0": P + 4}, {"a5": P + 8}):
        assert _with(lib.fvp_maxpool2_nhwc, good, **ch) == SHAPE, ch
    for fn in (lib.fvp_nchw_to_nhwc, lib.fvp_nhwc_to_nchw):
        good = [P, 2, 15, 5, 7, 16, P, None]  # (in, N, C, H, W, Cp, out, stream)
        assert _with(fn, good, a0=None) == NULL and _with(fn, good, a6=None) == NULL
        for ch in ({"a5": 14}, {"a1": 0}, {"a2": 0}, {"a3": 0}, {"a4": 0}):
            assert _with(fn, good, **ch) == SHAPE, (fn.__name__, ch)
    assert lib.fvp_copy_f4(None, P, 16, None) == NULL and lib.fvp_copy_f4(P, None, 16, None) == NULL
    for nb in (1, 8, 15, 17, 16 * 256 + 4):
        assert lib.fvp_copy_f4(P, P, nb, None) == SHAPE, nb
    assert lib.fvp_copy_f4(P, P, 0, None) == 0  # nothing to copy: no launch
