"""CPU tests of the one-launch 1-D net kernel's reference (tests/c2c_ref.py), its case list
(tests/c2c_cases.py), the host compiler fvp.cnn.Net1D and fvp_conv1d_net's argument checks.
tests/test_gpu_c2c_ops.py holds the kernel itself to the same reference on the GPU.

What is shown here, without a GPU:
  * run_program(), which starts every buffer as NaN and writes only what the kernel writes,
    reproduces the float64 torch module on the programs Net1D.build makes (1e-6 of the output
    scale: the residue is the fp32 BatchNorm fold) and meets no NaN -- the host compiler
    leaves no op reading an unwritten pad or a stale row;
  * op_reference() is torch's conv1d / conv_transpose1d / max_pool1d in float64;
  * on every op of every case, at every lg the case runs at, the fp32 evaluation in the
    kernel's order is inside the derived bound and every planted fault that applies leaves it;
  * the case list reaches every class of coverage(), and Net1D.build's programs are pinned.
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import c2c_cases as C
import c2c_ref as R

CASES = C.all_cases()
IDS = [c.name for c in CASES]


def _ops(net):
    return [tuple(o) for o in net.ops]


@pytest.mark.parametrize("cin0,cout", [(15, 1), (1, 1), (3, 2), (17, 5), (16, 4)])
def test_run_program_equals_float64_module(cin0, cout):
    from fvp.cnn import Net1D

    m = C.net_module(cin0, cout)
    m64 = C.net_module(cin0, cout).double()
    for z in (4, 8, 12, 20, 32, 64):
        n = Net1D.build(m, cin0, z)
        assert n is not None and n.lg == 4
        x = np.random.default_rng(z).uniform(-1, 1, (2, cin0, z)).astype(np.float32)
        got = R.run_program(n.ops, n.param.numpy(), x, slot=n.slot, nbuf=n.nbuf)
        with torch.no_grad():
            ref = m64(torch.from_numpy(x).double()).numpy()
        assert got.shape == ref.shape and not np.isnan(got).any()
        err = np.abs(got - ref).max() / np.abs(ref).max()
        assert err <= 1e-6, (z, err)
        # a prefix, and a buffer other than the last op's
        first = R.run_program(n.ops, n.param.numpy(), x, slot=n.slot, nbuf=n.nbuf, upto=1)
        b = list(m64.front_layers[0].block.children())
        with torch.no_grad():
            ref1 = torch.relu(b[1](b[0](torch.from_numpy(x).double()))).numpy()
        assert np.abs(first - ref1).max() <= 1e-6 * np.abs(ref1).max()


def test_run_program_shows_an_unwritten_pad_and_a_stale_row():
    """The interpreter's purpose: a conv that reads rows nobody wrote (here: buffer 1 given
    through `inputs` at one pitch and read at another) gives NaN or a wrong value."""
    case = next(c for c in CASES if c.name == "len8-k3")
    n = C.build(case, 4)
    x = C.inputs(case)
    good = R.run_program(n.ops, n.param.numpy(), x, slot=n.slot, nbuf=n.nbuf)
    assert np.isfinite(good).all()
    op = list(_ops(n)[0])
    op[R.SRC], op[R.DST] = 1, 0  # read a buffer that holds nothing
    assert np.isnan(R.run_program([op], n.param.numpy(), x, slot=n.slot, nbuf=n.nbuf)).all()
    stale = np.full((3, 4, 9), 7.0)  # rows of length 9 where the op reads rows of length 8
    bad = R.run_program([op], n.param.numpy(), x, slot=n.slot, nbuf=n.nbuf, inputs={1: stale})
    same = R.run_program([op], n.param.numpy(), x, slot=n.slot, nbuf=n.nbuf, inputs={1: stale[:, :, :8]})
    assert np.isfinite(same).all() and not np.allclose(bad, same)


@pytest.mark.parametrize("k,cin,cout,ln", [(1, 4, 3, 5), (3, 8, 5, 1), (3, 4, 2, 6), (5, 4, 3, 7), (7, 4, 3, 2),
                                           (7, 8, 2, 9), ("t", 4, 3, 1), ("t", 8, 5, 6)])
def test_op_reference_is_torch_float64(k, cin, cout, ln):
    rng = np.random.default_rng(cin * 100 + cout * 10 + ln)
    kk = 2 if k == "t" else k
    lo = 2 * ln if k == "t" else ln
    w = rng.normal(0, 1, (cin, kk, cout)).astype(np.float32)
    sc, sh = rng.uniform(-2, 2, cout).astype(np.float32), rng.normal(0, 1, cout).astype(np.float32)
    params = np.concatenate([np.zeros(4, np.float32), w.reshape(-1), sc, sh])
    x = rng.normal(0, 1, (2, cin, ln)).astype(np.float32)
    pre, post = (rng.normal(0, 1, (2, cout, lo)).astype(np.float32) for _ in range(2))
    op = (1 if k == "t" else 0, cin, cout, kk, ln, 0, 1, 2, 3, 1, 4, cin)
    ref, tol = R.op_reference(op, params, x, pre, post)
    xt, wt = torch.from_numpy(x).double(), torch.from_numpy(w).double()
    if k == "t":
        y = F.conv_transpose1d(xt, wt.permute(0, 2, 1), stride=2)  # [cin][cout][2]
        yabs = F.conv_transpose1d(xt.abs(), wt.abs().permute(0, 2, 1), stride=2)
    else:
        y = F.conv1d(xt, wt.permute(2, 0, 1), padding=(k - 1) // 2)  # [cout][cin][k]
        yabs = F.conv1d(xt.abs(), wt.abs().permute(2, 0, 1), padding=(k - 1) // 2)
    s, b = torch.from_numpy(sc).double()[None, :, None], torch.from_numpy(sh).double()[None, :, None]
    want = torch.relu(y * s + b + torch.from_numpy(pre).double()) + torch.from_numpy(post).double()
    assert np.abs(ref - want.numpy()).max() <= 1e-13 * max(1.0, float(want.abs().max()))
    products = cin * (1 if k == "t" else k)
    tw = (products + 8) * R.U * ((s.abs() * yabs + b.abs()).numpy() + np.abs(pre) + np.abs(post))
    assert np.allclose(tol, tw, rtol=1e-12, atol=0)
    # without residuals and ReLU
    ref0, _ = R.op_reference(op[:7] + (-1, -1, 0) + op[10:], params, x)
    assert np.abs(ref0 - (y * s + b).numpy()).max() <= 1e-13 * max(1.0, float(y.abs().max()))


def test_pool_reference_is_max_pool1d_with_nan():
    rng = np.random.default_rng(3)
    for ln in (2, 3, 7, 8):
        x = rng.normal(0, 1, (2, 5, ln)).astype(np.float32)
        x[0, 1, 0] = np.nan           # first slot of a window
        x[1, 2, 1] = np.nan           # second slot
        x[1, 4, ln - 1] = -np.inf
        op = (2, 5, 5, 2, ln, 0, 1, -1, -1, 0, 0, 1)
        ref, tol = R.op_reference(op, None, x)
        assert tol is None
        assert R.same_bits(ref, F.max_pool1d(torch.from_numpy(x), 2, 2).numpy())
        assert R.same_bits(R.emulate(op, None, x, lg=4), ref)


def test_plan_restatements():
    assert [R.splits(i, c) for i, c in ((1, 4), (1, 8), (1, 12), (1, 16), (256, 128), (257, 128), (512, 128),
                                        (513, 128), (1024, 16))] == [1, 2, 2, 4, 4, 2, 2, 1, 1]
    op = (0, 20, 64, 7, 9, 0, 1, -1, -1, 1, 0, 8)
    assert R.chunking(op) == (8, 8, 4) and R.groups(op, 4) == (3, 192, 1) and R.groups(op, 8) == (2, 128, 1)
    assert R.groups((1, 4, 5, 2, 3, 0, 1, -1, -1, 0, 0, 4), 4) == (2, 10, 2)
    assert [R.nstage(w) for w in (4096, 8192, 12288)] == [1, 2, 3]


def _pool_probe(src):
    """A pool's inputs with a NaN in a first slot and in a second slot (and a -Inf)."""
    src = np.array(src, np.float32)
    src[0, 0, 0] = np.nan
    src[-1, -1, 1] = np.nan
    if src.shape[2] >= 4:
        src[0, 0, 3] = -np.inf
    return src


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_emulation_inside_bound_and_planted_faults_outside(case):
    lgs = C.legal_lgs(case)
    assert lgs, "the case runs at no lg"
    for lg in lgs:
        n = C.build(case, lg)
        par = n.param.numpy()
        trace = []
        x = C.inputs(case)
        out = R.run_program(n.ops, par, x, slot=n.slot, nbuf=n.nbuf, trace=trace)
        assert np.isfinite(out).all()
        for o, (op, (src, pre, post, _)) in enumerate(zip(_ops(n), trace)):
            f32 = [None if a is None else a.astype(np.float32) for a in (src, pre, post)]
            if op[R.KIND] == R.POOL:
                f32[0] = _pool_probe(f32[0])
            good = R.emulate(op, par, *f32, lg=lg)
            assert R.check_op(op, par, *f32, good, lg) <= 1.0
            ref, tol = R.op_reference(op, par, *f32)
            if case.group == "reuse" and o == 0:
                continue  # the 1e30 filler (its bound is 1e24: no fault of the sums can leave it)
            for fault in R.FAULTS:
                if not R.applicable(fault, op, lg):
                    continue
                bad = R.emulate(op, par, *f32, lg=lg, fault=fault)
                if tol is None:
                    assert not R.same_bits(bad, ref), f"op {o} lg {lg}: fault {fault} goes unnoticed"
                else:
                    assert R.within(bad, ref, tol) > 1.0, f"op {o} lg {lg}: fault {fault} stays inside the bound"


def test_every_fault_applies_somewhere():
    seen = set()
    for case in CASES:
        for lg in C.legal_lgs(case):
            for op in _ops(C.build(case, lg)):
                seen.update(f for f in R.FAULTS if R.applicable(f, op, lg))
    assert seen == set(R.FAULTS)


@pytest.mark.parametrize("case", C.nonfinite_cases(), ids=[c.name for c in C.nonfinite_cases()])
def test_check_op_with_non_finite_inputs(case):
    """check_op() on the fp32 evaluation of the non-finite cases: it accepts the correct
    result and refuses one that drops the NaN, moves it, or lets ReLU swallow it."""
    for lg in C.LGS:
        n = C.build(case, lg)
        par = n.param.numpy()
        hold = {0: np.pad(C.nonfinite_inputs(case), ((0, 0), (0, -case.cin0 % 4), (0, 0)))}
        planted = 0
        for op in _ops(n):
            ins = [hold[op[R.SRC]]] + [hold[b] if b >= 0 else None for b in (op[R.RES_PRE], op[R.RES_POST])]
            got = R.emulate(op, par, *ins, lg=lg)
            R.check_op(op, par, *ins, got, lg)
            hold[op[R.DST]] = got
            nan = np.argwhere(np.isnan(got))
            if len(nan):
                planted += 1
                for repl in (0.0, 1.0):
                    bad = got.copy()
                    bad[tuple(nan[0])] = repl
                    with pytest.raises(AssertionError):
                        R.check_op(op, par, *ins, bad, lg)
        assert planted
        if case.name == "nf-res":
            rp, rq, y = hold[n.bufs["rp"][0]], hold[n.bufs["rq"][0]], hold[n.bufs["y"][0]]
            for r, at in zip((rp, rq), C.NF_RES):
                assert [tuple(i[1:]) for i in np.argwhere(np.isnan(r))] == [at] * 3
            assert sorted({tuple(i[1:]) for i in np.argwhere(np.isnan(y))}) == sorted(C.NF_RES)


def test_case_list_reaches_every_class():
    cov = C.coverage()
    # products: every (k | convt) x lg x KS x chunk count class.  Nothing is excluded: cic is
    # wchunk / (k cout) rounded down to 4, so a wide cout gives cic 4 (KS 1) or 8 / 12 (KS 2)
    # at any k, a short tail needs cin % cic != 0 (cic >= 8; at cic 4, KS 1 comes from more
    # than 512 items instead), and one output position keeps the items at cout.
    excluded = {}
    want = set(itertools.product(C.KOPS, C.LGS, (1, 2, 4), C.NCLASSES)) - set(excluded)
    assert cov["products"] == want, (sorted(want - cov["products"], key=str), sorted(cov["products"] - want, key=str))
    assert {(ks, w) for ks, w in cov["ways"] if w in ("cic", "items")} == set(itertools.product((1, 2), ("cic", "items")))
    assert cov["staging"] == set(itertools.product((1, 2, 3), C.FILLS))
    assert cov["store"] == {(lg, r) for lg in C.LGS for r in list(range(lg)) + ["short"]}
    assert cov["epilogue"] == set(itertools.product(("conv", "convt"), C.EPILOGUES))
    # the done-when list, spelled out
    assert {c[1] for c in cov["products"]} == {4, 8} and {c[2] for c in cov["products"]} == {1, 2, 4}
    assert {c[0] for c in cov["products"]} == {1, 3, 5, 7, "t"}
    names = {c.name for c in CASES}
    assert len(names) == len(CASES)
    # each product case gets from Net1D.conv the plan the search predicted for it
    for cls, case in C.product_cases().items():
        kop, lg, ks, nc = cls
        op = _ops(C.build(case, lg))[0]
        assert (C.split_way(op, lg)[0], C.nchunk_class(op)) == (ks, nc) and lg in C.legal_lgs(case)
    by = {c.name: c for c in CASES}
    assert R.groups(_ops(C.build(by["items1024-lg4"], 4))[0], 4)[1] == 1024
    assert R.groups(_ops(C.build(by["items1024-lg8"], 8))[0], 8)[1] == 1024
    assert C.build(by["items1024-lg8"], 4) is None  # 2,048 items at lg 4: refused by _finish
    for case in C.reuse_cases():
        n = C.build(case, 4)
        big, b = C.reused_buffer(n)
        assert big == b and n.bufs["big"][1:] == (32, 16) and n.bufs["b"][1:] == (12, 8)


def test_net1d_build_programs_are_pinned():
    from fvp.cnn import Net1D

    m = C.net_module(15, 1)
    for z, slot, wchunk in ((20, 1424, 12288), (32, 1808, 12288), (64, 2832, 8192)):
        n = Net1D.build(m, 15, z)
        assert (len(n.ops), n.nbuf, n.lg, n.slot, n.wchunk) == (25, 6, 4, slot, wchunk)
        assert (n.cin0, n.L0, n.cout, n.Lout) == (15, z, 1, z)
        assert tuple(n.prog.shape) == (25, 12) and n.prog.dtype == torch.int32
        assert n.param.numel() == n.off and n.param.dtype == torch.float32
        kinds = [o[0] for o in n.ops]
        assert kinds.count(2) == 2 and kinds.count(1) == 2
        assert n.ops[0][:5] == [0, 16, 16, 7, z] and n.ops[-1][:5] == [0, 32, 1, 1, z]
        # the lg override replans the same ops (where the LDS has the room)
        again = n._finish(n.cin0, n.L0, n.out_buf, n.cout, n.Lout, "cpu", lg=8)
        over = R.lds_bytes(slot, 6, wchunk, 8) > R.LDS_LIMIT
        assert (again is False) == over and n.lg == (4 if over else 8)


def test_no_c2cnet_geometry_selects_lg_8():
    """lg = 8 is chosen only when some conv has more than 1,024 (co, 4 positions) items:
    32 x Z / 4, 64 x Z / 8 or 128 x Z / 16 > 1,024, i.e. Z > 128.  At Z = 128 the six buffers
    (slot 128 x (Z / 4 + 6) + 16 = 4,880 floats) with the smallest weight chunks already take
    166 KB of the 160 KB, and the slot only grows with Z and with cin0: Net1D.build returns
    None before lg = 8 is ever needed.  c2c_net_kernel<8> is reachable through the ABI only."""
    from fvp.cnn import Net1D

    m = C.net_module(15, 1)
    assert Net1D.build(m, 15, 124).lg == 4
    for z in (128, 132, 256):
        assert Net1D.build(m, 15, z) is None
    assert R.lds_bytes(128 * (128 // 4 + 6) + 16, 6, 4096, 4) > R.LDS_LIMIT


def test_conv1d_net_argument_validation_without_gpu():
    """NULL and shape errors come back before any launch (fake non-null pointers)."""
    from fvp import _lib

    lib = _lib.load()
    f = lib.fvp_conv1d_net
    # (x, ncols, cin0, L0, prog, nops, params, slot, nbuf, wchunk, out_buf, cout_final, Lfinal, lg, y, stream)
    ok = dict(x=1, ncols=2, cin0=15, L0=20, prog=1, nops=3, params=1, slot=1424, nbuf=6, wchunk=12288, out_buf=0,
              cout_final=1, Lfinal=20, lg=4, y=1, stream=None)

    def call(**kw):
        return f(*{**ok, **kw}.values())

    for p in ("x", "prog", "params", "y"):
        assert call(**{p: None}) == 1001, p
    for name in ("ncols", "cin0", "L0", "nops", "slot", "nbuf", "cout_final", "Lfinal"):
        for v in (0, -1):
            assert call(**{name: v}) == 1002, (name, v)
    assert call(out_buf=-1) == 1002 and call(out_buf=6) == 1002
    assert call(slot=16 * 26 - 1) == 1002                      # the input's 16 x (20 + 6) floats
    assert call(cin0=17, slot=16 * 26) == 1002                 # 17 channels pad to 20 rows
    assert call(cout_final=55, slot=1424) == 1002              # the output's 55 x 26 floats
    assert call(Lfinal=1419, slot=1424) == 1002
    for w in (0, 4095, 4097, 16384, -4096):
        assert call(wchunk=w) == 1002, w
    for lg in (2, 16, 0, 6):
        assert call(lg=lg) == 1002, lg
    assert call(slot=4880, nbuf=6, wchunk=4096, L0=128, Lfinal=128) == 1002   # 166 KB
    assert call(slot=2832, nbuf=6, wchunk=8192, lg=8, L0=64, Lfinal=64) == 1002  # fits at lg 4 only
    for slot, nbuf, wchunk, lg in ((1424, 6, 12288, 4), (2832, 6, 8192, 8), (1, 1, 4096, 4)):
        assert lib.fvp_conv1d_net_lds_bytes(slot, nbuf, wchunk, lg) == 4 * (2 * wchunk + 1024 * lg + slot * nbuf) \
            == R.lds_bytes(slot, nbuf, wchunk, lg)
