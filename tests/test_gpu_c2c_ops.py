"""The one-launch 1-D net kernel (csrc/fvp_c2c.hip: c2c_net_kernel<4> / <8> behind
fvp_conv1d_net) held op by op to the float64 reference and derived bound of tests/c2c_ref.py
on the case list of tests/c2c_cases.py (tests/test_c2c_ref.py shows on the CPU that the bound
holds for a correct fp32 evaluation and that planted faults leave it).

Stepwise.  A program of n ops is launched as its n prefixes (the same prog and params,
nops = o + 1, out_buf / cout_final / Lfinal those of op o's dst).  Op o is then checked with
op_reference() on the kernel's own fp32 outputs of its src, res_pre and res_post, as the
earlier prefixes returned them (the launches are bit-reproducible: asserted).  By induction
every intermediate activation is within its per-op bound, nothing compounds, and the pools
are held bit for bit.  Every case runs at every lg it is legal at.
"""
import collections

import numpy as np
import pytest
import torch

import c2c_cases as C
import c2c_ref as R

pytestmark = pytest.mark.gpu

CASES = C.all_cases()
PARAMS = [pytest.param(c, lg, id=f"{c.name}@lg{lg}") for c in CASES for lg in C.legal_lgs(c)]
REL = 2e-5  # tests/test_cnn_1d_weight.py's criterion: max error of the output's max magnitude
RATIOS = collections.defaultdict(float)  # (k | "t", lg) -> the largest error / tol seen (reported, not asserted)


def _launch(net, x, nops, out_buf, c, ln, lg):
    """fvp_conv1d_net on the first nops ops; buffer out_buf's [c][ln] per column (NaN-filled
    first, so an element the kernel does not write shows)."""
    from fvp import _lib
    from fvp.cnn import _ptr, _stream

    x = x.float().contiguous()
    y = torch.full((x.shape[0], c, ln), float("nan"), dtype=torch.float32, device=x.device)
    _lib.call("fvp_conv1d_net", _ptr(x), x.shape[0], net.cin0, net.L0, _ptr(net.prog), nops, _ptr(net.param),
              net.slot, net.nbuf, net.wchunk, out_buf, c, ln, lg, _ptr(y), _stream(y))
    return y.cpu().numpy()


def _prefixes(net, x, lg):
    """[the output of op o, fetched by the prefix launch o + 1]."""
    outs = []
    for o, op in enumerate(net.ops):
        c = op[R.CIN] if op[R.KIND] == R.POOL else op[R.COUT]
        outs.append(_launch(net, x, o + 1, op[R.DST], c, R.out_len(op), lg))
    return outs


def _stepwise(case, lg, x, dev):
    """Checks every op of the case on input x [N][cin0][L0] (numpy); -> the prefix outputs."""
    net = C.build(case, lg, dev)
    assert net is not None
    par = net.param.cpu().numpy()
    outs = _prefixes(net, torch.from_numpy(x).to(dev), lg)
    hold = {0: np.pad(x, ((0, 0), (0, -case.cin0 % 4), (0, 0)))}  # buffer -> what it holds now
    for o, (op, got) in enumerate(zip(net.ops, outs)):
        op = tuple(op)
        ins = [hold[op[R.SRC]]] + [hold[b] if b >= 0 else None for b in (op[R.RES_PRE], op[R.RES_POST])]
        try:
            ratio = R.check_op(op, par, *ins, got, lg)
        except AssertionError as e:
            raise AssertionError(f"{case.name} lg {lg} op {o} {op}: {e}") from None
        if op[R.KIND] != R.POOL:
            key = ("t" if op[R.KIND] == R.CONVT else op[R.K], lg)
            RATIOS[key] = max(RATIOS[key], ratio)
        hold[op[R.DST]] = got
    return net, outs


def test_prefix_launches_are_bit_reproducible(gpu_device):
    case = next(c for c in CASES if c.name == "net15-1-z20")
    for lg in C.LGS:
        net = C.build(case, lg, gpu_device)
        x = torch.from_numpy(C.inputs(case)).to(gpu_device)
        a, b = _prefixes(net, x, lg), _prefixes(net, x, lg)
        assert len(a) == 25 and all(R.same_bits(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("case,lg", PARAMS)
def test_every_op_within_its_bound(gpu_device, case, lg):
    x = C.inputs(case)
    net, outs = _stepwise(case, lg, x, gpu_device)
    assert np.isfinite(outs[-1]).all()
    # the whole program, as Net1D launches it, is the last prefix
    assert net.lg == lg
    y = net(torch.from_numpy(x).to(gpu_device)).cpu().numpy()
    assert R.same_bits(y, outs[-1])
    if case.group == "reuse":
        big, b = C.reused_buffer(net)
        assert big == b and np.abs(outs[0]).min() > 1e29  # the 1e30 rows were there, and are gone
    if case.net:
        with torch.no_grad():
            ref = C.net_module(*case.net).double()(torch.from_numpy(x).double()).numpy()
        err = np.abs(y - ref).max() / max(np.abs(ref).max(), 1e-6)
        assert err <= REL, f"{case.name} at lg {lg}: {err:.3g} of the output scale against the float64 module"


@pytest.mark.parametrize("case,lg", PARAMS)
def test_columns_do_not_mix(gpu_device, case, lg):
    """Three different columns, the middle one all NaN: the others come out bit-identical to
    their single-column launches, the NaN column all NaN."""
    net = C.build(case, lg, gpu_device)
    x = C.inputs(case)
    x[1] = np.nan
    xt = torch.from_numpy(x).to(gpu_device)
    y = net(xt).cpu().numpy()
    assert np.isnan(y[1]).all()
    for col in (0, 2):
        one = net(xt[col:col + 1]).cpu().numpy()
        assert np.isfinite(one).all() and R.same_bits(y[col], one[0]), f"column {col}"


NF = C.nonfinite_cases()


@pytest.mark.parametrize("case,lg", [pytest.param(c, lg, id=f"{c.name}@lg{lg}") for c in NF for lg in C.LGS])
def test_non_finite_inputs_per_op(gpu_device, case, lg):
    """A NaN makes exactly its receptive field NaN, +Inf goes through positive weights and the
    ReLU, -Inf behind the ReLU gives 0, a NaN in res_pre / res_post stays where it is (the
    ReLU between them keeps it), and a pool propagates a NaN from either slot -- check_op()
    holds every other output to the bound of the reference without the non-finite element."""
    x = C.nonfinite_inputs(case)
    net, outs = _stepwise(case, lg, x, gpu_device)
    y = outs[-1]
    if case.name == "nf-res":
        rp, rq = outs[0], outs[1]
        for r, at in zip((rp, rq), C.NF_RES):
            assert [tuple(i[1:]) for i in np.argwhere(np.isnan(r))] == [at] * 3
        assert sorted({tuple(i[1:]) for i in np.argwhere(~np.isfinite(y))}) == sorted(C.NF_RES)
        assert np.isnan(y[:, 2, 4]).all() and np.isnan(y[:, 5, 7]).all()
    elif case.name == "nf-pool":
        p = outs[0]
        assert [tuple(i) for i in np.argwhere(np.isnan(p))] == [(0, 1, 1), (0, 2, 2)]
        assert [tuple(i) for i in np.argwhere(np.isnan(y).all(axis=1))] == [(0, 1), (0, 2)]
        assert np.isfinite(y[1:]).all()
    else:
        op = net.ops[0]
        c, at = C.NF_AT
        if op[R.KIND] == R.CONVT:
            field = [2 * at, 2 * at + 1]
        else:
            p = (op[R.K] - 1) // 2
            field = list(range(at - p, at + p + 1))
        rest = [l for l in range(y.shape[2]) if l not in field]
        assert np.isnan(y[0][:, field]).all() and np.isfinite(y[0][:, rest]).all()
        assert (y[1][:, field] == np.inf).all() and np.isfinite(y[1][:, rest]).all()
        assert (y[2][:, field] == 0).all() and np.isfinite(y[2]).all()


def test_report_largest_error_to_bound_ratios():
    """Not a criterion: prints what the stepwise tests saw (run with -s)."""
    for key in sorted(RATIOS, key=str):
        print(f"c2c ops: k {key[0]} lg {key[1]}: largest error / tol {RATIOS[key]:.3f}")
