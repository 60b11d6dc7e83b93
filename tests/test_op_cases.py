"""Every registered torch.ops.fvp op against the case table (tests/op_cases.py), without a GPU.

Under a FakeTensorMode with fake "cuda" inputs -- what torch.compile and export trace with --
the registered op's fake kernel must describe what the implementation returns: the table's
shape and dtype (written from the implementation's allocation statements), on the inputs'
device, contiguous.  tests/test_gpu_op_contract.py makes the fake-against-real comparison on
a device; this file is the half that needs none.
"""
import inspect

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensor, FakeTensorMode

import op_cases as OC
from op_cases import CASES


def _wrappers():
    """{name: wrapper} of every fvp.ops name that carries a registered op."""
    from fvp import ops

    return {n: f for n, f in vars(ops).items() if callable(f) and hasattr(f, "op") and hasattr(f, "impl")}


def test_every_registered_op_has_cases():
    """The ops with cases are exactly the registered ones: a new op without a case fails here."""
    registered = OC.registered_ops()
    assert len(registered) == 26, registered
    assert OC.OPS_WITH_CASES == registered
    assert sorted(_wrappers()) == registered


def test_every_wrapper_carries_its_registered_op():
    """wrapper.op is the CustomOpDef registered under the wrapper's own name."""
    for name, f in _wrappers().items():
        assert isinstance(f.op, torch._library.custom_ops.CustomOpDef), name
        assert f.op._qualname == f"fvp::{name}", (name, f.op._qualname)
        assert f.impl is not f and callable(f.impl)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_arguments_follow_the_signature(case):
    """The table's argument names are the op's parameters, in order (they are passed by position)."""
    params = list(inspect.signature(_wrappers()[case.op].impl).parameters)
    assert list(case.args) == params


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_inputs_are_small(case):
    for name, a in case.args.items():
        if isinstance(a, OC.T):
            nbytes = torch.empty((), dtype=a.dtype).element_size() * int(torch.Size(a.shape).numel())
            assert nbytes <= 64 * 1024, (name, nbytes)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_fake_kernel_gives_the_implementation_outputs(case):
    """The wrapper, called on fake tensors, routes to the registered op, whose fake kernel must
    give the implementation's outputs: shape, dtype, the inputs' device, contiguous."""
    wrapper = _wrappers()[case.op]
    with FakeTensorMode():
        args = OC.fake_args(case)
        outs = wrapper(*args)
        direct = getattr(torch.ops.fvp, case.op)(*args)
    outs = outs if isinstance(outs, tuple) else (outs,)
    direct = direct if isinstance(direct, tuple) else (direct,)
    assert len(outs) == len(direct) == len(case.outs)
    for i, (o, d, (shape, dtype)) in enumerate(zip(outs, direct, case.outs)):
        for t in (o, d):
            assert isinstance(t, FakeTensor), f"output {i}: {type(t)} (the wrapper did not route to the op)"
            assert tuple(t.shape) == shape, f"output {i}: fake shape {tuple(t.shape)}, implementation {shape}"
            assert t.dtype == dtype, f"output {i}: fake dtype {t.dtype}, implementation {dtype}"
            assert t.device.type == "cuda", f"output {i}: on {t.device}"
            assert t.is_contiguous(), f"output {i}: strides {t.stride()}"


def test_real_args_are_valid_and_differ_between_seeds():
    """real_args on the CPU: the specs' shapes and dtypes, indices and counts in range, heatmaps
    in [0, 1), and two seeds differing in every tensor argument that has elements."""
    for case in CASES:
        a, b = OC.real_args(case, "cpu", 0), OC.real_args(case, "cpu", 1)
        for (name, spec), x, y in zip(case.args.items(), a, b):
            if not isinstance(spec, OC.T):
                assert x == y == spec or (x is None and spec is None)
                continue
            assert tuple(x.shape) == tuple(spec.shape) and x.dtype == spec.dtype, (case.id, name)
            if x.numel():
                assert not torch.equal(x, y), (case.id, name)
            kind = spec.fill if isinstance(spec.fill, tuple) else (spec.fill,)
            for t in (x, y):
                if t.numel() == 0:
                    continue
                if kind[0] == "index":
                    assert 0 <= int(t.min()) and int(t.max()) < kind[1], (case.id, name)
                elif kind[0] == "count":
                    assert 1 <= int(t.min()) and int(t.max()) <= kind[1], (case.id, name)
                elif kind[0] == "unit":
                    assert 0.0 <= float(t.min()) and float(t.max()) <= 1.0, (case.id, name)
                elif t.is_floating_point():
                    assert bool(torch.isfinite(t).all()), (case.id, name)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_dynamo_traces_the_chain_to_the_registered_ops(dtype):
    """torch.compile(fullgraph=True) of the detection chain, stopped at the backend (nothing runs,
    so no device is needed): the graph calls the four registered ops and carries the
    implementation's dtypes -- an fp32 cube, and an fp32 sum of it, from fp16 heatmaps too."""
    class Stop(Exception):
        pass

    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        raise Stop

    torch._dynamo.reset()
    hm = torch.rand((OC.B, OC.V, OC.J, OC.H, OC.W)).to(dtype)
    with pytest.raises(Exception) as err:
        torch.compile(OC.detection_chain, backend=backend, fullgraph=True)(
            hm, torch.rand((OC.N, OC.GV, 2)), torch.rand((OC.B, 2, OC.X, OC.Y)))
    assert "Stop" in repr(err.value) and len(graphs) == 1
    torch._dynamo.reset()
    nodes = list(graphs[0].graph.nodes)
    called = [n.target for n in nodes if n.op == "call_function"]
    for name in ("voxelize", "nms_topk_columns", "gather_bbox", "proposal_centers"):
        assert getattr(torch.ops.fvp, name).default in called, name
    outs = [n.meta["example_value"] for n in nodes[-1].args[0]]
    want = [torch.float32, torch.float32, torch.float32, torch.float16, torch.float32, torch.int64, torch.int64,
            torch.float32, torch.float32, torch.float32]
    assert [o.dtype for o in outs] == want
    assert tuple(outs[0].shape) == (OC.B, OC.J, OC.X, OC.Y, OC.Z) and tuple(outs[7].shape) == (OC.B, OC.K, OC.J, OC.Z)
