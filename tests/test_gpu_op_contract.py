"""Every registered torch.ops.fvp op on the device: its fake kernel against the real call
(torch.library.opcheck), a compiled chain against eager, and the caller's stream.

Stream honouring.  An op must launch everything -- its kernels, the conversions of its operands,
the memset of the pre-zeroed person planes -- on the current stream.  Per case: the device
inputs hold seed A; on a non-blocking side stream a long sleep kernel is queued, then
copies of seed B into the same buffers, then the op.  Whatever does not go to the side stream
runs during the sleep and reads A, so the outputs then differ from the default-stream result
on B.  The sleep is 100 times the case's own default-stream wall time (enqueue plus execution)
and at least 5 ms.  Three controls queue the same sleep and copy but call the op on the default
stream: their results must be those of A, which shows on the machine that the test can fail.
The side stream is one that is seen to overlap the default stream (_side_stream says why a
fresh torch.cuda.Stream() need not).

Record (MI355X, gfx950, torch 2.10 ROCm): torch.cuda._sleep takes 0.418 ms per 10^6 cycles; the
largest default-stream case time was 0.074 ms (voxelize_cams-heatmaps-f64), so every case sleeps
between 5 and 7.4 ms.  With the control's procedure on 150 fresh streams in turn, every fourth
stream ran in order with the default stream (the default-stream call returned after 4.96 of the
5 ms sleep and read seed B); on the other three in four it read seed A within 0.02 ms.
"""
import time

import pytest
import torch

import op_cases as OC
from op_cases import CASES

pytestmark = pytest.mark.gpu

LAUNCHING = [c for c in CASES if c.launches]
OPCHECK_UTILS = ("test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_dynamic")


def _wrapper(case):
    from fvp import ops

    return getattr(ops, case.op)


def _tuple(out):
    return out if isinstance(out, tuple) else (out,)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return (a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape)
            and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)))


# ---------------------------------------------------------------------------
# a. opcheck: the fake kernel against the real call (shape, dtype, device, strides), the schema
# (no input mutated, no output aliasing an input) and the op under AOT dispatch
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_opcheck(gpu_device, case):
    utils = [u for u in OPCHECK_UTILS if u not in case.opcheck_off]
    assert "test_schema" in utils and "test_faketensor" in utils
    args = tuple(OC.real_args(case, gpu_device, 0))
    result = torch.library.opcheck(_wrapper(case).op, args, {}, test_utils=utils)
    assert result == {u: "SUCCESS" for u in utils}, result
    outs = _tuple(_wrapper(case)(*args))
    assert [(tuple(o.shape), o.dtype) for o in outs] == [tuple(o) for o in case.outs]  # the table itself
    ptrs = {a.data_ptr() for a in args if isinstance(a, torch.Tensor) and a.numel()}
    assert all(o.is_contiguous() and (o.numel() == 0 or o.data_ptr() not in ptrs) for o in outs)


# ---------------------------------------------------------------------------
# b. a compiled chain equals eager, dtypes included
_detect = OC.detection_chain


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_compiled_chain_equals_eager(gpu_device, dtype):
    """voxelize -> nms_topk_columns -> gather_bbox -> proposal_centers under torch.compile
    (aot_eager: no code generator) gives every output of the eager run bit for bit, dtype included."""
    case = next(c for c in CASES if c.id == "voxelize-f32")
    hm, packed = OC.real_args(case, gpu_device, 0)[:2]
    hm = hm.to(dtype)
    size = torch.rand((OC.B, 2, OC.X, OC.Y), generator=torch.Generator().manual_seed(5)).to(gpu_device)
    eager = _detect(hm, packed, size)
    torch._dynamo.reset()
    compiled = torch.compile(_detect, backend="aot_eager", fullgraph=True)(hm, packed, size)
    torch.cuda.synchronize(gpu_device)
    assert eager[0].dtype == torch.float32 and eager[3].dtype == torch.float16
    assert len(compiled) == len(eager)
    for i, (c, e) in enumerate(zip(compiled, eager)):
        assert c.dtype == e.dtype and _same_bits(c, e), f"output {i}: {c.dtype} vs {e.dtype}"


# ---------------------------------------------------------------------------
# c. the caller's stream
_SLEEP = {}


def _ms_per_cycle(dev) -> float:
    """torch.cuda._sleep's cycle in ms, measured once per session with device events."""
    if "ms" not in _SLEEP:
        torch.cuda._sleep(1000)
        torch.cuda.synchronize(dev)
        n = 100_000
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(n)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 2.0 or n >= 10 ** 9:
                break
            n *= 10
        assert ms > 0.0
        _SLEEP["ms"] = ms / n
        print(f"\n[op-contract] _sleep: {1e6 * _SLEEP['ms']:.3f} ms per 1e6 cycles (from {n} cycles)")
    return _SLEEP["ms"]


def _side_stream(dev):
    """A non-blocking stream that is seen to run beside the default stream.  HIP maps its streams
    onto a few hardware queues (4 unless GPU_MAX_HW_QUEUES says otherwise), and a stream that shares
    the null stream's queue runs in order with it (every fourth fresh torch.cuda.Stream() in the
    module's record): a launch that went to the null stream by mistake would then wait for the
    sleep and the copies like a correct one, and pass.  So each candidate goes through the
    control's procedure with torch's own kernels -- a sleep and a copy into a buffer on it, a read
    of the buffer on the default stream, which must see the old value and finish while the sleep
    still runs -- and the first that does serves every test of the session."""
    if "side" not in _SLEEP:
        cycles = int(20.0 / _ms_per_cycle(dev))
        ones = torch.ones(64, device=dev)
        for n in range(32):  # torch hands out its 32 pooled streams in turn
            side = torch.cuda.Stream(dev)
            buf = torch.zeros(64, device=dev)
            torch.cuda.synchronize(dev)
            with torch.cuda.stream(side):
                torch.cuda._sleep(cycles)
                buf.copy_(ones)
            seen = buf + 0.0
            torch.cuda.current_stream(dev).synchronize()
            overlapped = not side.query()
            side.synchronize()
            if overlapped and float(seen.sum()) == 0.0:
                _SLEEP["side"] = side
                print(f"\n[op-contract] side stream: candidate {n} runs beside the default stream")
                break
        else:
            pytest.fail("no torch.cuda.Stream() runs beside the default stream: the stream tests cannot tell")
    return _SLEEP["side"]


def _wall_ms(fn, dev) -> float:
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0)


def _sleep_cycles(wall_ms: float, dev) -> int:
    return int(max(5.0, 100.0 * wall_ms) / _ms_per_cycle(dev)) + 1


def _stream_setup(case, dev):
    """(op, ref = op(B), op(A), device buffers holding A, B's tensors, sleep cycles)."""
    op = _wrapper(case)
    a, b = OC.real_args(case, dev, 0), OC.real_args(case, dev, 1)
    ref, out_a = _tuple(op(*b)), _tuple(op(*a))
    torch.cuda.synchronize(dev)
    for i, (r, o) in enumerate(zip(ref, out_a)):
        assert r.numel() == 0 or not _same_bits(r, o), f"{case.id}: output {i} is the same for both seeds"
    wall = _wall_ms(lambda: op(*a), dev)  # warm: the two calls above loaded the code objects
    _SLEEP["max"] = max(_SLEEP.get("max", (0.0, "")), (wall, case.id))
    bufs = [t.clone() if isinstance(t, torch.Tensor) else t for t in a]
    torch.cuda.synchronize(dev)
    return op, ref, out_a, bufs, b, _sleep_cycles(wall, dev)


def _sleep_then_copy(cycles, bufs, b):
    """On the current stream: the sleep, then seed B into the buffers."""
    torch.cuda._sleep(cycles)
    for dst, src in zip(bufs, b):
        if isinstance(dst, torch.Tensor):
            dst.copy_(src)


@pytest.mark.parametrize("case", LAUNCHING, ids=[c.id for c in LAUNCHING])
def test_op_runs_on_the_current_stream(gpu_device, case):
    op, ref, _, bufs, b, cycles = _stream_setup(case, gpu_device)
    side = _side_stream(gpu_device)
    with torch.cuda.stream(side):
        _sleep_then_copy(cycles, bufs, b)
        out = _tuple(op(*bufs))
        side.synchronize()
    torch.cuda.synchronize(gpu_device)
    for i, (o, r) in enumerate(zip(out, ref)):
        assert _same_bits(o, r), f"{case.id}: output {i} was not computed from the side stream's inputs"


@pytest.mark.parametrize("case_id", ["gather_columns-f32", "nms_topk-f32", "render_keypoints-f64-joints"])
def test_control_default_stream_call_reads_the_stale_inputs(gpu_device, case_id):
    """The same sleep and copy on the side stream, the op on the DEFAULT stream: it runs during the
    sleep and reads seed A (valid values throughout), so its result is op(A), not the reference."""
    case = next(c for c in CASES if c.id == case_id)
    op, ref, out_a, bufs, b, cycles = _stream_setup(case, gpu_device)
    side = _side_stream(gpu_device)
    with torch.cuda.stream(side):
        _sleep_then_copy(cycles, bufs, b)
    out = _tuple(op(*bufs))  # outside the block: on the default stream
    side.synchronize()
    torch.cuda.synchronize(gpu_device)
    for i, (o, r, oa) in enumerate(zip(out, ref, out_a)):
        assert not _same_bits(o, r), f"{case_id}: output {i} equals the reference: the side stream blocked the call"
        assert _same_bits(o, oa), f"{case_id}: output {i} is neither op(A) nor op(B)"


# The pre-zeroed person planes, through the C ABI with a caller-owned planes buffer: the cases whose
# operands already have the ABI's types (the ops convert nothing) and that ask for the planes.
def _abi_typed(case) -> bool:
    if case.op not in ("person_planes", "person_planes_cams", "person_planes_cl"):
        return False
    a = case.args
    if not (case.launches and a["want_planes"]) or (a["frame_of"] is not None and a["frame_of"].dtype != torch.int32):
        return False
    floats = [v for k, v in a.items() if isinstance(v, OC.T) and k not in ("frame_of", "heatmaps_cl")]
    return all(v.dtype == torch.float32 for v in floats)


PLANE_CASES = [c for c in CASES if _abi_typed(c)]


def _abi_person_planes(case, a, cubes, planes, offset, ws, stream):
    from fvp import _lib
    from fvp.ops import _f3, _i3, _ptr

    spec = _lib.PersonSpec(_i3(a["fine"]), _f3(a["scale"]), _f3(a["bias"]), _f3(a["whole_size"]), _f3(a["ind_size"]),
                           _i3(a["bins"]))
    P = a["proposals"].shape[0]
    tail = (_ptr(a["proposals"]), _ptr(a["frame_of"]), P, _ptr(cubes), _ptr(planes), _ptr(offset))
    if case.op == "person_planes_cl":
        hm = a["heatmaps_cl"]
        B, V, H, W, cp = hm.shape
        name = "fvp_person_planes_cl_f16" if hm.dtype == torch.float16 else "fvp_person_planes_cl"
        _lib.call(name, _ptr(hm), cp, B, V, a["J"], H, W, _ptr(a["fine_grid"]), spec, *tail, stream)
        return
    hm = a["heatmaps"]
    B, V, J, H, W = hm.shape
    if case.op == "person_planes":
        _lib.call("fvp_person_planes", _ptr(hm), B, V, J, H, W, _ptr(a["fine_grid"]), spec, *tail, _ptr(ws),
                  ws.numel() * 4, stream)
    else:
        g = _lib.GridSpec(_f3(a["start"]), _f3(a["end"]), _f3(a["center"]), _i3(a["fine"]))
        im = _lib.ImageSpec(a["ori_max"], a["img_w"], a["img_h"], W, H)
        _lib.call("fvp_person_planes_cams", _ptr(hm), B, V, J, H, W, _ptr(a["cams"]), _ptr(a["resize_t"]), g, im, spec,
                  *tail, _ptr(ws), ws.numel() * 4, stream)


@pytest.mark.parametrize("case", PLANE_CASES, ids=[c.id for c in PLANE_CASES])
def test_person_planes_are_zeroed_on_the_callers_stream(gpu_device, case):
    """fvp_person_planes / _cams / _cl / _cl_f16 with the caller's planes buffer, filled with 2.0 on
    the side stream after the sleep.  The entry point zeroes the planes before its kernel takes
    atomicMax into them; a memset on another stream would run during the sleep and be overwritten
    by the fill, and the maxima (heatmaps are below 1) would then leave 2.0 behind."""
    from fvp import _lib, ops

    kind = {"person_planes": "planar", "person_planes_cams": "cams"}.get(case.op)
    names = list(case.args)
    a = dict(zip(names, OC.real_args(case, gpu_device, 1)))
    hm = a["heatmaps_cl"] if case.op == "person_planes_cl" else a["heatmaps"]
    if kind is None:
        kind = "cl_f16" if hm.dtype == torch.float16 else "cl"
    B, V = hm.shape[:2]
    J, H, W = (a["J"], hm.shape[2], hm.shape[3]) if kind.startswith("cl") else tuple(hm.shape[2:])
    P = a["proposals"].shape[0]
    st, plan = ops.person_plan(kind, B, V, J, H, W, a["bins"], a["fine"], P, want_cubes=a["want_cubes"],
                               want_planes=True, cp=hm.shape[4] if kind.startswith("cl") else 0)
    assert st == 0 and plan and plan[0].zeroed_planes > 0, "this shape does not pre-zero its planes"
    ref = _tuple(_wrapper(case)(*a.values()))
    ws_bytes = 0 if kind.startswith("cl") else _lib.load().fvp_person_workspace_bytes(B, V, J, H, W)
    ws = torch.empty(((ws_bytes + 3) // 4,), dtype=torch.float32, device=gpu_device)
    cubes = torch.empty_like(ref[0]) if a["want_cubes"] else None
    planes, offset = torch.empty_like(ref[1]), torch.empty_like(ref[2])
    wall = _wall_ms(lambda: _abi_person_planes(case, a, cubes, planes, offset, ws,
                                               torch.cuda.current_stream(gpu_device).cuda_stream), gpu_device)
    assert _same_bits(planes, ref[1])  # the direct call is the op's
    cycles = _sleep_cycles(wall, gpu_device)
    side = _side_stream(gpu_device)
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        planes.fill_(2.0)
        _abi_person_planes(case, a, cubes, planes, offset, ws, side.cuda_stream)
        side.synchronize()
    torch.cuda.synchronize(gpu_device)
    assert float(planes.max()) < 2.0, "a fill value survived: the planes were not zeroed on the caller's stream"
    assert _same_bits(planes, ref[1]) and _same_bits(offset, ref[2])
    if cubes is not None:
        assert _same_bits(cubes, ref[0])


def test_case_times_stay_short(gpu_device):
    """Prints the calibration and the slowest case of this run (-s shows it); the sleeps are 100
    times a case's time, so a case that takes 10 ms on the default stream would sleep a second."""
    ms = _ms_per_cycle(gpu_device)
    wall, cid = _SLEEP.get("max", (0.0, "none"))
    print(f"\n[op-contract] _sleep {1e6 * ms:.3f} ms per 1e6 cycles; largest default-stream case time "
          f"{wall:.3f} ms ({cid}), slept {max(5.0, 100.0 * wall):.1f} ms")
    assert 100.0 * wall < 1000.0, f"{cid}: {wall} ms on the default stream makes its sleep longer than a second"
