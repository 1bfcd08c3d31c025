"""A second and a third way of running the memory-contract cases (tests/golden/memory_contract.py): every launch behind a delay on
a side stream, and every launch captured into a graph on one stream and replayed.  Both go in through memory_contract's hooks
(DEFAULT_LAUNCH, RECORD), which only the context manager `hooks` here sets, and resets.

delayed(side, real_call, cycles) -> launch(name, *args).  On stream `side`: clone every `const` tensor argument and zero the
original (the poison: index 0 and 0.0f are in bounds and finite, a kernel that runs early still reads valid memory), spin for
`cycles`, copy the clones back, record the event `restored`, call real_call, and assert that `restored` has NOT happened yet: the
delay was long enough for a kernel that is not ordered behind `side` to have read the poison, and the entry point did not block
the host.  In-out parameters, the state bytes of a workspace and the outputs are left alone.

replaying(real_call) -> launch(name, *args).  One eager call on a side stream (warm-up, and the first set of expected values), one
capture of exactly one real_call on one stream (no fork, no second stream, no wait inside), then
  replay 1 with every writable non-in-out tensor and every workspace byte past `keep` refilled with 0xFF: the eager bits;
  replay 2 on the workspace replay 1 left, the `const` tensors overwritten IN PLACE with a second draw (floats uniform in the first
  draw's own [min, max], indices uniform in theirs: positive stays positive, an index stays in bounds): the bits of an eager call
  on those values from a freshly armed workspace.  A ticket that is not re-armed and a host decision taken from device data at
  capture time both show here;
  replay 3 on the first values again, which is what the case goes on to hold to its value bar.
In-out parameters are reset to their precondition before every run.  Only the spec's `open` ranges and `bound` apply, through
memory_contract.compare_runs as check() applies them."""
import contextlib
import time

import torch

import memory_contract as mc
from memory_contract import ContractError

SLEEP_MS = 4.0                # the delay in front of every launch of the side-stream run (LABLOG R30.1: how it was arrived at)
_CYCLES_PER_MS = {}
HOST_MS = []                  # (entry point, milliseconds of host time between enqueuing the delay and the entry point's return)


def cycles_per_ms(device=None):
    """torch.cuda._sleep counts ticks of a device clock whose rate is not the same everywhere: timed once per device, with events"""
    dev = torch.cuda.current_device() if device is None else device
    if dev not in _CYCLES_PER_MS:
        n = 2_000_000
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(n)
        b.record()
        b.synchronize()
        _CYCLES_PER_MS[dev] = n / max(a.elapsed_time(b), 1e-3)
    return _CYCLES_PER_MS[dev]


def sleep_cycles(ms=SLEEP_MS):
    return int(ms * cycles_per_ms())


@contextlib.contextmanager
def hooks(default_launch=None, record=None, grid_stats=None):
    """memory_contract's hooks for the time of the block; grid_stats: what stands in for mc.launch_grid_stats, the one launch a case
    passes by hand"""
    saved = (mc.DEFAULT_LAUNCH, mc.RECORD, mc.launch_grid_stats)
    mc.DEFAULT_LAUNCH, mc.RECORD = default_launch, record
    if grid_stats is not None:
        mc.launch_grid_stats = grid_stats
    try:
        yield
    finally:
        mc.DEFAULT_LAUNCH, mc.RECORD, mc.launch_grid_stats = saved


def _active(name, proto, contract):
    if proto is None:
        assert mc.ACTIVE is not None and mc.ACTIVE[0] == name, f"{name}: launched outside check() and without a prototype"
        _, proto, contract, _ = mc.ACTIVE
    return proto, contract


def _classify(name, args, proto, contract):
    """-> values, consts [(param, tensor)], writable [(param, tensor, spec, in-out for this call)]"""
    params = proto.params
    values = {p.name: a for p, a in zip(params, args)}
    consts, writable = [], []
    for p, a in zip(params, args):
        if not isinstance(a, torch.Tensor):
            continue
        if mc.is_writable(p):
            spec = mc.spec_of(name, p.name, contract)
            inout = spec.kind == "inout" and (spec.inout_when is None or spec.inout_when(values))
            writable.append((p, a, spec, inout))
        else:
            consts.append((p, a))
    return values, consts, writable


# ------------------------------------------------------------------------------------------------------------------------------
def delayed(side, real_call, cycles, proto=None, contract=None):
    def launch(name, *args, **kw):
        pr, ct = _active(name, proto, contract)
        _, consts, _ = _classify(name, args, pr, ct)
        side.wait_stream(torch.cuda.default_stream())
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            saved = [(a, a.clone()) for _, a in consts]
            for a, _ in saved:
                a.zero_()
            t0 = time.perf_counter()
            torch.cuda._sleep(cycles)
            for a, keep in saved:
                a.copy_(keep)
            restored = torch.cuda.Event()
            restored.record(side)
            out = real_call(name, *args, **kw)
            early = restored.query()
            HOST_MS.append((name, 1e3 * (time.perf_counter() - t0)))
        assert not early, (f"{name}: the inputs were restored before the entry point returned: it blocked the host, or the delay of "
                           f"{cycles} cycles is too short to order anything")
        return out
    return launch


def compare_records(plain, other, what):
    """two RECORD lists of the same case: every check() of it, output by output"""
    assert len(plain) == len(other), f"{what}: {len(other)} check() calls, the plain run made {len(plain)}"
    for (name, values, w1), (name2, _, w2) in zip(plain, other):
        assert name == name2 and set(w1) == set(w2), (name, name2)
        mc.compare_runs(name, values, what, [(k, a, s) for k, (a, s) in w2.items()], "the plain run on the default stream",
                        [(k, a, s) for k, (a, s) in w1.items()])


# ------------------------------------------------------------------------------------------------------------------------------
def _raw(t):
    return t.view(-1).view(torch.uint8) if t.dtype != torch.uint8 else t.view(-1)


def _second_draw(t, gen):
    """a tensor of t's shape and dtype drawn again inside t's own range"""
    if t.numel() == 0:
        return t.clone()
    if t.dtype.is_floating_point:
        lo, hi = float(t.double().min()), float(t.double().max())
        if not (lo == lo and hi == hi) or abs(lo) == float("inf") or abs(hi) == float("inf"):
            return t.clone()
        u = torch.rand(t.shape, generator=gen, dtype=torch.float64)
        return (lo + (hi - lo) * u).to(t.dtype).clamp_(lo, hi).to(t.device)
    if t.dtype == torch.bool:
        return t.clone()
    lo, hi = int(t.min()), int(t.max())
    return torch.randint(lo, hi + 1, t.shape, generator=gen).to(t.dtype).to(t.device)


def replaying(real_call, proto=None, contract=None, stats=None):
    def launch(name, *args, **kw):
        pr, ct = _active(name, proto, contract)
        values, consts, writable = _classify(name, args, pr, ct)
        pre = [(a, a.clone()) for _, a, _, inout in writable if inout]
        first = [(a, a.clone()) for _, a in consts]

        def prepare(fill=True, arm=False):
            for _, a, spec, inout in writable:
                if inout:
                    continue
                raw = _raw(a)
                if fill:
                    raw[spec.keep:].fill_(mc.FILL_A)
                if arm and spec.keep:
                    raw[:spec.keep].zero_()
            for a, was in pre:
                a.copy_(was)

        def outputs():
            torch.cuda.synchronize()
            return [(p.name, a.clone(), spec) for p, a, spec, _ in writable]

        def eager():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                real_call(name, *args, **kw)
            torch.cuda.current_stream().wait_stream(side)
            return outputs()

        prepare(fill=False)
        want1 = eager()                                       # the warm-up, on the memory as the case prepared it
        prepare(fill=False)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            real_call(name, *args, **kw)
        if stats is not None:
            stats.append(name)

        prepare(arm=True)                                     # replay 1 is a first call: the state bytes as the header wants them
        graph.replay()
        mc.compare_runs(name, values, "replay 1", outputs(), "the eager call", want1)

        gen = torch.Generator().manual_seed(9000 + sum(map(ord, name)))
        for a, _ in first:
            a.copy_(_second_draw(a, gen))
        prepare(fill=False)                                   # (the workspace stays as replay 1 left it)
        graph.replay()
        got2 = outputs()
        prepare(arm=True)
        mc.compare_runs(name, values, "replay 2, on a second draw of the inputs written in place", got2,
                        "an eager call on those values", eager())

        for a, was in first:
            a.copy_(was)
        prepare(fill=False)
        graph.replay()
        torch.cuda.synchronize()
    return launch


def replayed(name, build, real_call=None, proto=None, contract=None, sizefn=None):
    """one entry point with the arguments build(arena), as check() takes them, through `replaying`: -> its writable tensors after the
    last replay, {parameter: tensor}"""
    if real_call is None:
        from learning3d_amd import _lib
        real_call = _lib.call
    proto = proto or mc.prototypes()[name]
    arena = mc.Arena(mc.FILL_B)
    values, writable = mc._run(name, proto, build, replaying(real_call, proto, contract), arena, contract, sizefn)
    return {p.name: a for p, a, _ in writable}
