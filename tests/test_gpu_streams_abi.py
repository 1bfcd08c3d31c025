"""Every stream-taking entry point of the C ABI on a side stream and in a replayed graph: the memory-contract cases
(tests/test_gpu_memory_contract.py::CASES, and the memory-contract tests of the include/ext entry points where they live) run a
second time with every launch behind a delay on a side stream, its `const` inputs poisoned until the delay ends, and a third time
with every launch captured on one stream and replayed (tests/golden/stream_cases.py).  A launch that is not put on the stream it
was given, a ticket that is not re-armed between two replays and a host decision taken from device data at capture time fail here;
none of them can be seen by an eager run on the default stream.

Not marked gpu: the accounting tests (every stream-taking prototype is in both runs, or in the pinned NOT_CAPTURED)."""
import importlib
import inspect
import itertools
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import memory_contract as mc                                                            # noqa: E402
import stream_cases as sc                                                               # noqa: E402
import test_gpu_memory_contract as contract_cases                                       # noqa: E402
from memory_contract import ContractError, Spec, check                                  # noqa: E402
from test_gpu_memory_contract import FAKE, FAKE_CONTRACT, Param, Proto, _fake_size      # noqa: E402

gpu = pytest.mark.gpu
CASES = contract_cases.CASES

# ------------------------------------------------------------------------------------------------------------------------------
# the include/ext entry points: their memory-contract tests, called as they stand (each one's own parameter sets)
EXT_TESTS = [("test_gpu_rpmnet", "test_memory_contract_ppf_group_and_rigid_and_affine"), ("test_gpu_rpmnet", "test_memory_contract_gn_conv"),
             ("test_gpu_rpmnet", "test_memory_contract_sinkhorn"), ("test_gpu_rpmnet_match", "test_memory_contract"),
             ("test_gpu_rpmnet_train", "test_memory_contract"), ("test_gpu_rpmnet_param", "test_memory_contract"),
             ("test_gpu_prnet", "test_memory_contract_keypoints"), ("test_gpu_prnet", "test_memory_contract_soft_correspondence_pair"),
             ("test_gpu_partial", "test_memory_contract"), ("test_gpu_pointconv", "test_memory_contract_aggregate")]


def _names_of(code):
    yield from code.co_names
    for c in code.co_consts:
        if inspect.iscode(c):
            yield from _names_of(c)


def _ext_entries(fn):
    """the stream-taking include/ext entry points a test names: as a string, or through a module constant (NAME, KP, PAIR)"""
    from learning3d_amd import _lib
    launching = {n for n, p in _lib.EXT_PROTOTYPES.items() if mc.has_stream(p)}
    named = set(re.findall(r"\"(l3d_\w+)\"", inspect.getsource(fn)))
    named |= {v for v in (fn.__globals__.get(n) for n in _names_of(fn.__code__)) if isinstance(v, str)}
    return tuple(sorted(named & launching))


def _ext_cases():
    out = {}
    for module, test in EXT_TESTS:
        fn = getattr(importlib.import_module(module), test)
        marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        names = [[n.strip() for n in m.args[0].split(",")] for m in marks]
        sets = [[v if isinstance(v, (tuple, list)) and len(n) > 1 else (v,) for v in m.args[1]] for m, n in zip(marks, names)]
        for combo in itertools.product(*sets):
            kw = {k: v for n, vs in zip(names, combo) for k, v in zip(n, vs)}
            ident = f"{module[9:]}.{test[5:]}" + "".join(f"-{v}" for v in kw.values())
            assert ident not in out and ident not in CASES, ident
            out[ident] = (_ext_entries(fn), (lambda fn, kw: lambda: fn(**kw))(fn, kw))
    return out


EXT_CASES = _ext_cases()
ALL_CASES = {**CASES, **EXT_CASES}

# An entry point that must not be captured: ident -> "file:line, why", decided by reading its host code (an entry that reads device
# memory on the host, or that its header calls host-only).  learning3d_amd/csrc holds no hipMemcpy, hipStreamSynchronize or
# hipDeviceSynchronize and no entry point reads a device value on the host: the table is empty.
NOT_CAPTURED = {}
PINNED_NOT_CAPTURED = frozenset()


_SEEN_EXT = {}


def _launched_as_declared(ident, launched):
    """a case of CASES launches exactly the entry points it is registered under; a parameter set of an include/ext test launches some
    of those its text names (a pooled layer has a winner kernel, a plain one has not): the union is held by the last test below"""
    declared = set(ALL_CASES[ident][0])
    if ident in EXT_CASES:
        assert launched and launched <= declared, f"{ident} names {sorted(declared)}, its check() calls were {sorted(launched)}"
        _SEEN_EXT[ident] = launched
    else:
        assert launched == declared, f"{ident} names {sorted(declared)}, its check() calls were {sorted(launched)}"


def _run_case(ident, **hook):
    """the case under the hooks -> (its records, the AssertionError of its own value bars if one was raised)"""
    records, failed = [], None
    with sc.hooks(record=records, **hook):
        try:
            ALL_CASES[ident][1]()
        except AssertionError as e:
            failed = e
    return records, failed


@gpu
@pytest.mark.parametrize("ident", sorted(ALL_CASES))
def test_entry_point_runs_on_the_stream_it_is_given(ident):
    from learning3d_amd import _lib
    plain, failed = _run_case(ident)
    if failed is not None:
        raise failed
    _launched_as_declared(ident, {r[0] for r in plain})
    side = torch.cuda.Stream()
    cycles = sc.sleep_cycles()
    side.wait_stream(torch.cuda.default_stream())
    with torch.cuda.stream(side):
        other, failed = _run_case(ident, default_launch=sc.delayed(side, _lib.call, cycles),
                                  grid_stats=sc.delayed(side, mc.launch_grid_stats, cycles))
    torch.cuda.synchronize()
    sc.compare_records(plain, other, "the run on a side stream behind a delay")       # (first: it names the parameter)
    if failed is not None:
        raise failed


@gpu
@pytest.mark.parametrize("ident", sorted(set(ALL_CASES) - set(NOT_CAPTURED)))
def test_entry_point_replays(ident):
    from learning3d_amd import _lib
    captured = []
    plain, failed = _run_case(ident, default_launch=sc.replaying(_lib.call, stats=captured),
                              grid_stats=sc.replaying(mc.launch_grid_stats, stats=captured))
    if failed is not None:
        raise failed
    _launched_as_declared(ident, set(captured))


@gpu
def test_every_ext_entry_point_named_was_launched_by_some_parameter_set():
    """(after the two tests above: it looks at what they saw; a group of which only some parameter sets ran is not judged)"""
    for module, test in EXT_TESTS:
        group = [i for i in EXT_CASES if i.startswith(f"{module[9:]}.{test[5:]}")]
        if group and all(i in _SEEN_EXT for i in group):
            seen = set().union(*(_SEEN_EXT[i] for i in group))
            assert seen == set(EXT_CASES[group[0]][0]), f"{module}::{test} names {EXT_CASES[group[0]][0]}, its parameter sets launched {sorted(seen)}"


# ------------------------------------------------------------------------------------------------------------------------------
def _launching():
    from learning3d_amd import _lib
    protos = {**mc.prototypes(), **_lib.EXT_PROTOTYPES}
    return {n for n, p in protos.items() if mc.has_stream(p)}


def test_every_stream_taking_entry_point_is_in_the_side_stream_test():
    covered = {e for entries, _ in ALL_CASES.values() for e in entries}
    missing = sorted(_launching() - covered)
    assert not missing, f"entry points that take a stream and have no side-stream case: {missing}"
    for ident, (entries, _) in EXT_CASES.items():
        assert entries, f"{ident}: no include/ext entry point found in the test's text"


def test_every_stream_taking_entry_point_replays_or_is_not_captured():
    replayed = {e for ident, (entries, _) in ALL_CASES.items() if ident not in NOT_CAPTURED for e in entries}
    exempt = {e for ident in NOT_CAPTURED for e in ALL_CASES[ident][0]}
    missing = sorted(_launching() - replayed - exempt)
    assert not missing, f"entry points that are neither replayed nor in NOT_CAPTURED: {missing}"


def test_not_captured_names_cases_gives_reasons_and_is_pinned():
    for ident, why in NOT_CAPTURED.items():
        assert ident in ALL_CASES, ident
        assert re.match(r"\S+:\d+, \S", why), f"{ident}: the reason must be `file:line, why`, got {why!r}"
    assert set(NOT_CAPTURED) == PINNED_NOT_CAPTURED, "NOT_CAPTURED changed: read the entry's host code, then pin the new set here"


def test_hooks_are_never_left_set():
    with sc.hooks(default_launch=print, record=[]):
        assert mc.DEFAULT_LAUNCH is print and mc.RECORD == []
    assert mc.DEFAULT_LAUNCH is None and mc.RECORD is None and mc.ACTIVE is None
    with pytest.raises(KeyError):
        with sc.hooks(default_launch=print, record=[], grid_stats=print):
            raise KeyError("x")
    assert mc.DEFAULT_LAUNCH is None and mc.RECORD is None and mc.launch_grid_stats is not print


# ------------------------------------------------------------------------------------------------------------------------------
# the harness must be able to fail: fake entry points in torch, each harmless
def _side_fake(rule):
    """y = 2 x; `rule` names the one mistake it makes"""
    def launch(name, x, n, ws, y):
        if rule == "launches on the default stream":
            with torch.cuda.stream(torch.cuda.default_stream()):
                y.copy_(2 * x)
            return
        if rule == "blocks the host":
            torch.cuda.current_stream().synchronize()
        y.copy_(2 * x)
    return launch


def _side_run(rule):
    x = torch.arange(1.0, 38.0).cuda()
    build = lambda a: (x, 37, a.f32(37), a.f32(37))
    kw = dict(contract=FAKE_CONTRACT, proto=FAKE, sizefn=_fake_size)
    plain, other = [], []
    with sc.hooks(record=plain):
        check("l3d_fake", build, launch=_side_fake(None), **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.default_stream())
    with torch.cuda.stream(side), sc.hooks(record=other):
        out = check("l3d_fake", build, launch=sc.delayed(side, _side_fake(rule), sc.sleep_cycles(), FAKE, FAKE_CONTRACT), **kw)
    torch.cuda.synchronize()
    sc.compare_records(plain, other, "the run on a side stream behind a delay")
    return out["y"], x


@gpu
def test_side_stream_harness_passes_a_correct_launch():
    y, x = _side_run(None)
    assert torch.equal(y, 2 * x)


@gpu
def test_side_stream_harness_names_the_output_of_a_launch_on_the_default_stream():
    with pytest.raises(ContractError, match="`y`.*side stream"):
        _side_run("launches on the default stream")
    torch.cuda.synchronize()


@gpu
def test_side_stream_harness_refuses_an_entry_point_that_blocks_the_host():
    with pytest.raises(AssertionError, match="restored before the entry point returned"):
        _side_run("blocks the host")
    torch.cuda.synchronize()


TICKET = Proto(None, (Param("const float *", "x", "float", 1), Param("void *", "ws", "void", 1), Param("float *", "y", "float", 1),
                      Param("l3d_stream_t", "stream", "l3d_stream_t", 0)))
TICKET_CONTRACT = {"l3d_fake": {"ws": Spec("scratch", "the first 8 bytes zero before the first call (the kernel re-arms them)", keep=8)}}


def _replay_fake(rule):
    """y = x + 2 x[0] + ticket, and the ticket goes up and is re-armed; `rule` names the one mistake it makes"""
    host = {}

    def launch(name, x, ws, y):
        ticket = ws[:8].view(torch.int64)
        if rule == "bakes a device value read before the capture":
            if not torch.cuda.is_current_stream_capturing():
                host["x0"] = float(x[0])                      # a device value read on the host: whatever it was at the last eager call
            torch.add(x, ticket.float() + 2.0 * host["x0"], out=y)
        else:
            torch.add(x, ticket.float() + 2.0 * x[0], out=y)
        ticket += 1
        if rule != "does not re-arm its ticket":
            ticket.zero_()
    return launch


def _replay_run(rule):
    x = torch.arange(1.0, 6.0).cuda()
    build = lambda a: (x, a.bytes(64, zero_first=8, key="ws"), a.f32(5))
    return sc.replayed("l3d_fake", build, real_call=_replay_fake(rule), proto=TICKET, contract=TICKET_CONTRACT)["y"], x


@gpu
def test_replay_harness_passes_a_correct_launch():
    y, x = _replay_run(None)
    assert torch.equal(y, x + 2.0 * x[0])


@gpu
@pytest.mark.parametrize("rule", ["does not re-arm its ticket", "bakes a device value read before the capture"])
def test_replay_harness_fails_at_replay_2(rule):
    with pytest.raises(ContractError, match="`y`.*replay 2"):
        _replay_run(rule)
