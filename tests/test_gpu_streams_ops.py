"""The public ops, the backward functions and the models the way they are used: on a side stream, with the process-wide caches cold
and two streams arriving at once, with the Chamfer workspaces growing and shrinking on one stream, and captured into a graph on one
stream and replayed on new inputs.  Every result is held, bit for bit, to the plain call on the default stream (the Chamfer life
cycle: to the three-step route, at the bars of tests/test_gpu_parity.py).

Driven from the tables of tests/test_gpu_views_ops.py, test_gpu_views_backward.py and test_gpu_views_models.py at their own shapes.
Not marked gpu: the keying of the attention workspace, what a cache hit costs on its own stream, the pinned MODELS_NOT_CAPTURED."""
import os
import re
import sys

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import layout_audit                                                                     # noqa: E402
import stream_cases as sc                                                               # noqa: E402
import test_gpu_views_backward as view_bwd                                              # noqa: E402
import test_gpu_views_models as view_models                                             # noqa: E402
import test_gpu_views_ops as view_ops                                                   # noqa: E402
from seeded import seeded_params                                                        # noqa: E402
from view_cases import assert_identical, has_entry, leaves, logged                      # noqa: E402

gpu = pytest.mark.gpu
SHORT_MS = 0.05             # the delay in front of every C-ABI call of a whole op or model on the side stream
LONG_MS = 20.0              # the delay a cold cache is filled behind


def _sleeping(real_call, cycles, only=None):
    """an `inner` for layout_audit.install: a busy-wait on the current stream (on the stream `only`, if given) before every C-ABI call"""
    def call(name, *args, **kw):
        if only is None or torch.cuda.current_stream() == only:
            torch.cuda._sleep(cycles)
        return real_call(name, *args, **kw)
    return call


def _on_side(monkeypatch, fn, args):
    """fn(*args) on a side stream that is behind the host by a delay per C-ABI call"""
    from learning3d_amd import _lib
    side = torch.cuda.Stream()
    with monkeypatch.context() as m:
        layout_audit.install(m, inner=_sleeping(_lib.call, sc.sleep_cycles(SHORT_MS)))
        side.wait_stream(torch.cuda.default_stream())
        with torch.cuda.stream(side):
            out = fn(*args)
        torch.cuda.synchronize()
    return out


def _backward_case(name):
    """a case of test_gpu_views_backward as fn() -> (outputs, gradients of every input) for seeded contiguous output gradients"""
    build = view_bwd.CASES[name][0]

    def fn():
        leaf = view_bwd.Leaves()
        outs = build(leaf)
        outs = tuple(outs) if isinstance(outs, (tuple, list)) else (outs,)
        gen = torch.Generator().manual_seed(60)
        grads = [torch.randn(o.shape, generator=gen).to(o.device) for o in outs]
        return [o.detach() for o in outs], view_bwd.backward(outs, leaf.inputs, grads)
    return fn


@gpu
@pytest.mark.parametrize("name", sorted(view_ops.CASES))
def test_public_op_on_a_side_stream(name, monkeypatch):
    spec = view_ops.CASES[name]()
    fn, args = spec[0], spec[1]
    fn(*args)                                           # (the first call fills the caches of weight images)
    want = fn(*args)
    torch.cuda.synchronize()
    got = _on_side(monkeypatch, fn, args)
    (view_ops.images_identical if name in view_ops.IMAGES else assert_identical)(got, want, f"{name}: on a side stream against the default stream")


@gpu
@pytest.mark.parametrize("name", sorted(view_bwd.CASES))
def test_backward_on_a_side_stream(name, monkeypatch):
    fn = _backward_case(name)
    fn()
    want = fn()
    torch.cuda.synchronize()
    assert any(g is not None for g in want[1])
    got = _on_side(monkeypatch, fn, ())
    assert_identical(got, want, f"{name}: forward and backward on a side stream against the default stream")


def _model_case(name, seed_shift=0):
    net, call, count, n, shape, *batch = view_models.MODELS[name]()
    base = view_models.clouds(n, sum(map(ord, name)) + seed_shift, count, *batch)
    return net, call, [b if shape == "bnc" else b.transpose(1, 2).contiguous() for b in base]


@gpu
@pytest.mark.parametrize("name", sorted(view_models.MODELS))
def test_model_on_a_side_stream(name, monkeypatch):
    net, call, args = _model_case(name)
    with torch.no_grad():
        call(net, *args)                                # (the first call fills the caches of weight images)
        want = call(net, *args)
        torch.cuda.synchronize()
        got = _on_side(monkeypatch, lambda *xs: call(net, *xs), args)
    assert_identical(got, want, f"{name}: on a side stream against the default stream", strides=False)


# ------------------------------------------------------------------------------------------------------------------------------
# cold caches, two streams at once
def _drop_process_caches():
    from learning3d_amd.models import _fused, _rows
    from learning3d_amd.utils import transformer
    for cache in (_fused._OBS_CACHE, _rows._A_IMG, _rows._ONES, transformer._ATT_WS):
        cache.clear()


def _rows_linear_f16():
    """view_ops' rows_linear at the smallest rows the f16x2 route of _rows.linear takes (4096): below them the op is one
    l3d_bmm_f32 and goes through no cache; from there on the rows' image is kept in _rows._A_IMG"""
    from learning3d_amd.models import _rows
    lin = seeded_params(nn.Linear(32, 256), 102).cuda()
    return view_ops.nograd(lambda x: _rows.linear(x, lin, relu=True)), [view_ops.rnd(2, 2048, 32, seed=102)], "l3d_split_f16_operand"


def _rows_square_distance_backward():
    """_rows.square_distance's backward multiplies by _rows._ones"""
    return _backward_case("square_distance"), [], "l3d_bmm_f32"


def _cold_model(name):
    def make():
        net, call, args = _model_case(name)
        return view_ops.nograd(lambda *xs: call(net, *xs)), args, view_models.FUSED[name]
    return make


COLD = {"dgcnn": _cold_model("dgcnn"), "pcn": _cold_model("pcn"), "dcp": _cold_model("dcp"), "rows_linear": _rows_linear_f16,
        "rows_square_distance_backward": _rows_square_distance_backward}


@gpu
@pytest.mark.parametrize("name", sorted(COLD))
def test_cold_caches_filled_on_one_stream_and_hit_from_another(name, monkeypatch):
    """The images are ENQUEUED on the side stream behind a long delay; the default stream arrives at once, hits the caches and must
    wait for them.  RANGE_POLICY "async": the default policy ends every model forward with a wait for its own stream."""
    from learning3d_amd import _lib
    from learning3d_amd.models import _fused
    fn, args, entry = COLD[name]()
    fn(*args)
    want, log = logged(fn, *args)
    assert has_entry(log, entry), (entry, log)
    monkeypatch.setattr(_fused, "RANGE_POLICY", "async")
    fn, args, _ = COLD[name]()                          # a fresh module of the same seeded weights: nothing cached on it
    _drop_process_caches()
    side = torch.cuda.Stream()
    with monkeypatch.context() as m:
        layout_audit.install(m, inner=_sleeping(_lib.call, sc.sleep_cycles(4 * SHORT_MS), only=side))
        side.wait_stream(torch.cuda.default_stream())
        with torch.cuda.stream(side):
            torch.cuda._sleep(sc.sleep_cycles(LONG_MS))
            first = fn(*args)
        second = fn(*args)                              # at once: nothing has been waited for
        torch.cuda.synchronize()
    _fused.check_range(sync=True)
    assert_identical(second, want, f"{name}: the default stream, hitting caches another stream had enqueued", strides=False)
    assert_identical(first, want, f"{name}: the side stream, filling the caches", strides=False)


# ------------------------------------------------------------------------------------------------------------------------------
# the Chamfer workspaces on one stream: small, large (a re-allocation), small again on the large one
LIFE = [(2, 77, 130), (8, 1024, 1030), (2, 77, 130)]


@gpu
def test_chamfer_workspaces_small_large_small_on_one_stream():
    """bars: tests/test_gpu_parity.py::test_chamfer_forward_loss_one_launch_equals_search_plus_tail and
    ::test_chamfer_loss_local_equals_partials_plus_combine -- distances and indices bit for bit; the two fp64 sums are the same terms
    added in another order (relative 1e-13); the loss is one rounding of them to fp32 (relative 1.2e-7)"""
    import importlib
    cd = importlib.import_module("learning3d_amd.losses.chamfer_distance")
    from learning3d_amd._lib import call
    side = torch.cuda.Stream()                           # its workspaces are dropped below: both start from nothing
    side.wait_stream(torch.cuda.default_stream())
    sizes = []
    with torch.cuda.stream(side), torch.no_grad():
        key = (torch.cuda.current_device(), side.cuda_stream)
        cd._FL_WS.pop(key, None)                         # (torch hands out its streams from a pool: an earlier test may have had this one)
        cd._LL_WS.pop(key, None)
        for step, (B, N, M) in enumerate(LIFE):
            a, b = view_ops.rnd(B, N, 3, seed=200 + step), view_ops.rnd(B, M, 3, seed=210 + step)
            d1, d2 = torch.empty(B, N, device="cuda"), torch.empty(B, M, device="cuda")
            i1, i2 = torch.empty(B, N, dtype=torch.int32, device="cuda"), torch.empty(B, M, dtype=torch.int32, device="cuda")
            call("l3d_chamfer_forward", a, b, B, N, M, d1, d2, i1, i2)
            part_ref = cd.chamfer_partials(d1, d2)
            loss_ref = cd.chamfer_combine(part_ref)
            loss, part, e1, e2, j1, j2 = cd.chamfer_forward_loss(a, b, want="all")
            local = cd.chamfer_loss_local(d1, d2)
            sizes.append(cd._FL_WS[key][0].numel())
            what = f"step {step}, B={B} N={N} M={M}"
            assert torch.equal(e1, d1) and torch.equal(e2, d2) and torch.equal(j1, i1) and torch.equal(j2, i2), what
            pr, pg = part_ref.cpu(), part.cpu()
            assert pg[2] == B * N and pg[3] == B * M, what
            assert bool(((pg[:2] - pr[:2]).abs() <= 1e-13 * pr[:2].abs()).all()), (what, pg, pr)
            bar = 1.2e-7 * max(1.0, abs(float(loss_ref)))
            print(f"{what}: |forward_loss - three steps| = {abs(float(loss) - float(loss_ref)):g}, |loss_local - three steps| = "
                  f"{abs(float(local) - float(loss_ref)):g} (bar {bar:g})")
            assert abs(float(loss) - float(loss_ref)) <= bar, what
            assert abs(float(local) - float(loss_ref)) <= bar, what
    assert sizes[1] > sizes[0] and sizes[2] == sizes[1], f"the large shape did not force a re-allocation: {sizes}"


# ------------------------------------------------------------------------------------------------------------------------------
# replay of the models that have no graph test of their own
OWN_GRAPH_TEST = {"pointnetlk": "tests/test_gpu_registration.py::test_pointnetlk_loop_in_one_graph",
                  "ipcrnet": "tests/test_gpu_registration.py (the iteration loop is the captured unit there)",
                  "curvenet": "tests/test_gpu_curvenet.py"}
# a model whose forward reads a device value on the host: name -> "file:line, why" (from reading learning3d_amd/models and utils for
# .item(), .cpu(), .tolist(), torch.randint(, bool( and int(; FlowNet3D samples through pointnet2_utils.furthest_point_sample, which
# starts from point 0, and no model here calls model_common_utils.farthest_point_sample without start_with_first_point)
MODELS_NOT_CAPTURED = {
    "masknet2_pair": "learning3d_amd/models/masknet.py:48, mask > threshold: the number of selected points is read on the host and shapes the result",
}
PINNED_MODELS_NOT_CAPTURED = frozenset({"masknet2_pair"})
REPLAYED = sorted(set(view_models.MODELS) - set(OWN_GRAPH_TEST) - set(MODELS_NOT_CAPTURED))


def _snapshot(out):
    return [t.clone() for _, t in leaves(out)]


@gpu
@pytest.mark.parametrize("name", REPLAYED)
def test_model_replays_on_new_clouds(name):
    from learning3d_amd.models import _fused
    net, call, args = _model_case(name)
    others = [_model_case(name, shift)[2] for shift in (1, 2)]
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call(net, *args)                             # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        static = [a.clone() for a in args]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = call(net, *static)
        for i, values in enumerate(others):
            for s, v in zip(static, values):
                s.copy_(v)                               # in place: the graph reads the addresses it was captured with
            graph.replay()
            torch.cuda.synchronize()
            got = _snapshot(out)
            want = _snapshot(call(net, *[v.clone() for v in values]))
            assert_identical(got, want, f"{name}: replay {i + 1} on new clouds against an eager call on them", strides=False)
    _fused.check_range(sync=True)


# ------------------------------------------------------------------------------------------------------------------------------
# host level
def test_replayed_models_and_the_exempt_sets_are_pinned():
    assert set(MODELS_NOT_CAPTURED) == PINNED_MODELS_NOT_CAPTURED, "MODELS_NOT_CAPTURED changed: read the model's forward, then pin the new set"
    for name, why in {**MODELS_NOT_CAPTURED, **OWN_GRAPH_TEST}.items():
        assert name in view_models.MODELS, name
    for name, why in MODELS_NOT_CAPTURED.items():
        m = re.match(r"(\S+):(\d+), \S", why)
        assert m, f"{name}: the reason must be `file:line, why`, got {why!r}"
        with open(os.path.join(ROOT, m[1])) as f:
            line = f.read().split("\n")[int(m[2]) - 1]
        assert re.search(r"\.item\(\)|\.cpu\(\)|\.tolist\(\)|torch\.randint\(|bool\(|int\(", line), f"{name}: {m[1]}:{m[2]} reads nothing on the host: {line!r}"
    assert REPLAYED == ["classifier", "dcp", "dgcnn", "flownet3d", "masknet", "masknet2_masks", "pcn", "pointnet_bcn", "pointnet_bcn_bn",
                        "pointnet_bnc", "pointnet_bnc_bn", "segmentation"]


def test_attention_workspace_is_keyed_by_device_and_stream():
    from learning3d_amd.utils import transformer
    saved = dict(transformer._ATT_WS)
    try:
        a = transformer._attention_workspace("cpu", stream=11)
        b = transformer._attention_workspace("cpu", stream=12)
        assert a.data_ptr() != b.data_ptr(), "two streams share one maxima buffer"
        assert transformer._attention_workspace("cpu", stream=11) is a and transformer._attention_workspace("cpu", stream=12) is b
        assert a.numel() * a.element_size() == 16
    finally:
        transformer._ATT_WS.clear()
        transformer._ATT_WS.update(saved)


def test_cache_hit_on_its_own_stream_is_one_comparison(monkeypatch):
    """_lib.order_after_build with the stream query and the stream object replaced by counters: the same stream -> nothing is
    touched; another stream -> one wait on the entry's event; another stream while capturing -> none"""
    from learning3d_amd import _lib
    waits, current = [], [5]

    class Stream:
        def wait_event(self, event):
            waits.append(event)
    monkeypatch.setattr(torch._C, "_cuda_getCurrentRawStream", lambda index: current[0], raising=False)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda index=None: Stream())
    capturing = [False]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: capturing[0])
    mark = (0, 5, "the event")
    _lib.order_after_build(None)
    _lib.order_after_build(mark)
    assert waits == []
    current[0] = 6
    _lib.order_after_build(mark)
    assert waits == ["the event"]
    capturing[0] = True
    _lib.order_after_build(mark)
    _lib.order_after_build((0, 5, None))
    assert waits == ["the event"]
    assert _lib.built_on(None) is None and _lib.built_on(torch.zeros(1)) is None


def test_build_mark_survives_deepcopy_and_pickle(monkeypatch):
    """cache entries live in module __dict__s: copy.deepcopy(model) and pickle walk them, and an event can be neither copied nor
    pickled.  Without a device the copy knows of no build (it orders nothing); so does an unpickled one."""
    import copy
    import pickle
    from learning3d_amd import _lib
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    mark = _lib._Built((0, 5, torch.cuda.Event() if hasattr(torch.cuda, "Event") else object()))
    entry = (("key",), torch.zeros(3), [torch.zeros(2)], mark)
    for other in (copy.deepcopy(entry), pickle.loads(pickle.dumps(entry))):
        assert tuple(other[3]) == (0, None, None) and torch.equal(other[1], entry[1])
        _lib.order_after_build(None if other[3][1] is None else other[3])


@gpu
def test_deepcopy_of_a_model_with_filled_caches_is_ordered_and_equal():
    import copy
    net, call, args = _model_case("dgcnn")
    with torch.no_grad():
        want = call(net, *args)
        twin = copy.deepcopy(net)
        got = call(twin, *args)
    torch.cuda.synchronize()
    assert_identical(got, want, "a deep copy of a model whose caches are filled", strides=False)


@gpu
def test_dgcnn_forward_and_chamfer_loss_issue_the_pinned_calls(monkeypatch):
    """the benchmark step's front: the stream-aware caches add no C-ABI call, and a warm forward on one stream records and waits for
    no event"""
    import importlib
    cd = importlib.import_module("learning3d_amd.losses.chamfer_distance")
    net, call, args = _model_case("dgcnn")
    a, b = view_ops.rnd(2, 128, 3, seed=48), view_ops.rnd(2, 96, 3, seed=49)

    def step(x):
        return call(net, x), cd.chamfer_forward_loss(a, b)
    from learning3d_amd import _lib
    from learning3d_amd.models import _fused, _rows
    events = []
    with torch.no_grad():
        step(*args)
        monkeypatch.setattr(torch.cuda.Stream, "wait_event", lambda self, e: events.append("wait"))
        for mod in (_fused, _rows):
            monkeypatch.setattr(mod, "built_on", lambda t: events.append("build") or _lib.built_on(t))
        _, log = logged(step, *args)
    assert events == [], events
    print("the step's C-ABI calls:", log)
    assert log == DGCNN_STEP_CALLS, log


# read off the parent commit's log at these shapes (LABLOG R30.1)
DGCNN_STEP_CALLS = ["l3d_knn_graph", "l3d_edgeconv_forward_f16b", "l3d_pointwise_conv", "l3d_chamfer_forward_loss"]
