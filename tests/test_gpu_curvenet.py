"""CurveNet on the GPU: l3d_curve_walk and l3d_curve_prepare against the reference's fp64 results
(tests/golden/make_golden_curvenet.py), which route a forward takes, that the two routes walk the same curves, and that cached
walk parameters follow in-place edits of the module's state.  Paths are compared on the curves whose fp64 top-2 logit margin
exceeds the fixture's tau; values are held to 4 x the reference's own fp32-to-fp64 gap (test_curvenet_cpu.py)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_curvenet_cpu import (T, by_start, check_net_paths, check_walk, gap_close, run_seeded_net, seeded_grouping,      # noqa: E402
                               seeded_params, walk_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def seeded_net(dev):
    from learning3d_amd.models import CurveNet
    net = seeded_params(CurveNet(num_classes=40, k=20, setting='default'), 6000).eval().to(dev)
    cloud = torch.rand(2, 1024, 3, generator=torch.Generator().manual_seed(5)) * 2 - 1
    return net, (cloud / cloud.norm(dim=2).max(dim=1)[0].view(2, 1, 1)).to(dev)


def logged(fn):
    from learning3d_amd import _lib
    _lib.LAUNCH_LOG = []
    try:
        fn()
        return list(_lib.LAUNCH_LOG)
    finally:
        _lib.LAUNCH_LOG = None


def scaled_inputs(z, grp, dev):
    """the walk's own inputs from the fixture: x sigmoid(att) [B,C,N], idx, and the start points IN THE ORDER the reference's run had
    them (the walk depends on it: make_golden_curvenet.py)"""
    x = T(z["x"]).to(dev)
    return x * torch.sigmoid(grp.att(x)), T(z["idx"]).to(dev), T(z["start_run"]).to(dev)


def keyed(start, path, curves):
    start = start.long().cpu()
    order = torch.argsort(start, dim=1)
    curves = curves.cpu()
    return (torch.gather(start, 1, order), torch.gather(path.long().cpu(), 1, order.unsqueeze(-1).expand(-1, -1, path.shape[2])),
            torch.gather(curves, 2, order.view(order.shape[0], 1, -1, 1).expand_as(curves)))


@pytest.mark.parametrize("si", range(4))
def test_curve_walk_kernel_against_fp64(golden, dev, si):
    from learning3d_amd.utils.curvenet_util import curve_walk
    z, shape = walk_case(golden("curve_walk"), si)
    grp, _ = seeded_grouping(si, shape)
    grp = grp.to(dev)
    with torch.no_grad():
        xs, idx, start = scaled_inputs(z, grp, dev)
        curves, path = curve_walk(xs.transpose(1, 2).contiguous(), idx, start, grp.walk.folded(dev), shape[5])
    torch.cuda.synchronize()
    assert path.dtype == torch.int32 and tuple(path.shape) == (shape[0], shape[4], shape[5])
    check_walk(z, *keyed(start, path, curves), what=f"l3d_curve_walk {shape}")


@pytest.mark.parametrize("B,C,N", [(2, 16, 128), (3, 32, 1000), (1, 128, 72), (2, 48, 65)])
def test_curve_prepare_against_torch(dev, B, C, N):
    """att = sigmoid(w . x) and x att in channel-last layout, against fp64 torch.  Bars from the arithmetic: the C-term fp32 sum is
    within (C + 1) eps sum|w x| of the exact one, sigmoid's slope is at most 1/4 and its own evaluation (exp, add, divide) within
    4 eps; the product adds one rounding."""
    from learning3d_amd.utils.curvenet_util import curve_prepare
    g = torch.Generator().manual_seed(B * 1000 + C + N)
    x, w = torch.randn(B, C, N, generator=g), torch.randn(C, generator=g) * 0.3
    xa, att = curve_prepare(x.to(dev), w.to(dev))
    x64, w64 = x.double(), w.double()
    s = torch.einsum("c,bcn->bn", w64, x64)
    eps = 2.0 ** -24
    att_bar = 0.25 * (C + 1) * eps * torch.einsum("c,bcn->bn", w64.abs(), x64.abs()) + 4 * eps
    att_err = (att.cpu().double() - torch.sigmoid(s)).abs()
    want = (x64 * torch.sigmoid(s).unsqueeze(1)).transpose(1, 2)
    xa_err = (xa.cpu().double() - want).abs()
    xa_bar = x64.abs().transpose(1, 2) * att_bar.unsqueeze(-1) + eps * want.abs()
    print(f"prepare [{B},{C},{N}]: att error / bar {float((att_err / att_bar).max()):.3f}, x att error / bar {float((xa_err / (xa_bar + 1e-30)).max()):.3f}")
    assert tuple(xa.shape) == (B, N, C) and bool((att_err <= att_bar).all()) and bool((xa_err <= xa_bar).all())


def test_route_choice(seeded_net):
    net, cloud = seeded_net
    with torch.no_grad():
        log = logged(lambda: net(cloud))
    assert log.count("l3d_curve_walk") == 4 and log.count("l3d_curve_prepare") == 4
    net.cic11.conv1[0].weight.requires_grad_(True)
    with torch.enable_grad():
        log = logged(lambda: net(cloud))
    assert log.count("l3d_curve_walk") == 0 and log.count("l3d_curve_prepare") == 0
    net.train()
    try:
        with torch.no_grad():
            state = copy.deepcopy(net.state_dict())
            log = logged(lambda: net(cloud))
            net.load_state_dict(state)                   # the train-mode pass moved the running statistics
        assert log.count("l3d_curve_walk") == 0
    finally:
        net.eval()


@pytest.mark.parametrize("si", range(4))
def test_two_routes_walk_the_same_curves(golden, dev, si):
    """Walk.forward on the same start list through both routes: the same paths on the curves above tau, and both the reference's"""
    from learning3d_amd.utils import curvenet_util as cu
    z, shape = walk_case(golden("curve_walk"), si)
    grp, _ = seeded_grouping(si, shape)
    grp = grp.to(dev)
    walk = grp.walk
    with torch.no_grad():
        xs, idx, start = scaled_inputs(z, grp, dev)
        xyz = T(z["xyz"]).to(dev)
        log = logged(lambda: walk(xyz, xs, idx, start.unsqueeze(2)))
        assert log == ["l3d_curve_walk"]
        fused = by_start(walk, walk(xyz, xs, idx, start.unsqueeze(2)))
        cu.FUSED_WALK = False
        try:
            log = logged(lambda: walk(xyz, xs, idx, start.unsqueeze(2)))
            ops = by_start(walk, walk(xyz, xs, idx, start.unsqueeze(2)))
        finally:
            cu.FUSED_WALK = True
        assert "l3d_curve_walk" not in log
        log = logged(lambda: grp(T(z["x"]).to(dev), xyz, idx))          # CurveGrouping itself: prepare, topk, one walk
        assert log == ["l3d_curve_prepare", "l3d_curve_walk"]
    keep = z["margin"] > float(z["tau"])
    assert torch.equal(fused[0], ops[0])
    assert np.array_equal(fused[1].numpy()[keep], ops[1].numpy()[keep])
    check_walk(z, *fused, what=f"fused Walk {shape}")
    check_walk(z, *ops, what=f"op-sequence Walk on the device {shape}")


def test_seeded_curvenet_both_routes_against_fp64(golden, dev):
    """The whole classifier at B 2, N 1024 through both routes, every walk started from the fixture's lists: paths equal the fp64
    ones on every curve above tau on both routes; where a route walks the fp64 paths on ALL curves its 40 logits are within the gap
    bar of the fp64 logits with the same arg-max class; where the two routes walk the same paths their logits are within the same
    bar of each other.  (A curve at or below tau that flips changes the logits by an amount no rounding bound covers.)"""
    z = golden("curvenet_seeded")
    fused, fblocks, own = run_seeded_net(z, dev, fused=True)
    ops, oblocks, _ = run_seeded_net(z, dev, fused=False)
    for i in range(4):
        print(f"walk {i}: own start selection differs from the stored one in {int((own[i].numpy() != z[f'w{i}.start']).sum())} places")
    f_all, o_all = check_net_paths(z, fblocks, "fused"), check_net_paths(z, oblocks, "op-sequence")
    gap = np.abs(z["f32.logits"].astype(np.float64) - z["f64.logits"]).max()
    routes_same = all(torch.equal(a[1], b[1]) for a, b in zip(fblocks, oblocks))
    between = float((fused.double() - ops.double()).abs().max())
    print(f"fused on fp64 paths: {f_all}, op-sequence on fp64 paths: {o_all}, routes on the same paths: {routes_same}; "
          f"fused vs op-sequence logits {between:.3e}, reference fp32 vs fp64 {gap:.3e}")
    assert f_all and o_all and routes_same, "a curve at or below tau left the fp64 path: the logits are not comparable"
    gap_close(fused.numpy(), z, "logits", "fused 40 logits")
    gap_close(ops.numpy(), z, "logits", "op-sequence 40 logits")
    assert between <= 4.0 * gap
    assert np.array_equal(fused.numpy().argmax(1), z["f64.logits"].argmax(1)) and np.array_equal(ops.numpy().argmax(1), z["f64.logits"].argmax(1))


def test_shape_past_the_lds_limit_takes_the_op_sequence(dev):
    """C 128 with 64 curves needs 64 x 259 words of LDS, past l3d_curve_walk's 16384: -2 from the entry point, and Walk / CurveGrouping
    take the op-sequence route instead of raising; 63 curves fit and run fused"""
    from learning3d_amd.utils.curvenet_util import CurveGrouping
    g = torch.Generator().manual_seed(12)
    x, xyz = torch.randn(1, 128, 64, generator=g).to(dev), torch.rand(1, 3, 64, generator=g).to(dev)
    idx = torch.stack([torch.randperm(64, generator=g)[:8] for _ in range(64)]).unsqueeze(0).to(dev)
    with torch.no_grad():
        for cn, fused in ((64, False), (63, True)):
            grp = seeded_params(CurveGrouping(128, 8, cn, 3), 77).eval().to(dev)
            log = logged(lambda: grp(x, xyz, idx))
            assert ("l3d_curve_walk" in log) == fused and tuple(grp.walk.last_path.shape) == (1, cn, 3)


def test_forward_is_captured_in_a_graph(golden, dev):
    """no host read on the fused route: CurveGrouping's forward records into a graph and replays with the same picks"""
    z, shape = walk_case(golden("curve_walk"), 0)
    grp, _ = seeded_grouping(0, shape)
    grp = grp.to(dev)
    args = [T(z[k]).to(dev) for k in ("x", "xyz", "idx")]
    with torch.no_grad():
        want = grp(*args).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            grp(*args)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = grp(*args)
        out.zero_()
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


@pytest.mark.parametrize("what", ["agent_mlp.0.weight", "agent_mlp.1.running_mean"])
def test_cached_walk_parameters_follow_in_place_edits(golden, dev, what):
    """after an in-place edit the next fused forward equals, bit for bit, the fused forward of a fresh copy of the edited module
    (which has no cache), differs from the forward before the edit, and follows the op-sequence route.  "Exactly as the op-sequence
    route" cannot be asked of discrete picks with unknown margins (the fixture's margins belong to the unedited weights): at least
    95 % of the curves must walk the same path on both routes, the share the fixtures allow below tau, and on those curves the
    features agree to 2^-22 relative (the op-sequence route multiplies each row by (1 - y) + y, one ulp from 1)."""
    from learning3d_amd.utils import curvenet_util as cu
    z, shape = walk_case(golden("curve_walk"), 0)
    grp, _ = seeded_grouping(0, shape)
    grp = grp.to(dev)
    walk = grp.walk
    with torch.no_grad():
        xs, idx, start = scaled_inputs(z, grp, dev)
        args = (T(z["xyz"]).to(dev), xs, idx, start.unsqueeze(2))
        before = walk(*args).clone()
        if what == "agent_mlp.0.weight":
            t = walk.agent_mlp[0].weight
            t.add_(torch.randn(t.shape, generator=torch.Generator().manual_seed(9)).to(dev) * 0.2)
        else:
            walk.agent_mlp[1].running_mean.add_(0.7)
        after = walk(*args).clone()
        path_after = walk.last_path.long().cpu()
        fresh = copy.deepcopy(walk)
        fresh.__dict__.pop("_l3d_walk", None)
        want = fresh(*args)
        cu.FUSED_WALK = False
        try:
            feat_ops = walk(*args).cpu()
            path_ops = walk.last_path.long().cpu()
        finally:
            cu.FUSED_WALK = True
    assert torch.equal(after, want) and not torch.equal(after, before)
    agree = float((path_after == path_ops).all(dim=2).float().mean())
    print(f"{what}: curves on which the two routes agree after the edit {agree:.3f}")
    assert agree >= 0.95
    on = (path_after == path_ops).all(dim=2)                                     # B, curve_num
    on = on.view(on.shape[0], 1, on.shape[1], 1).expand_as(feat_ops)
    a, o = after.cpu()[on], feat_ops[on]
    assert bool(((a - o).abs() <= 2.0 ** -22 * o.abs()).all())
