"""PPFNet's differentiable HIP route without a GPU: the header include/ext/l3d_rpmnet_train.h in the open table, the statuses its
entry points return before any launch, the backward formulas the kernels implement (golden/rpmnet_train_fixture.py) against
torch.autograd through GroupNorm -> ReLU (-> max over K) in fp64, and the fallback: on CPU tensors the route is not taken and the
gradients are the op sequence's bit for bit."""
import copy
import ctypes
import os
import sys

import pytest
import torch

from learning3d_amd import _lib
from learning3d_amd.models import PPFNet, _fused, ppfnet

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import rpmnet_train_fixture as tf      # noqa: E402

NEW = ("l3d_gn_mean_rstd", "l3d_gn_pool_winner", "l3d_gn_relu", "l3d_gn_backward_workspace_bytes", "l3d_gn_backward_stats",
       "l3d_gn_backward_reduce", "l3d_gn_backward_apply")


def test_the_header_parses_into_the_open_table():
    for name in NEW:
        assert name in _lib.EXT_SIGNATURES and name in _lib.EXT_PROTOTYPES
        assert name not in _lib.SIGNATURES and name not in _lib.MODEL_SIGNATURES
    P = _lib.EXT_PROTOTYPES
    names = lambda n: [p.name for p in P[n].params]           # noqa: E731
    elements = lambda n: {p.name: p.element for p in P[n].params if p.indirection}       # noqa: E731
    assert names("l3d_gn_backward_stats") == ["du", "widx", "K", "y", "in_a", "in_s", "stat", "B", "C", "groups", "P", "part", "workspace",
                                              "stream"]
    assert names("l3d_gn_backward_apply") == ["du", "widx", "K", "y", "in_a", "in_s", "stat", "gamma", "m", "B", "C", "groups", "P", "dz",
                                              "stream"]
    assert names("l3d_gn_backward_reduce") == ["part", "gamma", "B", "C", "groups", "count", "m", "dgamma", "dbeta", "stream"]
    assert elements("l3d_gn_backward_stats") == {"du": "float", "widx": "unsigned char", "y": "float", "in_a": "float", "in_s": "float",
                                                 "stat": "double", "part": "double", "workspace": "void"}
    assert elements("l3d_gn_backward_apply")["m"] == "double" and elements("l3d_gn_backward_apply")["dz"] == "float"
    assert elements("l3d_gn_pool_winner") == {"y": "float", "in_a": "float", "widx": "unsigned char"}
    assert elements("l3d_gn_mean_rstd") == {"moments": "double", "stat": "double"}
    assert P["l3d_gn_backward_workspace_bytes"].restype is ctypes.c_size_t
    assert [p.element for p in P["l3d_gn_backward_workspace_bytes"].params] == ["int", "int", "int"]
    assert P["l3d_gn_backward_stats"].restype is ctypes.c_int
    assert _lib.L3D_GN_BWD_CHUNK == 8192 and "L3D_GN_BWD_CHUNK" in _lib.EXT_CONSTANTS
    for name in ("l3d_gn_backward_stats", "l3d_gn_backward_apply", "l3d_gn_pool_winner"):       # const inputs, one writable output each
        writable = [p.name for p in P[name].params if p.indirection and not p.ctype.startswith("const")]
        assert writable == {"l3d_gn_backward_stats": ["part", "workspace"], "l3d_gn_backward_apply": ["dz"],
                            "l3d_gn_pool_winner": ["widx"]}[name]


def test_null_and_unsupported_statuses_before_any_launch():
    h = _lib.lib()
    one = ctypes.c_void_p(16)                      # never dereferenced: every call below returns before a launch
    eps = ctypes.c_float(1e-5)
    assert h.l3d_gn_mean_rstd(None, 1, 16, 8, 4, eps, one, None) == -1
    assert h.l3d_gn_mean_rstd(one, 1, 12, 8, 4, eps, one, None) == -2
    assert h.l3d_gn_pool_winner(one, one, 1, 16, 0, 4, one, None) == -1
    assert h.l3d_gn_pool_winner(one, one, 1, 16, 65, 4, one, None) == -2
    assert h.l3d_gn_relu(one, one, None, 1, 16, 4, one, None) == -1
    assert h.l3d_gn_relu(one, one, one, 70000, 16, 4, one, None) == -2
    assert h.l3d_gn_backward_stats(one, None, 0, one, one, one, one, 1, 16, 8, 4, one, None, None) == -1        # no workspace
    assert h.l3d_gn_backward_stats(one, None, 2, one, one, one, one, 1, 16, 8, 4, one, one, None) == -1         # K without widx
    assert h.l3d_gn_backward_stats(one, one, 0, one, one, one, one, 1, 16, 8, 4, one, one, None) == -1          # widx without K
    assert h.l3d_gn_backward_stats(one, one, 3, one, one, one, one, 1, 16, 8, 4, one, one, None) == -1          # P % K
    assert h.l3d_gn_backward_stats(one, one, 65, one, one, one, one, 1, 16, 8, 130, one, one, None) == -2
    assert h.l3d_gn_backward_stats(one, None, 0, one, one, one, one, 1, 12, 8, 4, one, one, None) == -2         # C % groups
    assert h.l3d_gn_backward_reduce(one, None, 1, 16, 8, 4, one, None, None, None) == -1
    assert h.l3d_gn_backward_reduce(one, one, 1, 12, 8, 4, one, None, None, None) == -2
    assert h.l3d_gn_backward_apply(one, None, 0, one, one, one, one, one, one, 1, 16, 8, 4, None, None) == -1
    assert h.l3d_gn_backward_apply(one, one, 3, one, one, one, one, one, one, 1, 16, 8, 4, one, None) == -1
    assert h.l3d_gn_backward_apply(one, None, 0, one, one, one, one, one, one, 70000, 16, 8, 4, one, None) == -2
    assert h.l3d_gn_backward_workspace_bytes(2, 96, 8192) == 2 * 96 * 16 and h.l3d_gn_backward_workspace_bytes(2, 96, 8193) == 2 * 96 * 2 * 16
    assert h.l3d_gn_backward_workspace_bytes(2, 0, 10) == 0
    big = _lib.L3D_GN_BWD_MAX_P + 1                # a row the kernels' int indices do not reach
    assert _lib.L3D_GN_BWD_MAX_P == 2 ** 31 - 1 - _lib.L3D_GN_BWD_CHUNK
    assert h.l3d_gn_backward_stats(one, None, 0, one, one, one, one, 1, 16, 8, big, one, one, None) == -2
    assert h.l3d_gn_backward_apply(one, None, 0, one, one, one, one, one, one, 1, 16, 8, big, one, None) == -2
    assert h.l3d_gn_relu(one, one, one, 1, 16, big, one, None) == -2
    assert h.l3d_gn_pool_winner(one, one, 1, 16, 2, big // 2 + 1, one, None) == -2


@pytest.mark.parametrize("B,C,P,K", [(2, 16, 150, 0), (2, 48, 63, 0), (1, 16, 1, 0), (2, 16, 210, 3), (2, 48, 70, 1), (1, 16, 320, 64)])
def test_backward_formulas_are_autograd_through_group_norm_relu_max(B, C, P, K):
    """S1, S2 per (cloud, channel), M1, M2 per (cloud, group), dy = rstd (gamma g - M1 - zhat M2), dgamma = sum_b S2, dbeta = sum_b S1
    against torch.autograd in fp64, at rounding level; gamma = 0 in channel 1 and < 0 in channel 2"""
    y, gamma, beta, du = tf.layer_case(40 + P + K, B, C, P, K)
    assert float(gamma[1]) == 0.0 and float(gamma[2]) < 0.0
    mean, rstd = tf.group_stats64(y, tf.GROUPS)
    a, s = tf.affine64(gamma, beta, mean, rstd, tf.GROUPS)
    widx = tf.winners64(y.double(), a, K) if K else None
    dz, dgamma, dbeta, _, _ = tf.gn_relu_backward64(du, y, a, s, mean, rstd, gamma, tf.GROUPS, K, widx)
    want_dz, want_dgamma, want_dbeta, arg = tf.gn_relu_autograd64(du, y, gamma, beta, tf.GROUPS, K, widx)
    for got, want in ((dz, want_dz), (dgamma, want_dgamma), (dbeta, want_dbeta)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    if K > 1:
        # where the pooled activation is alive (and so unique over k) the forward's rule picks torch.max's winner, for either sign
        u = torch.relu(a[:, :, None] * y.double() + s[:, :, None]).view(B, C, K, P // K).amax(2)
        alive = u > 0
        assert bool(alive[:, 2].any()) and torch.equal(widx[alive], arg[alive])


def _tiny():
    net = tf.ppfnet_case(3, 16, 4, 24)[0]
    xyz, nrm = tf.clouds(4, 2, 24)
    return net, xyz, nrm


def _grads(net, xyz, nrm):
    net.zero_grad(set_to_none=True)
    out = net(xyz, nrm)
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(9))
    (out * w).sum().backward()
    return out.detach(), [p.grad.clone() for p in net.parameters()]


def test_cpu_tensors_take_the_op_sequence_bit_for_bit():
    net, xyz, nrm = _tiny()
    assert net._kernels_take() and not net.trains_on_hip(xyz, nrm)
    assert len(net._parameters_in_order()) == 22 and {id(p) for p in net._parameters_in_order()} == {id(p) for p in net.parameters()}
    _lib.LAUNCH_LOG = log = []
    try:
        out_on, g_on = _grads(net, xyz, nrm)
        _fused.TRAIN_HIP = False
        out_off, g_off = _grads(net, xyz, nrm)
    finally:
        _fused.TRAIN_HIP = True
        _lib.LAUNCH_LOG = None
    assert log == []
    assert torch.equal(out_on, out_off) and all(torch.equal(a, b) for a, b in zip(g_on, g_off))
    # the op sequence spelled here: the module stacks on the grouped features
    net.zero_grad(set_to_none=True)
    raw = ppfnet._sample_and_group_multi(net.radius, net.n_sample, xyz, nrm)
    x = torch.cat([raw["xyz"][:, :, None, :].expand(-1, -1, net.n_sample, -1), raw["dxyz"], raw["ppf"]], dim=-1)
    h = net.postpool(net.prepool(x.permute(0, 3, 2, 1)).max(dim=2)[0]).permute(0, 2, 1)
    out = h / torch.norm(h, dim=-1, keepdim=True)
    assert torch.equal(out.detach(), out_on)
    (out * torch.randn(out.shape, generator=torch.Generator().manual_seed(9))).sum().backward()
    assert all(torch.equal(p.grad, g) for p, g in zip(net.parameters(), g_on))


def test_gate_needs_grad_mode_a_parameter_and_the_switch():
    """the parts of trains_on_hip that need no device: a meta tensor stands for a device fp32 cloud"""
    net, xyz, nrm = _tiny()
    fake = lambda t: type("T", (), {"is_cuda": True, "dtype": torch.float32, "requires_grad": t})()      # noqa: E731
    assert net.trains_on_hip(fake(False), fake(False))
    assert not net.trains_on_hip(fake(True), fake(False))                 # a cloud that requires a gradient: the op sequence
    with torch.no_grad():
        assert not net.trains_on_hip(fake(False), fake(False))
    with ppfnet.op_sequence_only():
        assert not net.trains_on_hip(fake(False), fake(False))
    assert net.trains_on_hip(fake(False), fake(False))
    _fused.TRAIN_HIP = False
    try:
        assert not net.trains_on_hip(fake(False), fake(False))
    finally:
        _fused.TRAIN_HIP = True
    frozen = copy.deepcopy(net).requires_grad_(False)
    assert not frozen.trains_on_hip(fake(False), fake(False))
    frozen.postpool[6].bias.requires_grad_(True)
    assert frozen.trains_on_hip(fake(False), fake(False))
    assert not PPFNet(features=["ppf", "dxyz"]).trains_on_hip(fake(False), fake(False))
    assert not PPFNet(emb_dims=40).trains_on_hip(fake(False), fake(False))


@pytest.mark.parametrize("learn,want", [
    # which of (conv, norm) per layer learn -> the launches, last layer first
    ([(1, 1), (1, 1), (1, 1)], "w2 b2 d2 n1 w1 b1 d1 n0 w0 b0"),
    ([(0, 0), (0, 0), (1, 1)], "w2 b2"),                       # nothing underneath learns: no dgrad at all
    ([(0, 0), (0, 1), (1, 0)], "w2 b2 d2 n1"),                 # only the GroupNorm below: its backward, then stop
    ([(1, 0), (0, 0), (0, 0)], "d2 n1 d1 n0 w0 b0"),           # only the first convolution: all the way down, no wgrad on the way
    ([(0, 0), (1, 0), (0, 1)], "d2 n1 w1 b1"),
])
def test_backward_descent_stops_where_nothing_underneath_learns(monkeypatch, learn, want):
    """ppfnet.backward_descent on a three-layer stack with the launches stubbed (a gradient is a tensor holding its layer's number):
    what runs for each pattern of parameters that need a gradient, which gradients come back, that the list it takes dz in is
    emptied, and that only the pooled layer's GroupNorm gets the winner index"""
    from learning3d_amd.models import _train
    layers = [(torch.nn.Conv1d(4, 4, 1), torch.nn.GroupNorm(2, 4)) for _ in range(3)]
    order = [p for c, n in layers for p in (c.weight, c.bias, n.weight, n.bias)]
    slot = {id(p): j for j, p in enumerate(order)}
    needs = [bool(learn[j // 4][(j % 4) // 2]) for j in range(12)]
    ran = []
    at = lambda i: torch.full((1, 4, 1), float(i))                        # noqa: E731
    log = lambda tag, dz, out: ran.append(f"{tag}{int(dz[0, 0, 0])}") or out       # noqa: E731
    monkeypatch.setattr(_train, "wgrad", lambda dz, u: log("w", dz, torch.zeros(4, 4)) if u == int(dz[0, 0, 0]) else None)
    monkeypatch.setattr(_train, "channel_stats", lambda dz: log("b", dz, torch.zeros(1, 4, 2)))
    monkeypatch.setattr(_train, "sum_clouds", lambda t: t[0])
    monkeypatch.setattr(ppfnet, "gn_conv", lambda dz, a, s, w, b: (log("d", dz, dz), None, None, None))

    def gn_backward(du, y, a, s, stat, gamma, groups, widx=None, K=0, want_gamma=True, want_beta=True):
        i = int(du[0, 0, 0]) - 1                                          # du came from the layer above
        assert (y, a, s, stat) == (f"y{i}", f"a{i}", f"s{i}", f"stat{i}") and gamma is order[4 * i + 2] and groups == 2
        assert (widx, K) == (("widx", 5) if i == 1 else (None, 0))
        assert (want_gamma, want_beta) == (needs[4 * i + 2], needs[4 * i + 3])
        ran.append(f"n{i}")
        return at(i), at(i) if want_gamma else None, at(i) if want_beta else None
    monkeypatch.setattr(ppfnet, "gn_backward", gn_backward)

    grads, box = [None] * 12, [at(2)]
    ys, stats, affs = ["y0", "y1", "y2"], ["stat0", "stat1", "stat2"], ["a0", "s0", "a1", "s1", "a2", "s2"]
    ppfnet.backward_descent(layers, ys, affs, stats, order, needs, slot, grads, box, 2, lambda i: i, pooled=(1, "widx", 5))
    assert box == [] and " ".join(ran) == want
    for j, g in enumerate(grads):
        i, kind = j // 4, "wbnn"[j % 4]
        assert (g is not None) == (needs[j] and f"{kind}{i}" in want.split()), (j, g)


def test_the_plumbing_case_meets_its_condition_here():
    """the RPMNet pair of the GPU plumbing test: the op sequence's fp32 gradients within 1e-3 of scale of fp64 on every tensor, on
    this machine's CPU, and the fixture's table names every parameter"""
    net, t, s, igt = tf.plumbing_case()
    n64 = copy.deepcopy(net).double()
    g32 = tf.plumbing_gradients(net, t, s, igt)
    g64 = tf.plumbing_gradients(n64, t.double(), s.double(), igt.double())
    assert set(g64) == set(tf.PLUMBING_GAPS) == {n for n, _ in net.named_parameters()} and len(g64) == 52
    for n, want in g64.items():
        gap = float((g32[n].double() - want).abs().max() / want.abs().max())
        assert gap <= tf.PLUMBING_CONDITION, (n, gap)
        assert tf.PLUMBING_GAPS[n] <= tf.PLUMBING_CONDITION / 10
