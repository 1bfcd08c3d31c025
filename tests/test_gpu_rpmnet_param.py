"""ParameterPredictionNet's HIP routes on the GPU (models/rpmnet.py, rpmnet_param.hip, include/ext/l3d_rpmnet_param.h).

1. l3d_gn_conv_gpool at its edges: extremes and their lowest positions bit for bit those of the y that l3d_gn_conv(pool = 0) of the
   same build writes, the moments within the worst-case bound of any fp64 summation order, the same bits on repeated calls whatever
   the outputs and the workspace held.
2. l3d_gn_gpool_backward: dz, dgamma, dbeta one fp32 rounding of the fp64 formula (golden/rpmnet_param_fixture.py, which the CPU
   tests hold to torch.autograd) evaluated from the kernel's own fp32 y.
3. the module: all 30 parameter gradients against the reference's op sequence in fp64 on the branches the differentiated forward
   took (the tier, or twice the fp32 torch mirror's own error where that exceeds the tier); beta and alpha of both routes.
4. RPMNet's plumbing: the launch log of every route, the fused forward from a captured graph, all 52 parameter gradients with the
   switch on and off.
5. state and layout: repeat backward, an optimizer step, frozen lower layers, views, what the forward keeps for the backward.
6. the memory contract and the guards of both entry points."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import memory_contract as mc            # noqa: E402
import rpmnet_param_fixture as pf       # noqa: E402
import rpmnet_train_fixture as tf       # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEW = ("l3d_gn_conv_gpool", "l3d_gn_gpool_backward")
ULP = 2.0 ** -23


def _mods():
    from learning3d_amd import _lib
    from learning3d_amd.models import _fused, ppfnet, rpmnet
    return _lib, _fused, ppfnet, rpmnet


class _log:
    def __enter__(self):
        _mods()[0].LAUNCH_LOG = self.log = []
        return self.log

    def __exit__(self, *exc):
        _mods()[0].LAUNCH_LOG = None
        return False


class _switch:
    """`with _switch(module, "NAME", value):` -- a module switch for the block"""

    def __init__(self, mod, name, value):
        self.mod, self.name, self.value = mod, name, value

    def __enter__(self):
        self.prev = getattr(self.mod, self.name)
        setattr(self.mod, self.name, self.value)

    def __exit__(self, *exc):
        setattr(self.mod, self.name, self.prev)
        return False


def _offset(t):
    """the same values at a data pointer one element past a 16-byte boundary"""
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert flat.data_ptr() % 16 == 0
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


def _rounded_once(got, want64, what):
    err = (got.double() - want64).abs()
    bar = ULP * want64.abs() + 1e-12 * float(want64.abs().max())
    assert bool((err <= bar).all()), (what, float(err.max()), float(want64.abs().max()))


def _reference_y(x, in_a, in_s, w, bias):
    """y [B,Cout,P] as l3d_gn_conv(pool = 0) of this build writes it, 256 output channels (its limit) at a time: a channel's value
    does not depend on which workgroup or wave tile holds it"""
    _lib, _, ppfnet, _ = _mods()
    step = _lib.L3D_GN_CONV_MAX_COUT
    return torch.cat([ppfnet.gn_conv(x, in_a, in_s, w[c:c + step].contiguous(), bias[c:c + step].contiguous())[0]
                      for c in range(0, w.shape[0], step)], 1)


def _plan_p():
    """a P at which a workgroup takes more than one block of 64 positions under the kernel's plan, with a partial last block"""
    return _mods()[0].L3D_GN_GPOOL_PARTS * 64 + 70


def _raw_gpool(x, in_a, in_s, w, bias, fill):
    """the entry point itself on outputs and a workspace pre-filled with `fill` (NaN; -1 in the positions)"""
    _lib = _mods()[0]
    B, Cin, P = x.shape
    Cout = w.shape[0]
    f = lambda dt, *s: torch.full(s, fill if dt.is_floating_point else -1, dtype=dt, device=DEV)       # noqa: E731
    ymax, ymin, pmax, pmin = f(torch.float32, B, Cout), f(torch.float32, B, Cout), f(torch.int32, B, Cout), f(torch.int32, B, Cout)
    mom = f(torch.float64, B, Cout, 2)
    ws = f(torch.float64, _lib.lib().l3d_gn_conv_gpool_workspace_bytes(B, Cout, P) // 8)
    _lib.call("l3d_gn_conv_gpool", x, in_a, in_s, w, bias, B, Cin, Cout, P, ymax, ymin, pmax, pmin, mom, ws)
    return ymax, ymin, pmax, pmin, mom


# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cout", [16, 48, 1024])
def test_gpool_forward_at_its_edges(Cout):
    _lib, _, _, rpmnet = _mods()
    B = 3
    parts = _lib.lib().l3d_gn_conv_gpool_workspace_bytes(B, Cout, _plan_p()) // (B * Cout * 32)
    assert 1 < parts < (_plan_p() + 63) // 64, "a workgroup takes more than one block of positions at this P"
    for P in (1, 63, 64, 65, 150, _plan_p()):
        for Cin in (4, 5, 64, 130):
            for affine in (False, True):
                case = (Cout, P, Cin, affine)
                x, in_a, in_s, w, bias = pf.conv_case(11 * P + Cin + Cout + affine, B, Cin, Cout, P, affine, dev=DEV)
                y = _reference_y(x, in_a, in_s, w, bias)
                want = pf.extremes_of(y)
                if affine:
                    assert bool((in_a == 0).any()) and bool((in_a < 0).any())
                elif P >= 6:
                    assert bool(((y == want[0][:, :, None]).sum(2) >= 2).any()) and bool(((y == want[1][:, :, None]).sum(2) >= 2).any()), \
                        ("each extreme attained twice", case)
                    lift = y - bias[None, :, None]
                    assert bool(((lift > 0).all(2) | (lift < 0).all(2)).all()), ("a padding column would be an extreme", case)
                got = rpmnet.gn_conv_gpool(x, in_a, in_s, w, bias)
                for g, wnt, what in zip(got[:4], want, ("ymax", "ymin", "pmax", "pmin")):
                    assert torch.equal(g.long() if what[0] == "p" else g, wnt), (what, case)
                assert got[2].dtype == got[3].dtype == torch.int32
                y64 = y.double()
                for q, terms in enumerate((y64, y64 * y64)):
                    err = (got[4][..., q] - terms.sum(2)).abs()
                    assert bool((err <= P * 2.0 ** -53 * terms.abs().sum(2)).all()), ("moments", q, case, float(err.max()))
                for again in (_raw_gpool(x, in_a, in_s, w, bias, float("nan")), _raw_gpool(_offset(x), in_a, in_s, _offset(w), bias, float("nan"))):
                    assert all(torch.equal(a, b) for a, b in zip(again, got)), ("a repeated call differs", case)


# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 48])
def test_gpool_backward_at_its_edges(C):
    _lib, _, ppfnet, rpmnet = _mods()
    B, groups = 3, pf.groups_of(C)
    for P in (1, 63, 64, 65, 150, _plan_p()):
        for Cin, affine in ((5, False), (64, True), (130, True)):
            case = (C, P, Cin, affine)
            x, in_a, in_s, w, bias = pf.conv_case(13 * P + Cin + C, B, Cin, C, P, affine, dev=DEV)
            gamma, beta, du = pf.layer_case(17 * P + Cin + C, B, C, dev=DEV)
            beta[6:8] = 3.0                                           # the channels whose winners are moved below stay open
            y = _reference_y(x, in_a, in_s, w, bias)
            ymax, ymin, pmax, pmin, mom = rpmnet.gn_conv_gpool(x, in_a, in_s, w, bias)
            norm = torch.nn.GroupNorm(groups, C, eps=pf.EPS).to(DEV)
            with torch.no_grad():
                norm.weight.copy_(gamma)
                norm.bias.copy_(beta)
            a, s = ppfnet.gn_affine(mom, norm, P)
            stat = ppfnet.gn_mean_rstd(mom, groups, P, pf.EPS)
            assert bool((a == 0).any()) and bool((a < 0).any()) and bool((a > 0).any())
            ext, pw = torch.where(a >= 0, ymax, ymin), torch.where(a >= 0, pmax, pmin)
            want_ext, want_pw = pf.winners_of(y, a)
            assert torch.equal(ext, want_ext) and torch.equal(pw.long(), want_pw)
            # the formula holds for any position and the value of y there: winners at p = 0 and at P - 1, the last (partial) block
            pw, ext = pw.clone(), ext.clone()
            pw[:, 6], pw[:, 7] = 0, P - 1
            ext[:, 6], ext[:, 7] = y[:, 6, 0], y[:, 7, P - 1]
            mask = rpmnet.ParameterPredictionNet._pooled(a, s, ext) > 0
            g = du * mask
            assert bool((g == 0).any()) and bool((g[:, 6:8] != 0).all())
            want = pf.gpool_backward64(du, y, ext, pw, a, s, stat[..., 0], stat[..., 1], gamma, groups, mask=mask)
            outs = []
            for shift in (False, True):
                xx, ww = (_offset(x), _offset(w)) if shift else (x, w)
                dz, dg, db = rpmnet.gn_gpool_backward(xx, in_a, in_s, ww, bias, g, ext, pw, stat, gamma, groups)
                _rounded_once(dz, want[0], ("dz", case, shift))
                _rounded_once(dg, want[1], ("dgamma", case, shift))
                _rounded_once(db, want[2], ("dbeta", case, shift))
                outs.append((dz, dg, db))
            assert all(torch.equal(p, q) for p, q in zip(*outs)), ("operands off a 16-byte boundary give other bits", case)
            only = rpmnet.gn_gpool_backward(x, in_a, in_s, w, bias, g, ext, pw, stat, gamma, groups, want_dz=False, want_gamma=False)
            assert only[0] is None and only[1] is None and torch.equal(only[2], outs[0][2])


# ------------------------------------------------------------------------------------------------------------------------------
def _respell(net, src, ref):
    """the differentiated forward spelled with the public wrappers under no_grad -> (beta, alpha, pooled, masks, winners)"""
    _, _, ppfnet, rpmnet = _mods()
    x = pf.param_input(src, ref).contiguous()
    P = x.shape[2]
    a = s = None
    masks = []
    layers = net._layers()
    for conv, norm in layers[:-1]:
        y, _, _, mom = ppfnet.gn_conv(x, a, s, conv.weight, conv.bias)
        a, s = ppfnet.gn_affine(mom, norm, P)
        masks.append(ppfnet.gn_relu(y, a, s) > 0)
        x = y
    conv, norm = layers[-1]
    ymax, ymin, pmax, pmin, mom = rpmnet.gn_conv_gpool(x, a, s, conv.weight, conv.bias)
    a, s = ppfnet.gn_affine(mom, norm, P)
    pooled = torch.relu(a * torch.where(a >= 0, ymax, ymin) + s)
    masks.append(pooled > 0)
    h, post = pooled, net.postpool
    for i in (0, 3):
        h = post[i + 2](post[i + 1](post[i](h)))
        masks.append(h > 0)
    raw = post[6](h)
    sp = torch.nn.functional.softplus
    return sp(raw[:, 0]), sp(raw[:, 1]), pooled, masks, torch.where(a >= 0, pmax, pmin).long()


def _rel(got, want):
    return float((got.detach().cpu().double() - want.cpu()).abs().max()) / float(want.abs().max())


@pytest.mark.parametrize("B,J,K", [(2, 40, 27), (2, 70, 130)])
def test_module_gradients_vs_fp64(B, J, K, monkeypatch):
    _lib, _, _, rpmnet = _mods()
    cpu_net, src, ref = pf.param_case(90 + J, B, J, K)
    net = copy.deepcopy(cpu_net).to(DEV)
    src, ref = src.to(DEV), ref.to(DEV)
    calls = []
    real = torch.nn.functional.group_norm
    monkeypatch.setattr(torch.nn.functional, "group_norm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    assert net.trains_on_hip(src, ref)
    with _log() as log:
        beta, alpha = net([src, ref])
        n_fwd = len(log)
        pf.head_loss(beta, alpha).backward()
    assert len(calls) == 2, "the head's two GroupNorms are the only ones torch runs"
    assert log[:n_fwd].count("l3d_gn_conv") == 4 and log[:n_fwd].count("l3d_gn_conv_gpool") == 1 and log[:n_fwd].count("l3d_gn_mean_rstd") == 5
    assert log[n_fwd:].count("l3d_gn_gpool_backward") == 1 and log[n_fwd:].count("l3d_wgrad") == 5 and log[n_fwd:].count("l3d_gn_conv") == 4
    with torch.no_grad():
        beta_r, alpha_r, pooled_r, masks, pw = _respell(net, src, ref)
        assert torch.equal(beta_r, beta.detach()) and torch.equal(alpha_r, alpha.detach()), "the re-spelt route is not the function that was differentiated"
        assert net.fused_takes(src, ref)
        pooled_e = net.fused_prepool([src, ref])
        beta_e, alpha_e = net.fused_forward([src, ref])
    pooled_t = net._Train.apply(net, src, ref, *net._parameters_in_order())
    assert torch.equal(pooled_t.detach(), pooled_e) and torch.equal(pooled_e, pooled_r), "the training forward's pooled tensor is the eval route's"
    assert bool((pooled_e > 0).any()) and bool((pooled_e == 0).any())
    got = {n: p.grad for n, p in net.named_parameters()}
    assert len(got) == 30 and all(g is not None and bool(torch.isfinite(g).all()) for g in got.values())
    grads = {}
    for tag, dt in (("fp64", torch.float64), ("fp32", torch.float32)):
        p = {n: v.detach().to(dt).clone().requires_grad_() for n, v in net.named_parameters()}
        b, a = pf.param_mirror(p, src, ref, masks, pw)
        pf.head_loss(b, a).backward()
        grads[tag] = ({n: v.grad for n, v in p.items()}, b.detach(), a.detach())
    failed = []
    print(f"\nParameterPredictionNet (B, J, K) = ({B}, {J}, {K}): relative to max |fp64 gradient|")
    print(f"  {'tensor':<22} {'HIP':>10} {'fp32 torch':>11} {'bar':>10}")
    for n in got:
        want = grads["fp64"][0][n]
        scale = float(want.abs().max())
        e_hip = float((got[n].double() - want).abs().max()) / scale
        e_32 = float((grads["fp32"][0][n].double() - want).abs().max()) / scale
        bar = tf.TIER if e_32 <= tf.TIER else 2 * e_32
        print(f"  {n:<22} {e_hip:>10.2e} {e_32:>11.2e} {bar:>10.1e}")
        if not e_hip <= bar:
            failed.append((n, e_hip, e_32, bar))
    # beta, alpha: against the fp64 op sequence of the module itself, the unit the device op sequence's own gap
    with torch.no_grad():
        b64, a64 = copy.deepcopy(cpu_net).double()([src.cpu().double(), ref.cpu().double()])
        with _switch(rpmnet, "PARAM_HIP", False), _log() as log_seq:
            b_seq, a_seq = net([src, ref])
    assert not any(name.startswith("l3d_gn_") for name in log_seq)
    for what, want, seq, routes in (("beta", b64, b_seq, (beta_e, beta)), ("alpha", a64, a_seq, (alpha_e, alpha))):
        bar = max(pf.GAP_FACTOR * _rel(seq, want), tf.TIER)
        for route, v in zip(("eval", "training"), routes):
            e = _rel(v, want)
            print(f"  {what} on the {route} route: {e:.2e} of scale, bar {bar:.1e}")
            if not e <= bar:
                failed.append((what, route, e, bar))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------------------------
def test_rpmnet_plumbing_and_routes():
    _lib, _fused, _, rpmnet = _mods()
    cpu_net, t, s, igt = tf.plumbing_case()
    n64, dnet = copy.deepcopy(cpu_net).double(), copy.deepcopy(cpu_net).to(DEV)
    g64 = tf.plumbing_gradients(n64, t.double(), s.double(), igt.double())
    td, sd, igtd = t.to(DEV), s.to(DEV), igt.to(DEV)
    with _log() as log:
        hip = tf.plumbing_gradients(dnet, td, sd, igtd)
    assert log.count("l3d_gn_conv_gpool") == 2 and log.count("l3d_gn_gpool_backward") == 2, "once per iteration"
    with _switch(rpmnet, "PARAM_HIP", False), _log() as log_off:
        off = tf.plumbing_gradients(dnet, td, sd, igtd)
    assert not any(name in log_off for name in NEW) and "l3d_gn_conv" in log_off, "the feature network keeps its own route"
    assert len(g64) == 52
    failed = []
    print("\nRPMNet, 2 iterations: max |gradient - fp64| / max |fp64|")
    print(f"  {'tensor':<34} {'PARAM_HIP':>10} {'off':>10} {'on - off':>10} {'gap':>10} {'bar':>10}")
    for n, want in g64.items():
        scale = float(want.abs().max())
        bar = max(tf.GAP_FACTOR * tf.PLUMBING_GAPS[n], tf.TIER)
        e_on, e_off = _rel(hip[n], want), _rel(off[n], want)
        between = float((hip[n].double() - off[n].double()).abs().max()) / scale
        print(f"  {n:<34} {e_on:>10.2e} {e_off:>10.2e} {between:>10.2e} {tf.PLUMBING_GAPS[n]:>10.2e} {bar:>10.1e}")
        if not (e_on <= bar and e_off <= bar):
            failed.append((n, e_on, e_off, bar))
    assert not failed, failed

    # the routes that must stay on torch: neither new entry point, and no l3d_gn_conv at all
    wn = dnet.weights_net
    xs, xt = sd[:, :, :3], td[:, :, :3]

    def quiet(what, fn):
        with _log() as lg:
            out = fn()
        assert not any(name in lg for name in NEW + ("l3d_gn_conv",)), (what, lg)
        return out
    with _switch(rpmnet, "PARAM_HIP", False):
        assert not wn.trains_on_hip(xs, xt)
        quiet("PARAM_HIP = False", lambda: wn([xs, xt]))
    with _switch(_fused, "TRAIN_HIP", False):
        quiet("TRAIN_HIP = False", lambda: tf.plumbing_gradients(dnet, td, sd, igtd))
    quiet("a template that requires a gradient", lambda: dnet(td.clone().requires_grad_(True), sd, 2))
    quiet("CPU input", lambda: cpu_net.weights_net([s[:, :, :3], t[:, :, :3]]))
    quiet("fp64 input", lambda: copy.deepcopy(wn).double()([xs.double(), xt.double()]))
    with torch.no_grad():
        with _switch(rpmnet, "FUSED", False):
            quiet("no_grad with FUSED = False", lambda: dnet(td, sd, 2))
        loose = copy.deepcopy(dnet)
        loose.add_slack = False
        quiet("add_slack = False", lambda: loose(td, sd, 2))

    # the fused eval forward: once per iteration, and from a captured graph with equal bits
    flat = lambda r: [r["est_T"], r["beta"], r["alpha"], *r["transforms"], *r["perm_matrices"], *r["weighted_template"]]       # noqa: E731
    with torch.no_grad():
        with _log() as lg:
            eager = [v.clone() for v in flat(dnet._forward_fused(td, sd, 2))]
        assert lg.count("l3d_gn_conv_gpool") == 2 and "l3d_gn_gpool_backward" not in lg
        with _switch(rpmnet, "PARAM_HIP", False), _log() as lg:
            plain = [v.clone() for v in flat(dnet._forward_fused(td, sd, 2))]
        assert "l3d_gn_conv_gpool" not in lg and lg.count("l3d_ppf_group") == 3
        for q, a, b in zip(("est_T", "beta", "alpha"), eager, plain):
            assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max()), (q, "the two routes are one function")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            dnet._forward_fused(td, sd, 2)                               # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = flat(dnet._forward_fused(td, sd, 2))
        for replay in range(2):
            for v in out:
                v.fill_(7.0)                                             # stale values must not survive a replay
            graph.replay()
            torch.cuda.synchronize()
            for i, (a, b) in enumerate(zip(out, eager)):
                assert torch.equal(a, b), (replay, i)


# ------------------------------------------------------------------------------------------------------------------------------
def _grads(net, src, ref):
    net.zero_grad(set_to_none=True)
    beta, alpha = net([src.clone(), ref.clone()])
    pf.head_loss(beta, alpha).backward()
    return (beta.detach(), alpha.detach()), [None if p.grad is None else p.grad.clone() for p in net.parameters()]


def test_route_and_state():
    _lib, _fused, _, rpmnet = _mods()
    cpu_net, src, ref = pf.param_case(31, 2, 70, 45)
    net, src, ref = cpu_net.to(DEV), src.to(DEV), ref.to(DEV)
    with _log() as log:
        out1, g1 = _grads(net, src, ref)
    assert log.count("l3d_wgrad") == 5 and log.count("l3d_gn_backward_apply") == 4 and log.count("l3d_gn_gpool_backward") == 1
    out2, g2 = _grads(net, src, ref)                                   # fresh inputs, stale workspaces: the same bits
    assert all(torch.equal(a, b) for a, b in zip(out1, out2)) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    frozen = [p for n, p in net.named_parameters() if n.startswith("prepool.") and int(n.split(".")[1]) < 9]
    assert len(frozen) == 12
    for p in frozen:                                                   # layers 4 and 5 and the head learn: the rest gets no gradient
        p.requires_grad_(False)
    with _log() as log:
        _, g3 = _grads(net, src, ref)
    assert all(g is None for g in g3[:12]) and log.count("l3d_wgrad") == 2
    assert log.count("l3d_gn_backward_apply") == 1 and log.count("l3d_gn_relu") == 2, "the backward stops at the lowest layer that learns"
    assert all(torch.equal(a, b) for a, b in zip(g3[12:], g1[12:]))
    for p in net.prepool.parameters():                                 # only the head learns: the pre-pool stack is torch's
        p.requires_grad_(False)
    assert not net.trains_on_hip(src, ref)
    for p in net.prepool.parameters():
        p.requires_grad_(True)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    _grads(net, src, ref)
    opt.step()
    out3 = [v.detach() for v in net([src, ref])]
    with torch.no_grad():
        assert not torch.equal(out3[0], out1[0])
        assert all(torch.equal(a, b) for a, b in zip(out3, net.fused_forward([src, ref])))


def test_forward_keeps_no_wide_tensor():
    """what lives between forward and backward, at B 2 and P = J + K = 1100: the HIP route keeps the input and y1..y4 (0.31 of one
    [B,1024,P] fp32 tensor), the op sequence at least the last layer's convolution output and its normalised value"""
    _lib, _fused, _, rpmnet = _mods()
    B, J, K = 2, 500, 600
    cpu_net, src, ref = pf.param_case(41, B, J, K)
    net, src, ref = cpu_net.to(DEV), src.to(DEV), ref.to(DEV)
    wide = B * 1024 * (J + K) * 4
    _grads(net, src[:, :8], ref[:, :8])            # the head's first matrix product allocates torch's BLAS workspace, which stays
    kept = {}
    for hip in (True, False):
        with _switch(rpmnet, "PARAM_HIP", hip):
            net.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            beta, alpha = net([src, ref])
            torch.cuda.synchronize()
            kept[hip] = torch.cuda.memory_allocated() - base
            pf.head_loss(beta, alpha).backward()
            del beta, alpha
    print(f"\nkept for the backward at B {B}, P {J + K}: {kept[True] / wide:.2f} of a [B,1024,P] tensor on the HIP route, "
          f"{kept[False] / wide:.2f} on the op sequence")
    assert kept[True] < wide and kept[False] > 2 * wide


# ------------------------------------------------------------------------------------------------------------------------------
# ParameterPredictionNet._Train as tests/test_gpu_views_backward.py holds every autograd.Function of the package: gradients that arrive
# as views and inputs that are views, bit for bit and launch for launch against contiguous clones; every tensor a launch receives is
# contiguous.
def _views_case(monkeypatch):
    import layout_audit
    from view_cases import assert_identical, float_views, grad_views, logged, whole_storage
    _lib, _, ppfnet, rpmnet = _mods()
    layout_audit.install(monkeypatch)
    for mod in (ppfnet, rpmnet):
        inner = mod.call

        def contiguous_only(name, *args, _inner=inner, **kw):
            for i, a in enumerate(args):
                assert not isinstance(a, torch.Tensor) or a.is_contiguous(), (name, i, tuple(a.shape), a.stride())
            return _inner(name, *args, **kw)
        monkeypatch.setattr(mod, "call", contiguous_only)
    cpu_net, src, ref = pf.param_case(51, 2, 70, 45)
    net = cpu_net.to(DEV)
    params = net._parameters_in_order()

    def run(a, b, g):
        out = net._Train.apply(net, a, b, *params)
        return out, torch.autograd.grad([out], params, [g])
    return net, src.to(DEV), ref.to(DEV), run, (assert_identical, float_views, grad_views, logged, whole_storage)


def test_train_function_on_view_gradients(monkeypatch):
    net, src, ref, run, (assert_identical, _, grad_views, logged, whole_storage) = _views_case(monkeypatch)
    shape = (2, 1024)
    views = dict(grad_views(shape, seed=50))
    assert set(views) == {"transposed", "stride2", "expand"}
    for kind, g in views.items():
        (out, want), log = logged(run, src, ref, g.contiguous())
        assert tuple(out.shape) == shape and "l3d_gn_gpool_backward" in log and "l3d_wgrad" in log
        before = whole_storage(g).clone()
        (out_v, got), vlog = logged(run, src, ref, g)
        assert vlog == log, (kind, vlog, log)
        assert_identical((out_v, got), (out, want), f"gradient as a {kind} view {g.stride()}")
        assert torch.equal(whole_storage(g), before), f"{kind}: the gradient's buffer was written to"


def test_train_function_on_view_inputs(monkeypatch):
    net, src, ref, run, (assert_identical, float_views, grad_views, logged, whole_storage) = _views_case(monkeypatch)
    g = dict(grad_views((2, 1024), seed=70))["stride2"]
    ran = 0
    for (kind, av), (_, bv) in zip(float_views(src), float_views(ref)):
        assert not av.is_contiguous() and not bv.is_contiguous()
        ad, bd = av.clone(memory_format=torch.contiguous_format), bv.clone(memory_format=torch.contiguous_format)
        want, log = logged(run, ad, bd, g)
        again, log2 = logged(run, ad, bd, g)
        assert log2 == log
        assert_identical(again, want, f"{kind}: two runs on the same contiguous inputs")
        before = [whole_storage(v).clone() for v in (av, bv)]
        got, vlog = logged(run, av, bv, g)
        assert vlog == log, (kind, vlog, log)
        assert_identical(got, want, f"inputs as {kind} views {av.stride()}")
        assert all(torch.equal(whole_storage(v), b) for v, b in zip((av, bv), before)), f"{kind}: an input's buffer was written to"
        ran += 1
    assert ran == 4


# ------------------------------------------------------------------------------------------------------------------------------
_SCRATCH = {
    "l3d_gn_conv_gpool": {"workspace": mc.Spec("scratch", "`workspace` (l3d_gn_conv_gpool_workspace_bytes(B, Cout, P) bytes",
                                               size=("l3d_gn_conv_gpool_workspace_bytes", lambda v: (v["B"], v["Cout"], v["P"]), 1))},
}


def _contract(name, build):
    _lib = _mods()[0]
    return mc.check(name, build, proto=_lib.EXT_PROTOTYPES[name], contract=_SCRATCH)


def _rand(seed, *shape):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)).to(DEV) * 2 - 1


@pytest.mark.parametrize("B,Cin,Cout,P,affine", [(2, 5, 16, 150, False), (1, 130, 48, 1094, True), (2, 64, 1024, 65, True), (3, 4, 32, 1, False)])
def test_memory_contract(B, Cin, Cout, P, affine):
    """both entry points: guards, two fills, const inputs unchanged, the workspace by its size function"""
    _lib = _mods()[0]
    G = pf.groups_of(Cout)
    x, w, bias = _rand(1, B, Cin, P), _rand(2, Cout, Cin) * 0.2, _rand(3, Cout)
    in_a, in_s = (_rand(4, B, Cin), _rand(5, B, Cin)) if affine else (None, None)
    ws_bytes = _lib.lib().l3d_gn_conv_gpool_workspace_bytes(B, Cout, P)
    assert ws_bytes % 8 == 0 and ws_bytes > 0
    out = _contract("l3d_gn_conv_gpool", lambda ar: [x, in_a, in_s, w, bias, B, Cin, Cout, P, ar.f32(B, Cout), ar.f32(B, Cout),
                                                     ar.out(torch.int32, B, Cout), ar.out(torch.int32, B, Cout),
                                                     ar.out(torch.float64, B, Cout, 2), ar.bytes(ws_bytes)])
    y = _reference_y(x, in_a, in_s, w, bias)
    want = pf.extremes_of(y)
    for name, wnt in zip(("ymax", "ymin", "pmax", "pmin"), want):
        assert torch.equal(out[name].long() if name[0] == "p" else out[name], wnt), name
    _contract("l3d_gn_conv_gpool", lambda ar: [x, in_a, in_s, w, None, B, Cin, Cout, P, ar.f32(B, Cout), ar.f32(B, Cout),
                                               ar.out(torch.int32, B, Cout), ar.out(torch.int32, B, Cout),
                                               ar.out(torch.float64, B, Cout, 2), ar.bytes(ws_bytes)])
    g, gamma = _rand(6, B, Cout), _rand(7, Cout)
    pw = out["pmax"].clone()
    mean, rstd = tf.group_stats64(y, G)
    stat = torch.stack([mean, rstd], -1).contiguous()
    m = (_rand(8, B, G, 2) * 0.1).double()
    dz = _contract("l3d_gn_gpool_backward", lambda ar: [x, in_a, in_s, w, bias, g, pw, stat, gamma, m, B, Cin, Cout, G, P,
                                                        ar.f32(B, Cout, P)])["dz"]
    cpg = Cout // G
    zhat = (y.double() - mean.repeat_interleave(cpg, 1)[:, :, None]) * rstd.repeat_interleave(cpg, 1)[:, :, None]
    top = torch.zeros_like(zhat).scatter_(2, pw.long()[:, :, None], (gamma.double()[None] * g.double())[:, :, None])
    want_dz = rstd.repeat_interleave(cpg, 1)[:, :, None] * ((top - m[..., 0].repeat_interleave(cpg, 1)[:, :, None])
                                                            - zhat * m[..., 1].repeat_interleave(cpg, 1)[:, :, None])
    _rounded_once(dz, want_dz, ("dz", B, Cin, Cout, P))


def test_guards_refuse_before_any_launch():
    _lib = _mods()[0]
    B, Cin, P = 1, 4, 8
    x = _rand(1, B, 4100, P)

    def fwd(Cin, Cout, P, x=x, w=None, B=B):
        w = _rand(2, 4112, 8) if w is None else w
        o = [torch.full((4112,), 3.0, device=DEV), torch.full((4112,), 3.0, device=DEV),
             torch.full((4112,), 3, dtype=torch.int32, device=DEV), torch.full((4112,), 3, dtype=torch.int32, device=DEV),
             torch.full((4112, 2), 3.0, dtype=torch.float64, device=DEV)]       # (sized for one cloud: B = 65536 is refused unread)
        ws = torch.full((4112 * 8,), 3.0, dtype=torch.float64, device=DEV)
        try:
            _lib.call("l3d_gn_conv_gpool", x, None, None, w, None, B, Cin, Cout, P, *o, ws)
        except _lib.L3DError as e:
            torch.cuda.synchronize()
            assert all(bool((t == 3).all()) for t in o + [ws]), "a refused call wrote"
            return str(e)
        return "ok"
    unsupported, invalid = f"status {_lib.L3D_ERR_UNSUPPORTED}", f"status {_lib.L3D_ERR_INVALID_ARG}"
    assert fwd(4, 16, P) == "ok"
    assert unsupported in fwd(4, 24, P) and unsupported in fwd(4, 8, P) and unsupported in fwd(4, _lib.L3D_GN_GPOOL_MAX_COUT + 16, P)
    assert unsupported in fwd(_lib.L3D_GN_CONV_MAX_CIN + 1, 16, P) and unsupported in fwd(4, 16, P, B=65536)
    assert invalid in fwd(4, 16, 0) and invalid in fwd(0, 16, P) and invalid in fwd(4, 16, P, x=None)
    a = _rand(3, B, 4)
    with pytest.raises(_lib.L3DError, match=invalid):
        _lib.call("l3d_gn_conv_gpool", x, a, None, _rand(2, 16, 4), None, B, 4, 16, P, *[torch.empty(B, 16, device=DEV)] * 2,
                  *[torch.empty(B, 16, dtype=torch.int32, device=DEV)] * 2, torch.empty(B, 16, 2, dtype=torch.float64, device=DEV),
                  torch.empty(64, dtype=torch.float64, device=DEV))

    def bwd(Cin, Cout, groups, P, g=_rand(4, B, 48)):
        dz = torch.full((B, 48, 8), 3.0, device=DEV)
        stat = torch.ones((B, 48, 2), dtype=torch.float64, device=DEV)
        try:
            _lib.call("l3d_gn_gpool_backward", x, None, None, _rand(2, 48, 8), None, g, torch.zeros((B, 48), dtype=torch.int32, device=DEV),
                      stat, _rand(5, 48), stat, B, Cin, Cout, groups, P, dz)
        except _lib.L3DError as e:
            torch.cuda.synchronize()
            assert bool((dz == 3).all()), "a refused call wrote"
            return str(e)
        return "ok"
    assert bwd(4, 48, 8, P) == "ok"
    assert unsupported in bwd(4, 48, 5, P) and unsupported in bwd(4, 40, 8, P) and unsupported in bwd(_lib.L3D_GN_CONV_MAX_CIN + 1, 48, 8, P)
    assert invalid in bwd(4, 48, 0, P) and invalid in bwd(4, 48, 8, P, g=None)
