"""PPFNet's differentiable HIP route on the GPU (models/ppfnet.py PPFNet._Train, rpmnet_train.hip, include/ext/l3d_rpmnet_train.h).

1. the kernels at their edges against the fp64 statement of the formulas (golden/rpmnet_train_fixture.py, which the CPU tests hold
   to torch.autograd): both the 16-byte and the scalar route, a GroupNorm scale with zeros and negatives, P below / at / above a wave,
   pooled with K = 1, an odd K and K = 64.  Outputs that are one fp32 rounding of an fp64 value are held to 2^-23 of their value.
2. every parameter gradient of PPFNet (22 tensors) against the reference's op sequence in fp64 on the branches the differentiated
   forward took, by the method of tests/test_gpu_grad_modules.py.  Bar: the tier, max |got - fp64| <= 1e-5 max |fp64| per tensor;
   a tensor on which the fp32 torch mirror itself exceeds the tier is held to twice the mirror's error (LABLOG.md R23.1).
3. RPMNet's plumbing: two iterations, the bench's loss, every parameter gradient against the device op sequence and the CPU fp64 one,
   each within GAP_FACTOR = 4 of the op sequence's own fp32-to-fp64 gap, floored at the tier.
4. route and state: the launch log, repeat backward, an optimizer step, the peak allocation against the op sequence's.
5. the memory contract of every new entry point."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import memory_contract as mc            # noqa: E402
import rpmnet_train_fixture as tf       # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEW = ("l3d_gn_mean_rstd", "l3d_gn_pool_winner", "l3d_gn_relu", "l3d_gn_backward_stats", "l3d_gn_backward_reduce",
       "l3d_gn_backward_apply")
ULP = 2.0 ** -23


def _mods():
    from learning3d_amd import _lib
    from learning3d_amd.models import _fused, ppfnet
    return _lib, _fused, ppfnet


class _log:
    def __enter__(self):
        _lib = _mods()[0]
        _lib.LAUNCH_LOG = self.log = []
        return self.log

    def __exit__(self, *exc):
        _mods()[0].LAUNCH_LOG = None
        return False


def _offset(t):
    """the same values at a data pointer one element (a float; a byte of the winner index) past a 16-byte boundary"""
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


# ------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 0), (63, 0), (64, 0), (65, 0), (150, 0), (70, 1), (210, 3), (320, 64)]          # (P, K): pooled N' = 70, 70, 5


@pytest.mark.parametrize("C", [16, 48, 96])
def test_kernels_at_their_edges(C):
    _lib, _, ppfnet = _mods()
    B = 2
    for P, K in SHAPES:
        y, gamma, beta, du = tf.layer_case(1000 + 7 * C + P + K, B, C, P, K, dev=DEV)
        y64 = y.double()
        moments = torch.stack([y64.sum(2), (y64 * y64).sum(2)], -1).contiguous()
        norm = torch.nn.GroupNorm(tf.GROUPS, C, eps=tf.EPS).to(DEV)
        with torch.no_grad():
            norm.weight.copy_(gamma)
            norm.bias.copy_(beta)
        a, s = ppfnet.gn_affine(moments, norm, P)
        stat = ppfnet.gn_mean_rstd(moments, tf.GROUPS, P, tf.EPS)
        # the entry points take eps as a float: the kernels add the fp32 value of 1e-5.  var = E y^2 - mean^2 carries a few 2^-53 of
        # E y^2, and rstd = (var + eps)^-1/2 multiplies an error of var by rstd^3 / 2
        mean, rstd = tf.group_stats64(y, tf.GROUPS, eps=float(torch.tensor(tf.EPS, dtype=torch.float32)))
        ey2 = (y64 * y64).view(B, tf.GROUPS, -1).mean(2)
        assert bool(((stat[..., 0] - mean).abs() <= 2.0 ** -50 * ey2.sqrt()).all()), (C, P, K)
        assert bool(((stat[..., 1] - rstd).abs() <= 2.0 ** -50 * (ey2 * rstd ** 3 + rstd)).all()), (C, P, K)
        assert bool((a == 0).any()) and bool((a < 0).any()) and bool((a > 0).any())
        widx = want_widx = None
        if K:
            widx = ppfnet.gn_pool_winner(y, a, K)
            want_widx = tf.winners64(y, a, K)
            assert widx.dtype == torch.uint8 and torch.equal(widx.long(), want_widx), (C, P, K)
            assert torch.equal(ppfnet.gn_pool_winner(_offset(y), a, K), widx)
        want_dz, want_dg, want_db, _, _ = tf.gn_relu_backward64(du, y, a, s, stat[..., 0], stat[..., 1], gamma, tf.GROUPS, K, want_widx)
        h64 = a.double()[:, :, None] * y64 + s.double()[:, :, None]
        want_u = h64.clamp_min(0.0)
        outs = []
        for shift in (False, True):
            yy, dd = (_offset(y), _offset(du)) if shift else (y, du)
            ww = _offset(widx) if (shift and K) else widx
            dz, dg, db = ppfnet.gn_backward(dd, yy, a, s, stat, gamma, tf.GROUPS, ww, K)
            _rounded_once(dz, want_dz, ("dz", C, P, K, shift))
            _rounded_once(dg, want_dg, ("dgamma", C, P, K, shift))
            _rounded_once(db, want_db, ("dbeta", C, P, K, shift))
            u = ppfnet.gn_relu(yy, a, s)
            if shift:                                                   # the output off a 16-byte boundary too: the entry point itself
                u_off = _offset(torch.empty_like(u))
                _lib.call("l3d_gn_relu", y, a, s, B, C, P, u_off)
                assert torch.equal(u_off, u)
            assert torch.equal(u > 0, h64 > 0), ("mask", C, P, K, shift)          # the sign of the single-rounded fma is fp64's
            _rounded_once(u, want_u, ("u", C, P, K, shift))
            outs.append((dz, u))
        # u is elementwise: the same bits on both routes.  (dz goes through S1, S2, whose fp64 summation order differs between them.)
        assert torch.equal(outs[0][1], outs[1][1]), ("the two routes differ", C, P, K)


def test_stats_of_several_chunks_and_more_clouds():
    """a row of more than L3D_GN_BWD_CHUNK positions goes through the workspace; B = 3, dense and pooled"""
    _lib, _, ppfnet = _mods()
    B, C = 3, 16
    for P, K in ((2 * _lib.L3D_GN_BWD_CHUNK + 68, 0), (2 * (_lib.L3D_GN_BWD_CHUNK + 5), 2)):
        y, gamma, beta, du = tf.layer_case(77 + K, B, C, P, K, dev=DEV)
        mean, rstd = tf.group_stats64(y, tf.GROUPS)
        stat = torch.stack([mean, rstd], -1).contiguous()
        a64, s64 = tf.affine64(gamma, beta, mean, rstd, tf.GROUPS)
        a, s = a64.float(), s64.float()
        widx = ppfnet.gn_pool_winner(y, a, K) if K else None
        want_dz, want_dg, want_db, _, _ = tf.gn_relu_backward64(du, y, a, s, mean, rstd, gamma, tf.GROUPS, K, None if widx is None else widx.long())
        dz, dg, db = ppfnet.gn_backward(du, y, a, s, stat, gamma, tf.GROUPS, widx, K)
        _rounded_once(dz, want_dz, ("dz", P, K))
        _rounded_once(dg, want_dg, ("dgamma", P, K))
        _rounded_once(db, want_db, ("dbeta", P, K))


# ------------------------------------------------------------------------------------------------------------------------------
def _respell(net, xyz, nrm):
    """train_features spelled with the public wrappers under no_grad -> (output, idx, masks, winners)"""
    _, _, ppfnet = _mods()
    from learning3d_amd.utils import ppfnet_util
    B, N, _ = xyz.shape
    K = net.n_sample
    itself = torch.arange(N, device=xyz.device)[None].repeat(B, 1)
    idx = ppfnet_util.query_ball_point(net.radius, K, xyz, xyz, itself_indices=itself)
    x, a, s, masks, widx = ppfnet.ppf_group(xyz, nrm, idx).view(B, 10, K * N), None, None, [], None
    for i, (conv, norm) in enumerate(net._layers()):
        y, ymax, ymin, mom = ppfnet.gn_conv(x, a, s, conv.weight, conv.bias, pool=K if i == 2 else 0)
        if norm is None:
            break
        a, s = ppfnet.gn_affine(mom, norm, K * N if i <= 2 else N)
        x = y
        if i == 2:
            widx = ppfnet.gn_pool_winner(y, a, K)
            x = torch.where((a >= 0)[:, :, None], ymax, ymin)
        masks.append(ppfnet.gn_relu(x, a, s) > 0)
    out = y.permute(0, 2, 1)
    return out / torch.norm(out, dim=-1, keepdim=True), idx, masks, widx


@pytest.mark.parametrize("emb_dims,K,N", [(32, 5, 70), (96, 64, 40)])
def test_ppfnet_parameter_gradients_vs_fp64(emb_dims, K, N, monkeypatch):
    _lib, _, ppfnet = _mods()
    cpu_net, xyz, nrm = tf.ppfnet_case(21 + K, emb_dims, K, N)
    net = copy.deepcopy(cpu_net).to(DEV)
    xyz, nrm = xyz.to(DEV), nrm.to(DEV)
    calls = []
    real = torch.nn.functional.group_norm
    monkeypatch.setattr(torch.nn.functional, "group_norm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with _log() as log:
        out = net(xyz, nrm)
        w = torch.randn(out.shape, generator=torch.Generator().manual_seed(977)).to(DEV)
        n_fwd = len(log)
        (out * w).sum().backward()
    assert not calls and all(name in log[n_fwd:] for name in ("l3d_gn_backward_stats", "l3d_gn_backward_apply", "l3d_wgrad", "l3d_gn_relu"))
    with torch.no_grad():
        out_r, idx, masks, widx = _respell(net, xyz, nrm)
    assert torch.equal(out_r, out.detach()), "the re-spelt route is not the function that was differentiated"
    pad = idx == torch.arange(N, device=DEV)[None, :, None]
    assert bool(pad.any()) and (K > N or bool((~pad).all(-1).any())), "short balls and, where they fit, full ones"
    got = {n: p.grad for n, p in net.named_parameters()}
    assert len(got) == 22 and all(g is not None and bool(torch.isfinite(g).all()) for g in got.values())
    grads = {}
    for tag, dt in (("fp64", torch.float64), ("fp32", torch.float32)):
        p = {n: v.detach().to(dt).clone().requires_grad_() for n, v in net.named_parameters()}
        o = tf.ppfnet_mirror(p, xyz, nrm, idx, masks, widx.long())
        (o * w.to(dt)).sum().backward()
        grads[tag] = ({n: v.grad for n, v in p.items()}, o.detach())
    o64 = grads["fp64"][1]
    err = (out.detach().double() - o64).abs()
    assert bool((err <= 1e-4 * o64.abs() + 1e-5 * float(o64.abs().max())).all()), ("forward against the mirror", float(err.max()))
    failed = []
    print(f"\nPPFNet(emb_dims={emb_dims}, num_neighbors={K}) N {N}: relative to max |fp64 gradient|")
    print(f"  {'tensor':<20} {'HIP':>10} {'fp32 torch':>11} {'bar':>10}")
    for n in got:
        want = grads["fp64"][0][n]
        scale = float(want.abs().max())
        e_hip = float((got[n].double() - want).abs().max()) / scale
        e_32 = float((grads["fp32"][0][n].double() - want).abs().max()) / scale
        bar = tf.TIER if e_32 <= tf.TIER else 2 * e_32
        print(f"  {n:<20} {e_hip:>10.2e} {e_32:>11.2e} {bar:>10.1e}")
        if not e_hip <= bar:
            failed.append((n, e_hip, e_32, bar))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------------------------
def test_rpmnet_trains_through_the_route():
    _lib, _fused, ppfnet = _mods()
    cpu_net, t, s, igt = tf.plumbing_case()
    n64, dnet = copy.deepcopy(cpu_net).double(), copy.deepcopy(cpu_net).to(DEV)
    g64 = tf.plumbing_gradients(n64, t.double(), s.double(), igt.double())
    td, sd, igtd = t.to(DEV), s.to(DEV), igt.to(DEV)
    with _log() as log:
        res = dnet(td, sd, 2)
        n_fwd = len(log)
        tf.bench_loss(res, igtd).backward()
    hip = {n: p.grad.detach().clone() for n, p in dnet.named_parameters()}
    assert log[:n_fwd].count("l3d_ppf_group") == 3, "the template's features once, the source's per iteration"
    assert all(name in log for name in NEW) and "l3d_sinkhorn_slack" not in log and "l3d_rigid_transform_weighted" not in log
    assert set(res) == {"est_R", "est_t", "est_T", "transformed_source", "perm_matrices_init", "perm_matrices", "weighted_template",
                        "beta", "alpha", "transforms"}
    assert dnet.feat_template.shape == (2, 64, 96) and dnet.feat_source.shape == (2, 50, 96) and dnet.feat_template.requires_grad
    assert torch.equal(dnet.feat_template.detach(), dnet.feat_extractor(td[:, :, :3], td[:, :, 3:]).detach())
    _fused.TRAIN_HIP = False
    try:
        with _log() as log_seq:
            seq = tf.plumbing_gradients(dnet, td, sd, igtd)
    finally:
        _fused.TRAIN_HIP = True
    assert not any(name in log_seq for name in NEW + ("l3d_gn_conv",))
    failed = []
    print("\nRPMNet, 2 iterations: max |gradient - fp64| / max |fp64|")
    print(f"  {'tensor':<34} {'HIP':>10} {'device ops':>11} {'HIP - ops':>10} {'gap':>10} {'bar':>10}")
    for n, want in g64.items():
        scale = float(want.abs().max())
        gap = tf.PLUMBING_GAPS[n]                          # the op sequence's own fp32-to-fp64 gap, measured on the CPU (the fixture)
        bar = max(tf.GAP_FACTOR * gap, tf.TIER)
        e_hip = float((hip[n].cpu().double() - want).abs().max()) / scale
        e_seq = float((seq[n].cpu().double() - want).abs().max()) / scale
        between = float((hip[n].double() - seq[n].double()).abs().max()) / scale
        print(f"  {n:<34} {e_hip:>10.2e} {e_seq:>11.2e} {between:>10.2e} {gap:>10.2e} {bar:>10.1e}")
        if not (e_hip <= bar and between <= bar):
            failed.append((n, e_hip, e_seq, between, gap, bar))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------------------------
def _grads(net, xyz, nrm):
    net.zero_grad(set_to_none=True)
    out = net(xyz.clone(), nrm.clone())
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(out.device)
    (out * w).sum().backward()
    return out.detach(), [None if p.grad is None else p.grad.clone() for p in net.parameters()]


def test_route_and_state(monkeypatch):
    _lib, _fused, ppfnet = _mods()
    cpu_net, xyz, nrm = tf.ppfnet_case(31, 32, 8, 70)
    net = cpu_net.to(DEV)
    xyz, nrm = xyz.to(DEV), nrm.to(DEV)
    calls = []
    real = torch.nn.functional.group_norm
    monkeypatch.setattr(torch.nn.functional, "group_norm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with _log() as log:
        out1, g1 = _grads(net, xyz, nrm)
    assert all(name in log for name in NEW) and not calls
    assert log.count("l3d_gn_conv") == 6 + 5 and log.count("l3d_wgrad") == 6 and log.count("l3d_gn_backward_apply") == 5
    with _log() as log, torch.no_grad():
        fused = net.fused_features(xyz, nrm)
        assert not net.trains_on_hip(xyz, nrm)
        net(xyz, nrm)                                                  # the op sequence: no kernel of either GroupNorm route
    assert log[:13] == ["l3d_query_ball_point", "l3d_ppf_group"] + ["l3d_gn_conv", "l3d_gn_affine"] * 5 + ["l3d_gn_conv"]
    assert not any(name.startswith("l3d_gn_") or name == "l3d_ppf_group" for name in log[13:]) and len(calls) == 5
    assert torch.equal(fused, out1), "the differentiable forward is fused_features' launch list"
    out2, g2 = _grads(net, xyz, nrm)                                   # fresh inputs, stale workspaces: the same bits
    assert torch.equal(out1, out2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    frozen = [p for n, p in net.named_parameters() if n.startswith("prepool")]
    for p in frozen:                                                   # only the post-pool stack learns: the rest gets no gradient
        p.requires_grad_(False)
    with _log() as log:
        _, g3 = _grads(net, xyz, nrm)
    assert all(g is None for g in g3[:len(frozen)]) and log.count("l3d_wgrad") == 3
    assert log.count("l3d_gn_backward_apply") == 2, "the backward stops at the lowest layer that learns"
    assert all(torch.equal(a, b) for a, b in zip(g3[len(frozen):], g1[len(frozen):]))
    for p in frozen:
        p.requires_grad_(True)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    _grads(net, xyz, nrm)
    opt.step()
    out3 = net(xyz, nrm).detach()
    with torch.no_grad():
        assert not torch.equal(out3, out1) and torch.equal(out3, net.fused_features(xyz, nrm))


def test_peak_allocation_is_below_the_op_sequence():
    _lib, _fused, ppfnet = _mods()
    cpu_net, xyz, nrm = tf.ppfnet_case(41, 96, 64, 256)
    net, xyz, nrm = cpu_net.to(DEV), xyz.to(DEV), nrm.to(DEV)
    peaks = {}
    for hip in (True, False, True):
        _fused.TRAIN_HIP = hip
        try:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            _grads(net, xyz, nrm)
            torch.cuda.synchronize()
            peaks[hip] = torch.cuda.max_memory_allocated() - base
        finally:
            _fused.TRAIN_HIP = True
    print(f"\nPPFNet forward + backward at B 2, N 256, K 64: peak {peaks[True] / 2 ** 20:.1f} MiB on the HIP route, "
          f"{peaks[False] / 2 ** 20:.1f} MiB on the op sequence")
    assert peaks[True] < peaks[False]


# ------------------------------------------------------------------------------------------------------------------------------
_SCRATCH = {
    "l3d_gn_backward_stats": {"workspace": mc.Spec("scratch", "`workspace` (SCRATCH of l3d_gn_backward_workspace_bytes(B, C, P) bytes",
                                                   size=("l3d_gn_backward_workspace_bytes", lambda v: (v["B"], v["C"], v["P"]), 1))},
}


def _contract(name, build):
    _lib = _mods()[0]
    return mc.check(name, build, proto=_lib.EXT_PROTOTYPES[name], contract=_SCRATCH)


def _rand(seed, *shape):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)).to(DEV) * 2 - 1


@pytest.mark.parametrize("B,C,P,K", [(2, 16, 150, 0), (2, 48, 8200, 0), (1, 16, 68, 0), (2, 16, 210, 3), (2, 16, 16392, 2), (1, 48, 320, 64),
                                     (2, 16, 272, 4)])
def test_memory_contract(B, C, P, K):
    """every new entry point: guards, two fills, const inputs unchanged, the workspace by its size function.  Tails in P, rows of two
    chunks, pooled with N' a multiple of 4 (the 16-byte route) and not"""
    _lib = _mods()[0]
    G, NP = tf.GROUPS, (P // K if K else P)
    y, a, s, gamma = _rand(1, B, C, P), _rand(2, B, C), _rand(3, B, C), _rand(4, C)
    du = _rand(5, B, C, NP)
    moments = torch.stack([_rand(6, B, C).double() * P, (_rand(7, B, C).double().abs() + 1.5) * P], -1).contiguous()
    out = _contract("l3d_gn_mean_rstd", lambda ar: [moments, B, C, G, P, tf.EPS, ar.out(torch.float64, B, G, 2)])
    stat = out["stat"].clone()
    assert bool(torch.isfinite(stat).all())
    _contract("l3d_gn_relu", lambda ar: [y, a, s, B, C, P, ar.f32(B, C, P)])
    widx = None
    if K:
        widx = _contract("l3d_gn_pool_winner", lambda ar: [y, a, B, C, K, NP, ar.out(torch.uint8, B, C, NP)])["widx"].clone()
        assert int(widx.max()) < K
    ws_bytes = _lib.lib().l3d_gn_backward_workspace_bytes(B, C, P)
    part = _contract("l3d_gn_backward_stats", lambda ar: [du, widx, K, y, a, s, stat, B, C, G, P, ar.out(torch.float64, B, C, 2),
                                                          ar.bytes(ws_bytes)])["part"].clone()
    for want_g, want_b in ((True, True), (False, True), (False, False)):
        m = _contract("l3d_gn_backward_reduce", lambda ar: [part, gamma, B, C, G, P, ar.out(torch.float64, B, G, 2),
                                                            ar.f32(C) if want_g else None, ar.f32(C) if want_b else None])["m"].clone()
    dz = _contract("l3d_gn_backward_apply", lambda ar: [du, widx, K, y, a, s, stat, gamma, m, B, C, G, P, ar.f32(B, C, P)])["dz"]
    want = tf.gn_relu_backward64(du, y, a, s, stat[..., 0], stat[..., 1], gamma, G, K, None if widx is None else widx.long())[0]
    _rounded_once(dz, want, ("dz", B, C, P, K))


# ------------------------------------------------------------------------------------------------------------------------------
# PPFNet._Train as tests/test_gpu_views_backward.py holds every autograd.Function of the package: gradients that arrive as views and
# inputs that are views, bit for bit and launch for launch against contiguous clones.  Every tensor any launch receives is contiguous
# (layout_audit sees the entry points of include/*.h; the wrapper below holds those of include/ext/ to the same rule).
def _views_case(monkeypatch):
    import layout_audit
    from view_cases import assert_identical, float_views, grad_views, logged, whole_storage
    _lib, _, ppfnet = _mods()
    layout_audit.install(monkeypatch)
    inner = ppfnet.call

    def contiguous_only(name, *args, **kw):
        for i, a in enumerate(args):
            assert not isinstance(a, torch.Tensor) or a.is_contiguous(), (name, i, tuple(a.shape), a.stride())
        return inner(name, *args, **kw)
    monkeypatch.setattr(ppfnet, "call", contiguous_only)
    cpu_net, xyz, nrm = tf.ppfnet_case(51, 32, 8, 70)
    net = cpu_net.to(DEV)
    params = net._parameters_in_order()

    def run(x, n, g):
        out = net._Train.apply(net, x, n, *params)
        return out, torch.autograd.grad([out], params, [g])
    return net, xyz.to(DEV), nrm.to(DEV), run, (assert_identical, float_views, grad_views, logged, whole_storage)


def test_train_function_on_view_gradients(monkeypatch):
    net, xyz, nrm, run, (assert_identical, _, grad_views, logged, whole_storage) = _views_case(monkeypatch)
    shape = (2, net.postpool[6].out_channels, 70)
    views = dict(grad_views(shape, seed=50))
    assert set(views) == {"transposed", "stride2", "expand"}
    for kind, g in views.items():
        (out, want), log = logged(run, xyz, nrm, g.contiguous())
        assert tuple(out.shape) == shape and "l3d_gn_backward_apply" in log and "l3d_wgrad" in log
        before = whole_storage(g).clone()
        (out_v, got), vlog = logged(run, xyz, nrm, g)
        assert vlog == log, (kind, vlog, log)
        assert_identical((out_v, got), (out, want), f"gradient as a {kind} view {g.stride()}")
        assert torch.equal(whole_storage(g), before), f"{kind}: the gradient's buffer was written to"


def test_train_function_on_view_inputs(monkeypatch):
    net, xyz, nrm, run, (assert_identical, float_views, grad_views, logged, whole_storage) = _views_case(monkeypatch)
    g = dict(grad_views((2, net.postpool[6].out_channels, 70), seed=70))["stride2"]
    ran = 0
    for (kind, xv), (_, nv) in zip(float_views(xyz), float_views(nrm)):
        assert not xv.is_contiguous() and not nv.is_contiguous()
        xd, nd = xv.clone(memory_format=torch.contiguous_format), nv.clone(memory_format=torch.contiguous_format)
        want, log = logged(run, xd, nd, g)
        again, log2 = logged(run, xd, nd, g)
        assert log2 == log
        assert_identical(again, want, f"{kind}: two runs on the same contiguous inputs")
        before = [whole_storage(v).clone() for v in (xv, nv)]
        got, vlog = logged(run, xv, nv, g)
        assert vlog == log, (kind, vlog, log)
        assert_identical(got, want, f"inputs as {kind} views {xv.stride()}")
        assert all(torch.equal(whole_storage(v), b) for v, b in zip((xv, nv), before)), f"{kind}: an input's buffer was written to"
        ran += 1
    assert ran == 4
