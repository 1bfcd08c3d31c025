"""RPMNet / PPFNet on the GPU: the kernels of rpmnet.hip and the fused route against the fixture from the reference
(tests/golden/rpmnet_seeded.npz, make_golden_rpmnet.py; read through golden/rpmnet_fixture.py).

The bar everywhere is GAP_FACTOR = 4: the error against the reference's fp64 is at most 4 x the reference's own fp32-to-fp64 gap of
that quantity, the gap taken as the maximum over the fixture's cases of one kind.  Where the fixture stores a large tensor only
as samples, the whole fp64 tensor is this package's op sequence in fp64 on the CPU, which tests/test_rpmnet_cpu.py holds to 1e-9
against everything stored.  Beside every fused number the op-sequence route on the device is held to the same bar.
The tests named `..._edge_shapes` run the kernels at shapes the fixture does not have (several clouds per batch, tile edges, P = 1,
more blocks than partial slots); their gap is torch's own fp32 against fp64 on the same operands, computed in the test.

Measured ratios (error / gap) are printed by every test; the last run's are in LABLOG.md R19.1."""
import numpy as np
import pytest
import torch

import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import memory_contract as mc     # noqa: E402
import rpmnet_fixture as rf      # noqa: E402

pytestmark = pytest.mark.gpu
GAP_FACTOR = 4.0
DEV = "cuda"


def _mods():
    from learning3d_amd import _lib
    from learning3d_amd.models import ppfnet, rpmnet
    return _lib, ppfnet, rpmnet


def _clouds(seed, B=2, N=160, J=128, normals=True):
    """half the points in a cube of side 0.35 (their balls of radius 0.3 overflow 16 neighbours), half in [-1,1]^3 (below 16, many
    alone); the source is the first J points rotated about z and shifted"""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.cat([torch.rand((B, N // 2, 3), generator=g) * 0.35 - 0.175, torch.rand((B, N - N // 2, 3), generator=g) * 2 - 1], 1)
    xyz = xyz[:, torch.randperm(N, generator=g)]
    nrm = torch.randn((B, N, 3), generator=g)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    c, s = float(np.cos(0.5)), float(np.sin(0.5))
    R = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    src = xyz[:, :J] @ R.T + torch.tensor([0.1, -0.05, 0.08])
    if not normals:
        return xyz.contiguous(), src.contiguous()
    return torch.cat([xyz, nrm], -1).contiguous(), torch.cat([src, nrm[:, :J] @ R.T], -1).contiguous()


def _err(got, want64):
    return float((got.detach().cpu().double() - want64).abs().max())


def _held(pairs, what):
    """pairs: (error, gap) per case of one kind"""
    gap = max(g for _, g in pairs)
    worst = max(e for e, _ in pairs)
    print(f"{what}: error {worst:.2e}, gap {gap:.2e}, ratio {worst / gap if gap else float('inf'):.2f}")
    assert gap > 0 and worst <= GAP_FACTOR * gap, (what, worst, gap)


def test_ppf_group_edge_shapes():
    _lib, ppfnet, _ = _mods()
    pairs = []
    for normals in (True, False):
        t, _ = _clouds(11, normals=normals)
        xyz = t[:, :, :3].contiguous()
        nrm = t[:, :, 3:].contiguous() if normals else torch.zeros_like(xyz)
        B, N, _ = xyz.shape
        for K in (16, 64, 5):
            itself = torch.arange(N)[None].repeat(B, 1)
            idx = ppfnet._query_ball_point(0.3, K, xyz.double(), xyz.double(), itself)
            assert torch.equal(idx, ppfnet._query_ball_point(0.3, K, xyz, xyz, itself))
            f32 = ppfnet._sample_and_group_multi(0.3, K, xyz, nrm)
            f64 = ppfnet._sample_and_group_multi(0.3, K, xyz.double(), nrm.double())
            got = ppfnet.ppf_group(xyz.to(DEV), nrm.to(DEV) if normals else None, idx.to(DEV)).cpu()      # [B,10,K,N]
            got = got.permute(0, 3, 2, 1)                                                                  # [B,N,K,10]
            assert torch.equal(got[..., :3], xyz[:, :, None, :].expand(-1, -1, K, -1))
            want = torch.cat([f64["dxyz"], f64["ppf"]], -1)
            have32 = torch.cat([f32["dxyz"], f32["ppf"]], -1)
            pairs.append((_err(got[..., 3:], want), _err(have32, want)))
            pad = idx == torch.arange(N)[None, :, None]
            assert pad.any() and (~pad).any()
            assert float(got[..., 3:][pad].abs().max()) == 0.0                  # padded slots: exact zeros, -0 dot products included
    _held(pairs, "ppf_group")


def _conv_case(ppfnet, seed, B, Cin, Cout, K, NP, affine, bias=True):
    g = torch.Generator().manual_seed(seed)
    P = K * NP
    x = torch.randn((B, Cin, P), generator=g)
    w = (torch.rand((Cout, Cin), generator=g) * 2 - 1) / np.sqrt(Cin)
    bv = torch.rand((Cout,), generator=g) - 0.5 if bias else None
    a = torch.randn((B, Cin), generator=g) if affine else None               # both signs
    s = torch.randn((B, Cin), generator=g) * 0.3 if affine else None

    def ref(dt):
        u = x.to(dt)
        if affine:
            u = torch.relu(a.to(dt)[:, :, None] * u + s.to(dt)[:, :, None])
        y = torch.matmul(w.to(dt), u)
        return y + bv.to(dt)[None, :, None] if bias else y
    return x, w, bv, a, s, ref(torch.float32), ref(torch.float64)


def test_gn_conv_edge_shapes():
    """Cin 10 (not a multiple of 4), N' 160 (no multiple of the 64-position block), Cin 96 / 192 across LDS chunks, Cout 16 and 256,
    P = 1, more blocks than partial slots (N' 5000)"""
    _lib, ppfnet, _ = _mods()
    pairs, pool_pairs = [], []
    for i, (B, Cin, Cout, K, NP, affine, bias) in enumerate(((2, 10, 96, 16, 160, False, True), (2, 96, 96, 16, 160, True, True),
                                                             (2, 96, 192, 16, 160, True, True), (1, 192, 256, 3, 70, True, False),
                                                             (1, 70, 16, 1, 1, True, True), (1, 5, 32, 2, 5000, False, True))):
        x, w, bv, a, s, y32, y64 = _conv_case(ppfnet, 100 + i, B, Cin, Cout, K, NP, affine, bias)
        dv = lambda t: None if t is None else t.to(DEV)           # noqa: E731
        y, _, _, mom = ppfnet.gn_conv(dv(x), dv(a), dv(s), dv(w), dv(bv))
        gap = _err(y32, y64)
        pairs.append((_err(y, y64), gap))
        yk = y.cpu().double()
        want_m = torch.stack([yk.sum(2), (yk * yk).sum(2)], -1)

        def moments_ok(m):          # 1e-12 of the fp64 sums of the kernel's own y (of their magnitude: a sum can cancel to nothing)
            return float((m.cpu() - want_m).abs().max()) <= 1e-12 * float(want_m.abs().max())
        assert moments_ok(mom)
        yp, ymax, ymin, momp = ppfnet.gn_conv(dv(x), dv(a), dv(s), dv(w), dv(bv), pool=K, want_y=True)
        assert torch.equal(yp, y) and moments_ok(momp)        # another order of the same sums
        y64k = y64.view(B, Cout, K, NP)
        pool_pairs.append((max(_err(ymax, y64k.amax(2)), _err(ymin, y64k.amin(2))), gap))
        _, ymax2, ymin2, mom2 = ppfnet.gn_conv(dv(x), dv(a), dv(s), dv(w), dv(bv), pool=K, want_y=False)     # y = NULL
        assert torch.equal(ymax2, ymax) and torch.equal(ymin2, ymin) and torch.equal(mom2, momp)
    _held(pairs, "gn_conv y")
    _held(pool_pairs, "gn_conv ymax / ymin")


def test_gn_affine_is_group_norm():
    _lib, ppfnet, _ = _mods()
    g = torch.Generator().manual_seed(5)
    pairs = []
    for B, C, P in ((2, 96, 2560), (1, 192, 7), (3, 16, 1)):
        y = torch.randn((B, C, P), generator=g) * 2 + 0.7
        norm = torch.nn.GroupNorm(8, C)
        with torch.no_grad():
            norm.weight.copy_(torch.rand((C,), generator=g) * 2 - 1)
            norm.bias.copy_(torch.rand((C,), generator=g) - 0.5)
            want = torch.nn.functional.group_norm(y.double(), 8, norm.weight.double(), norm.bias.double(), norm.eps)
            have32 = norm(y)
        yd = y.double()
        mom = torch.stack([yd.sum(2), (yd * yd).sum(2)], -1).to(DEV)
        a, s = ppfnet.gn_affine(mom, norm.to(DEV), P)
        got = a.cpu()[:, :, None] * y + s.cpu()[:, :, None]                     # fp32 on the CPU, two roundings
        pairs.append((_err(got, want), _err(have32, want)))
    _held(pairs, "gn_affine")


SK_SHAPES = ((50, 70), (130, 67), (1, 1), (1, 64), (65, 1))


def test_sinkhorn_slack_edge_shapes():
    _lib, _, rpmnet = _mods()
    g = torch.Generator().manual_seed(9)
    for kind, cases in (("N(0,9)", [(J, K, 3.0) for J, K in SK_SHAPES]), ("+-200", [(50, 70, None), (130, 67, None)])):
        logs, perms, rows, wts = [], [], [], []
        for J, K, scale in cases:
            x = torch.randn((2, J, K), generator=g) * 3.0
            if scale is None:
                x = x / x.abs().max() * 200.0
            ref = torch.rand((2, K, 3), generator=g) * 2 - 1
            old = rpmnet.FUSED
            rpmnet.FUSED = False
            try:
                l32, l64 = rpmnet.sinkhorn(x, 5), rpmnet.sinkhorn(x.double(), 5)
            finally:
                rpmnet.FUSED = old
            p32, p64 = l32.exp(), l64.exp()
            w32 = p32 @ ref / (p32.sum(2, keepdim=True) + 1e-5)
            w64 = p64 @ ref.double() / (p64.sum(2, keepdim=True) + 1e-5)
            lp, pm, rs, wt = rpmnet.sinkhorn_slack(x.to(DEV), 5, xyz_ref=ref.to(DEV), want_perm=True)
            for t in (lp, pm, rs, wt):
                assert bool(torch.isfinite(t).all())
            logs.append((_err(lp, l64), _err(l32, l64)))
            perms.append((_err(pm, p64), _err(p32, p64)))
            rows.append((_err(rs, p64.sum(2)), _err(p32.sum(2), p64.sum(2))))
            wts.append((_err(wt, w64), _err(w32, w64)))
            assert torch.equal(rpmnet.sinkhorn(x.to(DEV), 5), lp)                        # the public function takes the kernel
            lp0, pm0, _, _ = rpmnet.sinkhorn_slack(x.to(DEV), 0, want_perm=True)
            assert torch.equal(lp0.cpu(), x)                                             # n_iters = 0: the input's bits
            only = rpmnet.sinkhorn_slack(x.to(DEV), 5, xyz_ref=ref.to(DEV), want_log=False)   # some outputs NULL
            assert only[0] is None and only[1] is None and torch.equal(only[2], rs) and torch.equal(only[3], wt)
        _held(logs, f"sinkhorn {kind} log_perm")
        _held(perms, f"sinkhorn {kind} perm")
        _held(rows, f"sinkhorn {kind} rowsum")
        _held(wts, f"sinkhorn {kind} weighted")


def test_rigid_transform_weighted_edge_shapes():
    _lib, _, rpmnet = _mods()
    g = torch.Generator().manual_seed(21)
    B = 3
    cases = []
    a = torch.rand((B, 128, 3), generator=g) * 2 - 1
    q = torch.linalg.qr(torch.randn((B, 3, 3), generator=g))[0]
    q = q * torch.det(q)[:, None, None]                                                 # proper rotations
    cases.append((a, a @ q + 0.05 * torch.randn((B, 128, 3), generator=g) + 0.2, torch.rand((B, 128), generator=g)))
    a3 = torch.rand((B, 3, 3), generator=g) * 2 - 1
    cases.append((a3, a3 @ q + 0.2, torch.rand((B, 3), generator=g) + 0.5))
    ar = torch.rand((B, 32, 3), generator=g) * 2 - 1
    mirror = torch.diag(torch.tensor([1.0, 1.0, -1.0]))
    cases.append((ar, ar @ mirror + 0.01 * torch.randn((B, 32, 3), generator=g) + 0.3, torch.rand((B, 32), generator=g) + 0.5))
    ca, cb = ar - ar.mean(1, keepdim=True), (ar @ mirror) - (ar @ mirror).mean(1, keepdim=True)
    assert bool((torch.det(ca.transpose(1, 2) @ cb) < 0).all())                          # the determinant branch decides
    pairs = []
    for a, b, w in cases:
        t32 = rpmnet.compute_rigid_transform(a, b, w)
        t64 = rpmnet.compute_rigid_transform(a.double(), b.double(), w.double())
        T = rpmnet.rigid_transform_weighted(a.to(DEV), b.to(DEV), w.to(DEV)).cpu()
        pairs.append((_err(T, t64), _err(t32, t64)))
        R = T[:, :, :3].double()
        assert float((R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-6
        assert float((torch.det(R) - 1).abs().max()) <= 1e-6
    _held(pairs, "rigid_transform_weighted")


# ------------------------------------------------------------------------------------------------------------------------------
# against the fixture
def _ratio(what, err, gap):
    print(f"{what}: error {err:.2e}, gap {gap:.2e}, ratio {err / gap:.2f}")
    assert err <= GAP_FACTOR * gap, (what, err, gap)


def _grouping64(name):
    fx = rf.load()
    _, ppfnet, _ = _mods()
    t = torch.from_numpy(fx["template"])
    xyz = t[:, :, :3].contiguous()
    nrm = t[:, :, 3:].contiguous() if name == "a" else None
    idx = rf.stored(f"group_{name}_idx").long()
    f64 = ppfnet._sample_and_group_multi(float(fx["radius"]), 16, xyz.double(), (nrm if nrm is not None else torch.zeros_like(xyz)).double())
    return xyz, nrm, idx, f64


def test_ppf_group_on_the_fixture():
    fx = rf.load()
    _, ppfnet, _ = _mods()
    gaps = {q: max(float(fx[f"group_{n}_{q}_gap"]) for n in "ac") for q in ("dxyz", "ppf")}
    for name in "ac":
        xyz, nrm, idx, f64 = _grouping64(name)
        got = ppfnet.ppf_group(xyz.to(DEV), None if nrm is None else nrm.to(DEV), idx.to(DEV)).cpu().permute(0, 3, 2, 1)
        assert torch.equal(got[..., :3], xyz[:, :, None, :].expand(-1, -1, 16, -1))
        _ratio(f"ppf_group {name} dxyz", _err(got[..., 3:6], f64["dxyz"]), gaps["dxyz"])
        _ratio(f"ppf_group {name} ppf", _err(got[..., 6:], f64["ppf"]), gaps["ppf"])
        pad = idx == torch.arange(xyz.shape[1])[None, :, None]
        assert pad.any() and float(got[..., 3:][pad].abs().max()) == 0.0            # the fixture's gap there is exactly 0: equality


def test_gn_conv_on_the_prepool_layers():
    """case a's three pre-pool layers through the kernels: Cin 10 and N' 160, both pool modes, ymax / ymin against the fp64 layer
    output, GroupNorm scales of both signs (the ymin branch), moments against fp64 sums of the kernel's own y"""
    fx = rf.load()
    _, ppfnet, _ = _mods()
    xyz, nrm, idx, f64 = _grouping64("a")
    B, N, K = xyz.shape[0], xyz.shape[1], 16
    net64 = rf.build("a").double().feat_extractor
    net = rf.build("a").feat_extractor.to(DEV)
    x64 = torch.cat([f64["xyz"][:, :, None, :].expand(-1, -1, K, -1), f64["dxyz"], f64["ppf"]], -1).permute(0, 3, 2, 1)
    layers64, h = [], x64
    with torch.no_grad():
        for i, m in enumerate(net64.prepool):
            h = m(h)
            if i in (0, 3, 6):
                layers64.append(h)
    x = x64.float().reshape(B, 10, K * N).contiguous().to(DEV)
    a = s = None
    for li, ci in enumerate((0, 3, 6)):
        conv, norm = net.prepool[ci], net.prepool[ci + 1]
        want = layers64[li].reshape(B, -1, K * N)
        gap = float(fx[f"layer{li}_gap"])
        y, _, _, mom = ppfnet.gn_conv(x, a, s, conv.weight, conv.bias)
        _ratio(f"gn_conv layer {li} y", _err(y, want), gap)
        yk = y.cpu().double()
        want_m = torch.stack([yk.sum(2), (yk * yk).sum(2)], -1)
        assert float((mom.cpu() - want_m).abs().max()) <= 1e-12 * float(want_m.abs().max())
        yp, ymax, ymin, momp = ppfnet.gn_conv(x, a, s, conv.weight, conv.bias, pool=K, want_y=(li != 2))
        w4 = want.view(B, -1, K, N)
        _ratio(f"gn_conv layer {li} ymax / ymin", max(_err(ymax, w4.amax(2)), _err(ymin, w4.amin(2))), gap)
        assert (yp is None) == (li == 2) and float((momp.cpu() - want_m).abs().max()) <= 1e-12 * float(want_m.abs().max())
        a, s = ppfnet.gn_affine(mom, norm, K * N)
        assert bool((a < 0).any()) and bool((a > 0).any())
        # the pooled activation from the extremes is the maximum over k of the GroupNorm + ReLU of the fp64 layer
        act64 = torch.relu(torch.nn.functional.group_norm(layers64[li], 8, net64.prepool[ci + 1].weight, net64.prepool[ci + 1].bias,
                                                          norm.eps)).amax(2)
        pooled = torch.relu(a[:, :, None] * torch.where((a >= 0)[:, :, None], ymax, ymin) + s[:, :, None])
        print(f"layer {li}: pooled activation error {_err(pooled, act64):.2e}")
        x = y


def test_sinkhorn_slack_on_the_fixture():
    fx = rf.load()
    _, _, rpmnet = _mods()
    names = [str(n) for n in fx["sinkhorn_cases"]]
    for kind in ([n for n in names if n != "wide"], ["wide"]):
        gap_log = max(float(fx[f"sk_{n}_gap"]) for n in kind)
        gap_perm = max(float(fx[f"sk_{n}_perm_gap"]) for n in kind)
        rows, wts = [], []
        for n in kind:
            x, ref, l64 = rf.stored(f"sk_{n}_in"), rf.stored(f"sk_{n}_ref"), rf.stored(f"sk_{n}_64")
            lp, pm, rs, wt = rpmnet.sinkhorn_slack(x.to(DEV), 5, xyz_ref=ref.to(DEV), want_perm=True)
            assert all(bool(torch.isfinite(t).all()) for t in (lp, pm, rs, wt))
            _ratio(f"sinkhorn {n} log_perm", _err(lp, l64), gap_log)
            _ratio(f"sinkhorn {n} perm", _err(pm, l64.exp()), gap_perm)
            # row sums and weighted points: the gap of the same torch ops in fp32 on the reference's own fp32 result
            rpmnet.FUSED = False
            try:
                p32 = rpmnet.sinkhorn(x, 5).exp()
            finally:
                rpmnet.FUSED = True
            p64 = l64.exp()
            w64 = p64 @ ref.double() / (p64.sum(2, keepdim=True) + 1e-5)
            rows.append((_err(rs, p64.sum(2)), _err(p32.sum(2), p64.sum(2))))
            wts.append((_err(wt, w64), _err(p32 @ ref / (p32.sum(2, keepdim=True) + 1e-5), w64)))
            assert torch.equal(rpmnet.sinkhorn_slack(x.to(DEV), 0)[0].cpu(), x)          # n_iters = 0: the input's bits
        _held(rows, f"sinkhorn {kind[0]}.. rowsum")
        _held(wts, f"sinkhorn {kind[0]}.. weighted")


def test_rigid_transform_weighted_on_the_fixture():
    fx = rf.load()
    _, _, rpmnet = _mods()
    names = [str(n) for n in fx["kabsch_cases"]]
    gap = max(float(fx[f"kab_{n}_gap"]) for n in names)
    for n in names:
        a, b, w, want = (rf.stored(f"kab_{n}_{q}") for q in ("a", "b", "w", "64"))
        T = rpmnet.rigid_transform_weighted(a.to(DEV), b.to(DEV), w.to(DEV)).cpu()
        _ratio(f"rigid_transform_weighted {n} (M {a.shape[1]})", _err(T, want), gap)
        R = T[:, :, :3].double()
        assert float((R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-6
        assert float((torch.det(R) - 1).abs().max()) <= 1e-6


def _routes(net, t, s, iters, fused=True):
    _lib, _, rpmnet = _mods()
    rpmnet.FUSED = fused
    _lib.LAUNCH_LOG = log = []
    try:
        with torch.no_grad():
            res = net(t, s, iters)
    finally:
        rpmnet.FUSED = True
        _lib.LAUNCH_LOG = None
    return res, log


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_model_fused_and_op_sequence_on_the_fixture(name):
    K, iters, _ = rf.cases()[name]
    t, s = (v.to(DEV) for v in rf.inputs(name))
    net = rf.build(name).to(DEV)
    fused, log = _routes(net, t, s, iters)
    assert log.count("l3d_ppf_group") == iters + 1, log                  # the template's features once
    assert log.count("l3d_sinkhorn_slack") == iters and log.count("l3d_rigid_transform_weighted") == iters
    assert isinstance(fused["beta"], np.ndarray) and fused["beta"].shape == (iters, t.shape[0])
    seq, log = _routes(net, t, s, iters, fused=False)
    assert "l3d_ppf_group" not in log and "l3d_sinkhorn_slack" not in log and "l3d_gn_conv" not in log
    assert set(fused) == set(seq) == set(rf.reference64(name))
    if name == "a":
        pm = fused["perm_matrices"][-1]
        assert float(pm.max()) >= 0.5 and float(pm.sum(2).min()) <= 0.85     # the fixture's regime, on the fused result itself
    e_fused, e_seq = rf.model_errors(fused, name), rf.model_errors(seq, name)
    for q in rf.QUANTITIES:
        gap = rf.pooled_gap(q)
        _ratio(f"case {name} op sequence {q}", e_seq[q], gap)
        _ratio(f"case {name} fused {q}", e_fused[q], gap)


def test_forward_fused_replays_from_one_graph():
    """_forward_fused captured into one graph on one stream and replayed twice gives the eager bits: no host read, no stale state"""
    name = "a"
    K, iters, _ = rf.cases()[name]
    t, s = (v.to(DEV) for v in rf.inputs(name))
    net = rf.build(name).to(DEV)
    flat = lambda r: [r["est_T"], r["beta"], r["alpha"], *r["transforms"], *r["perm_matrices"], *r["perm_matrices_init"],       # noqa: E731
                      *r["weighted_template"], r["transformed_source"]]
    with torch.no_grad():
        eager = [v.clone() for v in flat(net._forward_fused(t, s, iters))]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            net._forward_fused(t, s, iters)                              # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = flat(net._forward_fused(t, s, iters))
        for replay in range(2):
            for v in out:
                v.fill_(7.0)                                             # stale values must not survive a replay
            graph.replay()
            torch.cuda.synchronize()
            for i, (a, b) in enumerate(zip(out, eager)):
                assert torch.equal(a, b), (replay, i)


def test_fallbacks_take_the_op_sequence():
    """requires_grad inputs, add_slack=False, a width the kernel refuses and a feature subset take the op sequence (launch log);
    where the fused route exists for the same model the two agree within twice the bar (each is within the bar of fp64), elsewhere
    the device op sequence is held to 4 x the CPU fp32 op sequence's gap against the CPU fp64 op sequence of the same model"""
    import copy
    _lib, ppfnet, rpmnet = _mods()
    t, s = rf.inputs("a")
    td, sd = t.to(DEV), s.to(DEV)
    net = rf.build("a").to(DEV)
    fused, log = _routes(net, td, sd, 1)
    assert "l3d_ppf_group" in log
    _lib.LAUNCH_LOG = log = []
    try:
        with torch.enable_grad():
            res = net(td.clone().requires_grad_(True), sd, 1)
    finally:
        _lib.LAUNCH_LOG = None
    assert "l3d_ppf_group" not in log and "l3d_sinkhorn_slack" not in log and res["est_T"].requires_grad
    for q in ("est_T", "perm_matrices", "weighted_template"):
        a, b = (r[q][0] if isinstance(r[q], list) else r[q] for r in (res, fused))
        assert float((a.detach() - b).abs().max()) <= 2 * GAP_FACTOR * rf.pooled_gap(q), q
    variants = {"add_slack=False": (rf.build("a"), dict(add_slack=False)), "emb_dims=40": (rf.build("a", emb_dims=40), {}),
                "features ppf+dxyz": (rf.build("a", features=["ppf", "dxyz"]), {})}
    for what, (cpu_net, attrs) in variants.items():
        for k, v in attrs.items():
            setattr(cpu_net, k, v)
        with torch.no_grad():
            r32 = cpu_net(t, s, 1)
            r64 = copy.deepcopy(cpu_net).double()(t.double(), s.double(), 1)
        res, log = _routes(copy.deepcopy(cpu_net).to(DEV), td, sd, 1)
        # (the public sinkhorn still takes its kernel on device tensors, as it does for any caller: that is not the fused route)
        assert "l3d_ppf_group" not in log and "l3d_gn_conv" not in log and "l3d_rigid_transform_weighted" not in log, what
        assert ("l3d_sinkhorn_slack" in log) == (what != "add_slack=False"), what
        pairs = [(_err(res[q][0], r64[q][0]), _err(r32[q][0], r64[q][0])) for q in ("perm_matrices", "weighted_template", "transforms")]
        for (e, g), q in zip(pairs, ("perm_matrices", "weighted_template", "transforms")):
            _held([(e, g)], f"{what} {q}")


def test_weight_edits_are_picked_up():
    import copy
    t, s = rf.inputs("a")
    net = rf.build("a")
    dnet = copy.deepcopy(net).to(DEV)
    with torch.no_grad():
        before = dnet(t.to(DEV), s.to(DEV), 1)["perm_matrices"][0].clone()
        for m in (net, dnet):
            m.feat_extractor.prepool[1].weight.mul_(-1.5)
        after = dnet(t.to(DEV), s.to(DEV), 1)
        r64 = copy.deepcopy(net).double()(t.double(), s.double(), 1)
    gap = rf.pooled_gap("perm_matrices")
    moved = _err(after["perm_matrices"][0], before.cpu().double())
    print(f"a GroupNorm weight edit moves the permutation by {moved / gap:.0f} gaps")
    assert moved > 100 * gap
    _ratio("perm after a weight edit", _err(after["perm_matrices"][0], r64["perm_matrices"][0]), gap)


# ------------------------------------------------------------------------------------------------------------------------------
# the memory contract of every launching entry point: guards, two fills, workspaces by their size functions, const inputs unchanged
_SCRATCH = {
    "l3d_gn_conv": {"workspace": mc.Spec("scratch", "per-workgroup fp64 partials in `workspace` (l3d_gn_conv_workspace_bytes(B, Cout, P) bytes",
                                         size=("l3d_gn_conv_workspace_bytes", lambda v: (v["B"], v["Cout"], v["P"]), 1))},
    "l3d_sinkhorn_slack": {"workspace": mc.Spec("scratch", "Only the potentials live in `workspace` (fp64, l3d_sinkhorn_workspace_bytes(B, J, K) bytes",
                                                size=("l3d_sinkhorn_workspace_bytes", lambda v: (v["B"], v["J"], v["K"]), 1))},
}


def _rand(seed, *shape):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)).to(DEV) * 2 - 1


def _contract(name, build):
    _lib, _, _ = _mods()
    return mc.check(name, build, proto=_lib.EXT_PROTOTYPES[name], contract=_SCRATCH)


def test_memory_contract_ppf_group_and_rigid_and_affine():
    _lib, _, _ = _mods()
    B, N, K = 2, 70, 5
    xyz, nrm = _rand(1, B, N, 3), _rand(2, B, N, 3)
    idx = torch.randint(0, N, (B, N, K), generator=torch.Generator().manual_seed(3)).to(DEV)
    for normals in (nrm, None):
        _contract("l3d_ppf_group", lambda ar: [xyz, normals, idx, B, N, K, ar.f32(B, 10, K, N)])
    a, b, w = _rand(4, B, 37, 3), _rand(5, B, 37, 3), _rand(6, B, 37).abs()
    _contract("l3d_rigid_transform_weighted", lambda ar: [a, b, w, B, 37, 1e-5, ar.f32(B, 3, 4)])
    mom = torch.stack([_rand(7, B, 48).double() * 100, _rand(8, B, 48).double().abs() * 1000 + 200], -1).contiguous()
    gamma, beta = _rand(9, 48), _rand(10, 48)
    _contract("l3d_gn_affine", lambda ar: [mom, gamma, beta, B, 48, 8, 150, 1e-5, ar.f32(B, 48), ar.f32(B, 48)])


@pytest.mark.parametrize("B,Cin,Cout,K,NP,affine,pool,with_y", [(2, 10, 32, 1, 150, True, False, True), (2, 70, 48, 3, 70, True, True, False),
                                                                 (1, 96, 96, 2, 4200, False, True, True), (1, 5, 256, 1, 1, False, False, True)])
def test_memory_contract_gn_conv(B, Cin, Cout, K, NP, affine, pool, with_y):
    """plain and pooled, y = NULL, tails in N' and in Cout's 64-channel block, more position blocks than partial slots (N' 4200)"""
    P = K * NP
    x, w, bias = _rand(11, B, Cin, P), _rand(12, Cout, Cin), _rand(13, Cout)
    a, s = (_rand(14, B, Cin), _rand(15, B, Cin)) if affine else (None, None)
    ws_bytes = _mods()[0].lib().l3d_gn_conv_workspace_bytes(B, Cout, P)

    def build(ar):
        y = ar.f32(B, Cout, P) if with_y else None
        ymax, ymin = (ar.f32(B, Cout, NP), ar.f32(B, Cout, NP)) if pool else (None, None)
        return [x, a, s, w, bias, B, Cin, Cout, P, K if pool else 0, y, ymax, ymin, ar.out(torch.float64, B, Cout, 2), ar.bytes(ws_bytes)]
    out = _contract("l3d_gn_conv", build)
    u = x if not affine else torch.relu(a[:, :, None] * x + s[:, :, None])
    want = torch.matmul(w.double(), u.double()) + bias.double()[None, :, None]
    if with_y:
        assert float((out["y"].double() - want).abs().max()) <= 1e-4
    if pool:
        assert float((out["ymax"].double() - want.view(B, Cout, K, NP).amax(2)).abs().max()) <= 1e-4


@pytest.mark.parametrize("outputs", ["all", "rowsum+weighted", "log_perm"])
def test_memory_contract_sinkhorn(outputs):
    _lib, _, _ = _mods()
    B, J, K = 2, 50, 70
    A, ref = _rand(16, B, J, K) * 9, _rand(17, B, K, 3)
    ws_bytes = _lib.lib().l3d_sinkhorn_workspace_bytes(B, J, K)

    def build(ar):
        lp = ar.f32(B, J, K) if outputs in ("all", "log_perm") else None
        pm = ar.f32(B, J, K) if outputs == "all" else None
        rs, wt = (ar.f32(B, J), ar.f32(B, J, 3)) if outputs != "log_perm" else (None, None)
        return [A, B, J, K, 5, ref if outputs != "log_perm" else None, 1e-5, lp, pm, rs, wt, ar.bytes(ws_bytes)]
    _contract("l3d_sinkhorn_slack", build)
