"""PointConv on the GPU: l3d_pointconv_aggregate alone, the fused route of the set-abstraction layers and the whole network
against the fixture from the reference (tests/golden/pointconv_seeded.npz, make_golden_pointconv.py; read through
golden/pointconv_fixture.py).

The bar everywhere is GAP_FACTOR = 4: the error against the reference's fp64 is at most 4 x the reference's own fp32-to-fp64 gap
of that quantity.  Where the fixture stores a large tensor only as samples, the whole fp64 tensor is this package's op sequence
in fp64 on the CPU, which tests/test_pointconv_cpu.py holds to 1e-9 against everything stored.  Beside every fused number the
op-sequence route on the device is held to the same bar.  The kernel-alone tests run at shapes the fixture does not have; their
gap is torch's own fp32 against fp64 on the same operands (the layer's op sequence on the CPU), computed in the test.

Measured ratios (error / gap) are printed by every test; the last run's are in LABLOG.md R20.1."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import memory_contract as mc     # noqa: E402
import pointconv_fixture as pf   # noqa: E402
from seeded import seeded_params  # noqa: E402

pytestmark = pytest.mark.gpu
GAP_FACTOR = pf.GAP_FACTOR
DEV = "cuda"
NAME = "l3d_pointconv_aggregate"


def _mods():
    from learning3d_amd import _lib
    from learning3d_amd.utils import pointconv_util
    return _lib, pointconv_util


def _ratio(what, error, gap, factor=GAP_FACTOR):
    print(f"{what}: error {error:.2e}, gap {gap:.2e}, ratio {error / gap if gap else float('inf'):.2f}")
    assert gap > 0 and error <= factor * gap, (what, error, gap)


def _logged(fn, fused=True):
    """-> (fn(), the C-ABI calls it made) with pointconv_util.FUSED = fused"""
    _lib, PU = _mods()
    PU.FUSED = fused
    _lib.LAUNCH_LOG = log = []
    try:
        with torch.no_grad():
            res = fn()
    finally:
        PU.FUSED = True
        _lib.LAUNCH_LOG = None
    return res, log


# ------------------------------------------------------------------------------------------------------------------------------
# the kernel alone
def _nets(seed, dead=False):
    _, PU = _mods()
    wn = seeded_params(PU.WeightNet(3, 16), seed).eval()
    dn = seeded_params(PU.DensityNet(), seed + 1).eval()
    with torch.no_grad():
        for net in (wn, dn):
            for c in net.mlp_convs:
                c.weight.mul_(pf.CONV_FACTOR)
        dn.mlp_bns[-1].bias.fill_(-100.0 if dead else pf.DN_BIAS)
    return wn, dn


def _operands(seed, B, Cc, K, S, density):
    g = torch.Generator().manual_seed(seed)
    feat = torch.relu(torch.rand((B, Cc, K, S), generator=g) * 2 - 0.6)                 # a post-ReLU activation, a third of it zero
    gxyz = (torch.rand((B, S, K, 3), generator=g) - 0.5) * 0.4
    ginv = (torch.rand((B, S, K), generator=g) * 3 + 0.5) if density else None
    return feat, gxyz, ginv


def _aggregate_ops(feat, gxyz, ginv, wn, dn):
    """the layer's own op sequence for this step (utils/pointconv_util.py:_tail and the density product) -> [B,16 C,S]"""
    B, Cc, K, S = feat.shape
    if ginv is not None:
        scale = (ginv / ginv.max(dim=2, keepdim=True)[0])[:, :, :, None]                # [B,S,K,1]
        feat = feat * dn(scale.permute(0, 3, 2, 1))
    w = wn(gxyz.permute(0, 3, 2, 1))                                                    # [B,16,K,S]
    out = torch.matmul(feat.permute(0, 3, 1, 2), w.permute(0, 3, 2, 1)).reshape(B, S, 16 * Cc)
    return out.permute(0, 2, 1)


def _aggregate_dev(feat, gxyz, ginv, wn, dn, out=None):
    _lib, PU = _mods()
    B, Cc, K, S = feat.shape
    if out is None:
        return PU.pointconv_aggregate(feat.to(DEV), gxyz.to(DEV), None if ginv is None else ginv.to(DEV),
                                      PU._packed_net(wn).to(DEV), PU._packed_net(dn).to(DEV) if ginv is not None else None)
    _lib.call(NAME, feat.to(DEV), gxyz.to(DEV), None if ginv is None else ginv.to(DEV), PU._packed_net(wn).to(DEV),
              PU._packed_net(dn).to(DEV) if ginv is not None else None, B, Cc, K, S, out)
    return out


EDGE_SHAPES = [  # B, C, K, S, density
    (1, 16, 1, 5, True),          # one neighbour
    (2, 32, 5, 70, True),         # K below a chunk, S past one tile of 64 by 6
    (1, 48, 33, 3, True),         # K one past four chunks; C a multiple of 16 only: the four-channel instantiation
    (1, 16, 200, 1, True),        # a group_all layer: one centre, many neighbours (S = 1 has its own kernel: four chunks of 64)
    (2, 1024, 130, 1, True),      # that kernel at the widest channel count, two clouds, K two past two chunks
    (1, 48, 64, 1, False),        # that kernel with a partial channel block (48 of 64), exactly one chunk, no density
    (1, 32, 7, 2, True),          # the smallest S the general kernel takes
    (1, 1024, 3, 2, True),        # the widest channel count
    (3, 32, 9, 65, False),        # several clouds, no density, S one past a tile
    (2, 16, 8, 64, False),        # exactly one chunk and one tile
]


@pytest.mark.parametrize("B,Cc,K,S,density", EDGE_SHAPES)
def test_aggregate_edge_shapes(B, Cc, K, S, density):
    wn, dn = _nets(100 + Cc + K)
    feat, gxyz, ginv = _operands(7 + K + S, B, Cc, K, S, density)
    gxyz[0, 0] = 0.0                                  # a centre whose neighbours are all the centre itself
    with torch.no_grad():
        r32 = _aggregate_ops(feat, gxyz, ginv, wn, dn)
        r64 = _aggregate_ops(feat.double(), gxyz.double(), None if ginv is None else ginv.double(),
                             copy.deepcopy(wn).double(), copy.deepcopy(dn).double())
    got = _aggregate_dev(feat, gxyz, ginv, wn, dn)
    assert got.shape == (B, 16 * Cc, S) and got.is_contiguous()
    assert float(r64.abs().max()) > 0.01 and float(r64[0, :, 0].abs().max()) > 0                      # the zero-offset centre is alive
    _ratio(f"aggregate B {B} C {Cc} K {K} S {S} density {density}", pf.err(got, r64), pf.err(r32, r64))
    _ratio("  the centre with zero offsets", pf.err(got[0, :, 0], r64[0, :, 0]), pf.err(r32, r64))


def test_aggregate_dead_density_gives_exact_zeros_and_the_same_bits_twice():
    wn, dead = _nets(31, dead=True)
    feat, gxyz, ginv = _operands(5, 2, 32, 7, 70, True)
    got = _aggregate_dev(feat, gxyz, ginv, wn, dead)
    assert bool((got == 0).all())
    wn, dn = _nets(31)
    B, Cc, K, S = feat.shape
    outs = []
    for fill in (7.0, float("nan"), -1e30):
        out = torch.full((B, 16 * Cc, S), fill, dtype=torch.float32, device=DEV)
        outs.append(_aggregate_dev(feat, gxyz, ginv, wn, dn, out=out).clone())
    assert float(outs[0].abs().max()) > 0.01
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(outs[0], _aggregate_dev(feat, gxyz, ginv, wn, dn))


def test_aggregate_refuses_what_it_does_not_take():
    _lib, PU = _mods()
    wn, dn = _nets(3)
    feat, gxyz, ginv = _operands(5, 1, 24, 4, 4, True)
    with pytest.raises(_lib.L3DError, match="status -2"):
        _aggregate_dev(feat, gxyz, ginv, wn, dn)


@pytest.mark.parametrize("density", [True, False])
def test_memory_contract_aggregate(density):
    """guards, two fills, const inputs unchanged, at a shape with tails in S (70), K (5) and C (48: the four-channel instantiation)"""
    _lib, PU = _mods()
    B, Cc, K, S = 2, 48, 5, 70
    wn, dn = _nets(11)
    feat, gxyz, ginv = (None if t is None else t.to(DEV) for t in _operands(9, B, Cc, K, S, density))
    wnp, dnp = PU._packed_net(wn).to(DEV), (PU._packed_net(dn).to(DEV) if density else None)
    got = mc.check(NAME, lambda ar: [feat, gxyz, ginv, wnp, dnp, B, Cc, K, S, ar.f32(B, 16 * Cc, S)], proto=_lib.EXT_PROTOTYPES[NAME])
    assert torch.equal(got["out"], PU.pointconv_aggregate(feat, gxyz, ginv, wnp, dnp))


# ------------------------------------------------------------------------------------------------------------------------------
# the layers and the whole network on the fixture
@pytest.mark.parametrize("name", [c[0] for c in pf.LAYER_CASES])
def test_layer_fused_and_op_sequence_on_the_fixture(name):
    xyz, pts = pf.layer_inputs(name, pf.seed())
    xd, pd = xyz.to(DEV), None if pts is None else pts.to(DEV)
    net = pf.layer(name).to(DEV)
    ref = pf.layer_reference64(name)
    fused, log = _logged(lambda: net(xd, pd))
    assert log.count(NAME) == 1, log
    seq, log = _logged(lambda: net(xd, pd), fused=False)
    assert NAME not in log, log
    assert fused[0].shape == seq[0].shape == ref[0].shape and fused[1].shape == seq[1].shape == ref[1].shape
    assert float((fused[1] > 0).float().mean()) >= 0.25
    for what, res in (("op sequence", seq), ("fused", fused)):
        _ratio(f"layer {name} {what} points", pf.err(res[1], ref[1]), pf.gap(f"{name}_points"))
        if f"{name}_xyz_gap" in pf.load():
            _ratio(f"layer {name} {what} xyz", pf.err(res[0], ref[0]), pf.gap(f"{name}_xyz"))
        else:
            assert torch.equal(res[0].cpu().double(), ref[0]), (name, what)


@pytest.mark.parametrize("name", ["m1", "m2"])
def test_model_fused_and_op_sequence_on_the_fixture(name):
    x = pf.model_input(name).to(DEV)
    net = pf.model(name).to(DEV)
    ref = pf.model_reference64(name)
    fused, log = _logged(lambda: pf.run_model(net, x))
    assert log.count(NAME) == 3, log
    assert log.count("l3d_bmm_f32") == (6 if "logp" in ref else 3), log      # a Linear per layer, three in the head
    seq, log = _logged(lambda: pf.run_model(net, x), fused=False)
    assert NAME not in log, log
    assert set(fused) == set(seq) == set(ref)
    for q in pf.MODEL_QUANTITIES:
        if q in ref:
            _ratio(f"model {name} op sequence {q}", pf.err(seq[q], ref[q]), pf.gap(f"{name}_{q}"))
            _ratio(f"model {name} fused {q}", pf.err(fused[q], ref[q]), pf.gap(f"{name}_{q}"))
    if "logp" in ref:
        assert torch.equal(fused["logp"].argmax(-1).cpu(), ref["logp"].argmax(-1))
        assert torch.equal(seq["logp"].argmax(-1).cpu(), ref["logp"].argmax(-1))


def test_pointconv_util_golden_layer_on_both_routes(golden):
    """the layer of test_gpu_parity.py::test_pointconv_util_golden, with its tolerances, with the switch on and off"""
    _, PU = _mods()
    g = golden("pointconv_util")
    xyz = torch.from_numpy(g["xyz"]).to(DEV)
    sa = PU.PointConvDensitySetAbstraction(npoint=64, nsample=16, in_channel=8, mlp=[16, 32], bandwidth=0.1, group_all=False)
    sa.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w.")})
    sa = sa.to(DEV).eval()
    feats = torch.from_numpy(g["feats"]).to(DEV)
    for fused in (True, False):
        (sxyz, spts), log = _logged(lambda: sa(xyz.permute(0, 2, 1), feats), fused=fused)
        assert (NAME in log) == fused
        np.testing.assert_allclose(sxyz.cpu().numpy(), g["sa_xyz"], rtol=0, atol=0)
        np.testing.assert_allclose(spts.cpu().numpy(), g["sa_points"], rtol=1e-4, atol=1e-5)


def test_forward_fused_replays_from_one_graph():
    """the whole fused forward captured into one graph on one stream and replayed twice gives the eager bits: no host read, no
    stale state"""
    name = "m2"
    x = pf.model_input(name).to(DEV)
    net = pf.model(name).to(DEV)
    order = ("l1", "l2", "l3", "logp")
    with torch.no_grad():
        res = pf.run_model(net, x)
        eager = [res[q].clone() for q in order]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            pf.run_model(net, x)                                         # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        _lib, _ = _mods()
        _lib.LAUNCH_LOG = log = []
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                res = pf.run_model(net, x)
        finally:
            _lib.LAUNCH_LOG = None
        assert log.count(NAME) == 3
        out = [res[q] for q in order]
        for replay in range(2):
            for v in out:
                v.fill_(7.0)                                             # stale values must not survive a replay
            graph.replay()
            torch.cuda.synchronize()
            for i, (a, b) in enumerate(zip(out, eager)):
                assert torch.equal(a, b), (replay, order[i])


def _cpu_gap_and_ref(net, xyz, pts, grad=False):
    """the CPU op sequence of `net` in fp32 and fp64 -> (gap of the feature output, the fp64 output); the module's state is left
    as it was (train-mode BatchNorm updates running statistics: both runs work on copies)"""
    with torch.set_grad_enabled(grad):
        r32 = copy.deepcopy(net)(xyz, pts)[1]
        r64 = copy.deepcopy(net).double()(xyz.double(), None if pts is None else pts.double())[1]
    return pf.err(r32, r64.detach()), r64.detach()


def test_fallbacks_take_the_op_sequence():
    """requires_grad input, train-mode BatchNorm, fp64 and a width the kernel refuses take the op sequence (launch log).  Where the
    fused route exists for the same computation (requires_grad, fp64) the two agree within twice the bar (each is within the bar
    of fp64); train-mode BatchNorm and mlp[-1] = 40 compute something the fused route does not, and are held to 4 x the CPU fp32
    op sequence's gap against the CPU fp64 op sequence of the same module"""
    _lib, PU = _mods()
    name = "d0"
    xyz, pts = pf.layer_inputs(name, pf.seed())
    xd, pd = xyz.to(DEV), pts.to(DEV)
    cpu_net = pf.layer(name)
    net = copy.deepcopy(cpu_net).to(DEV)
    fused, log = _logged(lambda: net(xd, pd))
    assert NAME in log
    bar = 2 * GAP_FACTOR * pf.gap(f"{name}_points")
    _lib.LAUNCH_LOG = log = []
    try:
        with torch.enable_grad():
            res = net(xd, pd.clone().requires_grad_(True))
    finally:
        _lib.LAUNCH_LOG = None
    assert NAME not in log and res[1].requires_grad
    e = float((res[1].detach() - fused[1]).abs().max())
    print(f"requires_grad input against fused: {e:.2e}, bar {bar:.2e}")
    assert e <= bar
    res, log = _logged(lambda: copy.deepcopy(net).double()(xd.double(), pd.double()))
    assert NAME not in log and res[1].dtype == torch.float64
    e = float((res[1] - fused[1].double()).abs().max())
    print(f"fp64 against fused: {e:.2e}, bar {bar:.2e}")
    assert e <= bar
    # train-mode BatchNorm: batch statistics
    gap, ref = _cpu_gap_and_ref(copy.deepcopy(cpu_net).train(), xyz, pts)
    res, log = _logged(lambda: copy.deepcopy(net).train()(xd, pd))
    assert NAME not in log
    _ratio("train-mode BatchNorm, device op sequence", pf.err(res[1], ref), gap)
    assert float((res[1] - fused[1]).abs().max()) > 100 * gap                # batch statistics: another function than the fused one
    # a width the kernel refuses
    wide = pf.rescale(seeded_params(PU.PointConvDensitySetAbstraction(npoint=24, nsample=5, in_channel=8, mlp=[16, 40], bandwidth=0.1,
                                                                      group_all=False), pf.seed() + 99)).eval()
    gap, ref = _cpu_gap_and_ref(wide, xyz, pts)
    res, log = _logged(lambda: copy.deepcopy(wide).to(DEV)(xd, pd))
    assert NAME not in log and res[1].shape == (xyz.shape[0], 40, 24)
    _ratio("mlp[-1] = 40, device op sequence", pf.err(res[1], ref), gap)


def test_weight_edits_are_picked_up():
    """an in-place weight edit and a running_var edit under torch.no_grad(), and a load_state_dict, reach the cached folded
    parameters: the result moves by far more than the gap and again meets the bar"""
    _, PU = _mods()
    name = "d0"
    xyz, pts = pf.layer_inputs(name, pf.seed())
    xd, pd = xyz.to(DEV), pts.to(DEV)
    net = pf.layer(name)
    dnet = copy.deepcopy(net).to(DEV)
    other = pf.build_layer(PU, name, pf.seed() + 1).state_dict()

    def edits():
        yield "a WeightNet conv weight edit", lambda m: m.weightnet.mlp_convs[2].weight.mul_(-1.5)
        yield "a DensityNet running_var edit", lambda m: m.densitynet.mlp_bns[0].running_var.mul_(9.0)
        yield "an mlp BatchNorm running_var edit", lambda m: m.mlp_bns[0].running_var.mul_(4.0)
        yield "a bn_linear weight edit", lambda m: m.bn_linear.weight.mul_(-2.0)
        yield "a load_state_dict", lambda m: m.load_state_dict(other)
    before, log = _logged(lambda: dnet(xd, pd))
    assert NAME in log
    before = before[1].clone()
    for what, edit in edits():
        with torch.no_grad():
            for m in (net, dnet):
                edit(m)
        gap, ref = _cpu_gap_and_ref(net, xyz, pts)
        after, log = _logged(lambda: dnet(xd, pd))
        assert NAME in log
        moved = float((after[1] - before).abs().max())
        print(f"{what} moves the output by {moved / gap:.0f} gaps")
        assert moved > 100 * gap, what
        _ratio(f"after {what}", pf.err(after[1], ref), gap)
        before = after[1].clone()
