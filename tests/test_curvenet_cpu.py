"""CurveNet without a GPU: state_dict keys against the reference's, the op-sequence route on CPU tensors against the reference's
fp64 walk (tests/golden/make_golden_curvenet.py), one CIC block's train-mode gradients, and argument validation of curvenet.hip's
entry points.

A flipped arg-max changes a whole curve, so paths and curve features are compared on the curves whose fp64 top-2 logit margin
exceeds the fixture's tau (32 x the reference's own fp32-to-fp64 logit gap); values are held to GAP_FACTOR x the reference's own
fp32-to-fp64 gap on the same entries, the form of SERIES_GAP_FACTOR in test_gpu_registration.py."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from seeded import seeded_params      # noqa: E402

GROUPING_SEED, AGGREGATION_SEED = 5200, 5300          # make_golden_curvenet.py
GAP_FACTOR = 4.0


def T(a):
    return torch.from_numpy(np.asarray(a))


def walk_case(z, si):
    B, N, C, k, cn, cl = [int(v) for v in z["shapes"][si]]
    return {kk[len(f"s{si}."):]: v for kk, v in z.items() if kk.startswith(f"s{si}.")}, (B, N, C, k, cn, cl)


def seeded_grouping(si, shape):
    from learning3d_amd.utils.curvenet_util import CurveAggregation, CurveGrouping
    _, _, C, k, cn, cl = shape
    return (seeded_params(CurveGrouping(C, k, cn, cl), GROUPING_SEED + si).eval(),
            seeded_params(CurveAggregation(C), AGGREGATION_SEED + si).eval())


def by_start(walk, curves):
    """(start ascending, path, curves) of the last forward, keyed by start index like the fixture"""
    start = walk.last_start.long().cpu()
    order = torch.argsort(start, dim=1)
    path = torch.gather(walk.last_path.long().cpu(), 1, order.unsqueeze(-1).expand(-1, -1, walk.last_path.shape[2]))
    curves = curves.detach().cpu()
    return torch.gather(start, 1, order), path, torch.gather(curves, 2, order.view(order.shape[0], 1, -1, 1).expand_as(curves))


def gap_close(got, z, key, what, keep=None):
    """got against the fp64 value, bar = GAP_FACTOR x the reference's own fp32-to-fp64 gap over the same entries"""
    f32, f64 = z["f32." + key].astype(np.float64), z["f64." + key]
    got = np.asarray(got, dtype=np.float64)
    if keep is not None:
        got, f32, f64 = got[keep], f32[keep], f64[keep]
    gap, err = np.abs(f32 - f64).max(), np.abs(got - f64).max()
    print(f"{what}: ours vs fp64 {err:.3e}, reference fp32 vs fp64 {gap:.3e}, ratio {err / gap if gap > 0 else np.inf:.2f} (bar {GAP_FACTOR})")
    assert err <= GAP_FACTOR * gap, what


def check_walk(z, start, path, curves, what):
    """path exact and curves within the gap bar on the curves above tau; at most 5 % of the curves may be left out"""
    assert np.array_equal(start.numpy(), z["start"]), what + ": other start points"
    keep = z["margin"] > float(z["tau"])
    left = int((~keep).sum())
    print(f"{what}: {left} of {keep.size} curves at or below tau {float(z['tau']):.2e} left out")
    assert left <= 0.05 * keep.size
    assert np.array_equal(path.numpy()[keep], z["f64.path"][keep]), what + ": a curve above tau walks another path"
    keepc = np.broadcast_to(keep[:, None, :, None], curves.shape)
    gap_close(curves.numpy(), z, "curves", what + " curves", keep=keepc)


def test_state_dict_keys_match_the_reference(golden):
    from learning3d_amd.models import CurveNet
    from learning3d_amd.utils.curvenet_util import CIC, CurveAggregation, CurveGrouping
    z = golden("curve_walk")
    cic = CIC(npoint=128, radius=0.05, k=20, in_channels=32, output_channels=64, bottleneck_ratio=2, mlp_num=1, curve_config=[100, 5])
    assert list(cic.state_dict().keys()) == list(z["cic_keys"])
    assert list(CurveGrouping(16, 20, 100, 5).state_dict().keys()) == list(z["grouping_keys"])
    assert list(CurveAggregation(16).state_dict().keys()) == list(z["aggregation_keys"])
    assert "start_run" in "".join(z.keys())
    assert list(CurveNet(num_classes=40, k=20, setting='default').state_dict().keys()) == list(z["curvenet_keys"])


def test_op_sequence_walk_and_aggregation_on_cpu(golden):
    zz = golden("curve_walk")
    for si in range(len(zz["shapes"])):
        z, shape = walk_case(zz, si)
        grp, agg = seeded_grouping(si, shape)
        with torch.no_grad():
            curves = grp(T(z["x"]), T(z["xyz"]), T(z["idx"]))
            out = agg(T(z["x"]), curves)
        assert tuple(curves.shape) == (shape[0], shape[2], shape[4], shape[5])
        check_walk(z, *by_start(grp.walk, curves), what=f"shape {shape}")
        # the aggregation mixes ALL curves, those at or below tau included: on the CPU the route runs the reference's fp32 operations,
        # so it walks the reference's fp32 paths, which the fixture has equal to the fp64 ones
        assert np.array_equal(z["f32.path"], z["f64.path"])
        assert np.array_equal(by_start(grp.walk, curves)[1].numpy(), z["f32.path"])
        gap_close(out.numpy(), z, "agg", f"shape {shape} aggregation")


def test_cic_train_mode_gradients_on_cpu(golden):
    from learning3d_amd.utils.curvenet_util import CIC
    z = golden("curvenet_grad")
    B, C2, N = z["x"].shape
    blk = seeded_params(CIC(npoint=N, radius=0.05, k=20, in_channels=C2, output_channels=64, bottleneck_ratio=2, mlp_num=1,
                            curve_config=[100, 5]), int(z["seed"])).train()
    _, out = blk(T(z["xyz"]), T(z["x"]))
    loss = (out ** 2).mean()
    loss.backward()
    start, path, _ = by_start(blk.curvegrouping.walk, torch.zeros(B, 1, 100, 5))
    assert np.array_equal(start.numpy(), z["start"]) and np.array_equal(path.numpy(), z["f64.path"])     # every curve clears tau here
    gap_close(float(loss), z, "loss", "loss")
    gap_close(blk.conv1[0].weight.grad.numpy(), z, "grad_conv1", "conv1.0.weight gradient")
    gap_close(blk.curvegrouping.walk.agent_mlp[0].weight.grad.numpy(), z, "grad_agent", "curvegrouping.walk.agent_mlp.0.weight gradient")


def run_seeded_net(z, dev, fused=True):
    """The seeded classifier on the fixture's cloud with every walk started from the fixture's list, in the reference run's order
    (utils.curvenet_util.select_start replaced; the walk depends on that order).  Returns (logits, per block (start, path) keyed by
    start index, per block the start points the route would have selected itself, ascending)."""
    from learning3d_amd.models import CurveNet
    from learning3d_amd.utils import curvenet_util as cu
    net = seeded_params(CurveNet(num_classes=40, k=20, setting='default'), int(z["seed"])).eval().to(dev)
    lists = iter([T(z[f"w{i}.start_run"]).long().to(dev) for i in range(4)])
    own, orig, was = [], cu.select_start, cu.FUSED_WALK

    def stored(att, curve_num):
        own.append(orig(att, curve_num).sort(dim=1)[0].cpu())
        return next(lists)
    cu.select_start, cu.FUSED_WALK = stored, fused
    try:
        with torch.no_grad():
            logits = net(T(z["input"]).to(dev)).cpu()
    finally:
        cu.select_start, cu.FUSED_WALK = orig, was
    blocks = []
    for blk in (net.cic11, net.cic12, net.cic21, net.cic22):
        w = blk.curvegrouping.walk
        blocks.append(by_start(w, torch.zeros(w.last_path.shape[0], 1, w.last_path.shape[1], 1))[:2])
    return logits, blocks, own


def check_net_paths(z, blocks, what):
    """every block: the stored start points, the fp64 path on every curve above tau, at most 5 % of the curves left out.  Returns
    whether the curves at or below tau walk the fp64 paths too (only then are the logits comparable with the fixture's)."""
    all_agree = True
    for i, (start, path) in enumerate(blocks):
        assert np.array_equal(start.numpy(), z[f"w{i}.start"])
        keep = z[f"w{i}.margin"] > float(z[f"w{i}.tau"])
        same = (path.numpy() == z[f"w{i}.path"]).all(axis=2)
        print(f"{what} walk {i}: {int((~keep).sum())} of {keep.size} curves at or below tau {float(z[f'w{i}.tau']):.2e}, "
              f"{int((~same).sum())} curves off the fp64 path")
        assert (~keep).sum() <= 0.05 * keep.size
        assert same[keep].all(), f"{what} walk {i}: a curve above tau walks another path"
        all_agree = all_agree and bool(same.all())
    return all_agree


def test_seeded_curvenet_logits_on_cpu(golden):
    z = golden("curvenet_seeded")
    logits, blocks, own = run_seeded_net(z, torch.device("cpu"))
    for i in range(4):                                   # the reference's fp32 operations: the same selection
        assert np.array_equal(own[i].numpy(), z[f"w{i}.start"])
    assert check_net_paths(z, blocks, "CPU")             # the reference's fp32 run walks the fp64 paths on every curve (generator)
    gap_close(logits.numpy(), z, "logits", "40 logits")
    assert np.array_equal(logits.numpy().argmax(1), z["f64.logits"].argmax(1))


def test_curvenet_forward_on_cpu_and_exports():
    from learning3d_amd import models, utils
    from learning3d_amd.models.curvenet import curve_config
    assert models.CurveNet.__name__ == "CurveNet" and utils.CIC.__name__ == "CIC" and utils.LPFA.__name__ == "LPFA"
    assert curve_config == {'default': [[100, 5], [100, 5], None, None], 'long': [[10, 30], None, None, None]}
    net = seeded_params(models.CurveNet(num_classes=7, k=20, setting='long'), 11).eval()
    with torch.no_grad():
        out = net(torch.rand(1, 1024, 3, generator=torch.Generator().manual_seed(3)) * 2 - 1)
    assert tuple(out.shape) == (1, 7) and bool(torch.isfinite(out).all())
    assert tuple(net.cic11.curvegrouping.walk.last_path.shape) == (1, 10, 30) and not net.cic21.use_curve


def test_curvenet_argument_validation_without_gpu():
    import ctypes as C
    from learning3d_amd import _lib
    l = _lib.lib()
    buf = C.create_string_buffer(256)
    p = C.cast(buf, C.c_void_p)
    walk = lambda x=p, B=1, N=64, Cc=16, k=20, cn=10, cl=5, out=p: l.l3d_curve_walk(x, p, p, B, N, Cc, k, cn, cl, p, p, p, p, p, p, out, p, None)
    assert walk(x=None) == -1 and walk(out=None) == -1 and walk(B=0) == -1 and walk(cl=0) == -1 and walk(k=0) == -1
    assert walk(Cc=24) == -2 and walk(k=65) == -2 and walk(cn=65) == -2 and walk(Cc=144) == -2
    # a cloud's curves share one workgroup's LDS: curve_num (2 C + 3) <= 16384 words
    assert walk(N=64, Cc=128, cn=64) == -2 and walk(N=2000, Cc=16, cn=469) == -2
    from learning3d_amd.utils.curvenet_util import walk_shape_ok
    assert walk_shape_ok(128, 20, 63, 64) and not walk_shape_ok(128, 20, 64, 64) and not walk_shape_ok(16, 20, 469, 2000)
    assert walk_shape_ok(16, 20, 468, 2000) and not walk_shape_ok(16, 20, 100, 1024, B=65536) and not walk_shape_ok(16, 65, 10, 64)
    assert l.l3d_curve_prepare(p, p, 65536, 16, 8, p, p, None) == -2
    assert l.l3d_curve_prepare(None, p, 1, 16, 8, p, p, None) == -1
    assert l.l3d_curve_prepare(p, p, 1, 16, 0, p, p, None) == -1
    assert l.l3d_curve_prepare(p, p, 1, 16, 8, p, None, None) == -1
    assert l.l3d_curve_prepare(p, p, 1, 24, 8, p, p, None) == -2
    assert l.l3d_curve_prepare(p, p, 1, 144, 8, p, p, None) == -2
