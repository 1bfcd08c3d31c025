"""MaskNet and Segmentation without a GPU: the public names, the reference's state_dict keys, the op-sequence forward against the
reference's fp64 results (tests/golden/make_golden_masknet.py), l3d_masknet.h's entries in the ctypes table, and the numpy model of
l3d_mask_select's rank rule that the GPU tests compare the kernel with.

Bars: a whole model's output is held to 4 x the reference's own fp32-to-fp64 gap on the same input (GAP_FACTOR, the project's bar
for whole models: test_curvenet_cpu.py); selected sets must equal the fp64 sets on every point farther than the fixture's tau
(32 x that gap) from its cloud's boundary value."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from seeded import seeded_params      # noqa: E402

GAP_FACTOR = 4.0
MASK_CASES = ("a", "b", "c", "d")


def T(a):
    return torch.from_numpy(np.asarray(a))


def scaled_seeded_params(net, seed, factor):
    """the fixture's weights: seeded_params, then every 3-d tensor of the state (the conv weights) times `factor`"""
    seeded_params(net, seed)
    with torch.no_grad():
        for v in net.state_dict().values():
            if v.dim() == 3:
                v.mul_(factor)
    return net


def mask_case(z, name):
    return {k[len(name) + 1:]: v for k, v in z.items() if k.startswith(name + "_")}


def build_masknet(z, name):
    """our MaskNet with the weights of fixture case `name` (eval mode), and the case's arrays"""
    from learning3d_amd.models import MaskNet, PointNet
    c = mask_case(z, name)
    net = scaled_seeded_params(MaskNet(feature_model=PointNet(use_bn=True), is_training=False), int(c["seed"]), float(z["weight_factor"]))
    if int(c["threshold_mode"]):
        with torch.no_grad():
            net.maskNet.h3[8].bias.fill_(float(c["bias"]))
    return net.eval(), c


def build_segmentation(z, name):
    from learning3d_amd.models import PointNet, Segmentation
    net = Segmentation(PointNet(global_feat=False, use_bn=bool(int(z[name + "_use_bn"]))), num_classes=int(z["num_classes"]))
    return scaled_seeded_params(net, int(z[name + "_seed"]), float(z["weight_factor"])).eval()


def mask_ratio(mask, c):
    """max |mask - fp64| over the reference's own fp32-to-fp64 gap"""
    return float(np.abs(np.asarray(mask, dtype=np.float64) - c["mask64"]).max()) / float(c["gap"])


def check_selection(idx, masked, template, c, what):
    """idx ascending and distinct, masked = template[idx], and the set equal to the fp64 set outside the tau band"""
    idx, masked, template = np.asarray(idx), np.asarray(masked), np.asarray(template)
    assert idx.dtype == np.int64 and idx.ndim == 2
    far = np.abs(c["mask64"] - c["boundary"][:, None]) > float(c["tau"])
    for b in range(idx.shape[0]):
        assert bool((np.diff(idx[b]) > 0).all()), what + ": mask_idx is not ascending"
        assert np.array_equal(masked[b], template[b][idx[b]]), what + ": the masked template is not template[mask_idx]"
        got, want = np.zeros(template.shape[1], bool), np.zeros(template.shape[1], bool)
        got[idx[b]] = True
        want[c["idx64"][b]] = True
        assert np.array_equal(got[far[b]], want[far[b]]), what + ": another set outside the tau band"
    if not int(c["threshold_mode"]):
        assert idx.shape == c["idx64"].shape, what + ": count != k"


def run_masknet(net, c, dev="cpu"):
    template, source = T(c["template"]).to(dev), T(c["source"]).to(dev)
    with torch.no_grad():
        masked, mask = net(template, source, "threshold" if int(c["threshold_mode"]) else "topk")
    return masked.cpu().numpy(), mask.cpu().numpy(), net.mask_idx.cpu().numpy()


def mask_select_model(mask, k=0, threshold=0.5):
    """The rule of l3d_mask_select in numpy: mask [B,N] -> a list of ascending int64 index arrays, one per cloud.
    k > 0: the points of rank < k, rank(i) = #{j : m_j > m_i, or m_j == m_i and j < i}, a NaN above every number and equal to
    another NaN.  k == 0: m_i > threshold."""
    mask = np.asarray(mask, dtype=np.float32)
    out = []
    for m in mask:
        if k == 0:
            out.append(np.nonzero(m > np.float32(threshold))[0].astype(np.int64))
            continue
        nan = np.isnan(m)
        order = np.lexsort((np.arange(len(m)), -np.where(nan, np.float32(0), m), ~nan))      # NaNs, then descending value, then index
        out.append(np.sort(order[:k]).astype(np.int64))
    return out


def rank_literal(m):
    """rank(i) by the definition, O(N^2)"""
    nan = np.isnan(m)
    gt = (nan[:, None] & ~nan[None, :]) | (m[:, None] > m[None, :])                         # gt[j, i]: m_j orders above m_i
    eq = (nan[:, None] & nan[None, :]) | (m[:, None] == m[None, :])
    j, i = np.meshgrid(np.arange(len(m)), np.arange(len(m)), indexing="ij")
    return (gt | (eq & (j < i))).sum(axis=0)


# ---------------------------------------------------------------------------------------------------------------
def test_models_are_exported():
    import learning3d_amd.models as M
    assert M.MaskNet.__name__ == "MaskNet" and M.Segmentation.__name__ == "Segmentation"
    a, b = M.MaskNet(), M.MaskNet()
    assert a.maskNet.feature_model is not b.maskNet.feature_model          # a fresh feature model per instance
    assert a.is_training and a.maskNet.feature_model.use_bn
    assert callable(M.MaskNet.index_points) and callable(M.MaskNet.find_index)


def test_state_dict_keys_match_the_reference(golden):
    z = golden("masknet_seeded")
    net, _ = build_masknet(z, "a")
    assert list(net.state_dict().keys()) == list(z["state_keys"])
    # arrays under the reference's names load strictly
    state = {k: torch.zeros_like(v) for k, v in net.state_dict().items()}
    net.load_state_dict({str(k): state[str(k)] for k in z["state_keys"]}, strict=True)
    zs = golden("segmentation_seeded")
    for name in zs["cases"]:
        seg = build_segmentation(zs, str(name))
        assert list(seg.state_dict().keys()) == list(zs[str(name) + "_state_keys"])


@pytest.mark.parametrize("name", MASK_CASES)
def test_masknet_cpu_forward_against_fp64(golden, name):
    net, c = build_masknet(golden("masknet_seeded"), name)
    masked, mask, idx = run_masknet(net, c)
    ratio = mask_ratio(mask, c)
    print(f"MaskNet case {name} on the CPU: error / gap {ratio:.2f} (bar {GAP_FACTOR})")
    assert ratio <= GAP_FACTOR
    check_selection(idx, masked, c["template"], c, f"case {name}")


def test_segmentation_cpu_forward_against_fp64(golden):
    z = golden("segmentation_seeded")
    for name in map(str, z["cases"]):
        net = build_segmentation(z, name)
        with torch.no_grad():
            out = net(T(z[name + "_x"]))
        assert tuple(out.shape) == z[name + "_out64"].shape
        ratio = float(np.abs(out.double().numpy() - z[name + "_out64"]).max()) / float(z[name + "_gap"])
        print(f"Segmentation {name} on the CPU: error / gap {ratio:.2f} (bar {GAP_FACTOR})")
        assert ratio <= GAP_FACTOR


def test_masknet_header_entries():
    from learning3d_amd import _lib
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    want = {"l3d_mask_tail": [P, P, P, P, P, I, I, I, I, P, P], "l3d_mask_select": [P, P, I, I, I, F, P, P, P, P]}
    assert {n: _lib.SIGNATURES[n] for n in want} == want
    assert all(_lib.PROTOTYPES[n].restype is I for n in want)
    par = [(p.ctype, p.name) for p in _lib.PROTOTYPES["l3d_mask_select"].params]
    assert par[5] == ("float", "threshold") and par[6] == ("int64_t *", "idx") and par[8] == ("int32_t *", "count")
    assert len(_lib.SIGNATURES) == 113
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "l3d_mask_tail") and hasattr(handle, "l3d_mask_select")
    _lib.lib()                                                           # resolves MaskNet's symbols, too
    assert "l3d_mask_tail" in _lib._CALLS and "l3d_mask_select" in _lib._CALLS
    with pytest.raises(_lib.L3DError, match="float32"):                  # the one typed path serves them: dtype checks
        _lib.call("l3d_mask_select", torch.zeros(1, 4, dtype=torch.float64), torch.zeros(1, 4, 3), 1, 4, 1, 0.5,
                  torch.zeros(1, 1, dtype=torch.int64), torch.zeros(1, 1, 3), torch.zeros(1, dtype=torch.int32))


def test_mask_select_model():
    g = torch.Generator().manual_seed(11)
    m = torch.rand(3, 500, generator=g)                                   # tie-free: the rule is torch.topk's set
    assert len(np.unique(m.numpy())) == m.numel()
    for k in (1, 77, 500):
        want = torch.topk(m, k, dim=1)[1].sort(dim=1)[0].numpy()
        assert np.array_equal(np.stack(mask_select_model(m.numpy(), k)), want)
    # ties, saturation, signed zeros and NaNs against the literal definition
    q = (torch.floor(torch.rand(200, generator=g) * 16) / 16).numpy()
    q[7], q[150], q[31], q[32], q[99] = np.nan, np.nan, -0.0, 0.0, np.inf
    rank = rank_literal(q)
    assert sorted(rank) == list(range(200))                               # a total order
    assert rank[7] == 0 and rank[150] == 1 and rank[99] == 2              # NaN above every number, +inf included
    for k in (1, 2, 3, 50, 120, 200):
        assert np.array_equal(mask_select_model(q[None], k)[0], np.nonzero(rank < k)[0])
    assert np.array_equal(mask_select_model(q[None], 0, 0.5)[0], np.nonzero(q > 0.5)[0])      # strict, and never a NaN
    assert 7 not in mask_select_model(q[None], 0, 0.5)[0]
