"""MaskNet2 without a GPU: the public names, the reference's 76 state_dict keys, the op-sequence forward against the reference's fp64
masks (tests/golden/make_golden_masknet2.py), MaskNet2.forward's selection, clouds of unequal sizes, the header table of the three new
entry points, and the numpy models of Mish and of l3d_outer_softmax_mix that the GPU tests compare the kernels with.

Bars: a whole model's masks are held to 4 x the reference's own fp32-to-fp64 gap on the same input (GAP_FACTOR, the project's bar for
whole models: test_masknet_cpu.py); selected sets must equal the fp64 sets on every point farther than the fixture's tau (32 x that
gap) from 0.5."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from seeded import seeded_params      # noqa: E402

GAP_FACTOR = 4.0
CASES = ("a", "b", "c")


def T(a):
    return torch.from_numpy(np.asarray(a))


def case_arrays(z, name):
    return {k[len(name) + 1:]: v for k, v in z.items() if k.startswith(name + "_")}


def prepared(net, seed, factor, beta, bias=None):
    """the fixture's weights: seeded_params, every 3-d tensor of the state (the conv weights) times `factor`, every beta = `beta`,
    and the stored final bias"""
    seeded_params(net, seed)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            if v.dim() == 3:
                v.mul_(factor)
            if k.endswith(".beta"):
                v.fill_(beta)
        if bias is not None:
            net.maskNet.h3[3].bias.fill_(bias)
    return net


def build_masknet2(z, name):
    """our MaskNet2 with the weights of fixture case `name` (eval mode), and the case's arrays"""
    from learning3d_amd.models import MaskNet2
    from learning3d_amd.models.masknet2 import PointNet
    c = case_arrays(z, name)
    net = prepared(MaskNet2(feature_model=PointNet(use_bn=True), is_training=False), int(c["seed"]), float(z["weight_factor"]),
                   float(z["beta"]), float(c["bias"]))
    return net.eval(), c


def mask_ratios(template_mask, source_mask, c):
    """max |mask - fp64| over the reference's own fp32-to-fp64 gap, per mask"""
    return tuple(float(np.abs(np.asarray(m, dtype=np.float64) - c[k + "_mask64"]).max()) / float(c[k + "_gap"])
                 for k, m in (("t", template_mask), ("s", source_mask)))


def run_masks(net, c, dev="cpu"):
    with torch.no_grad():
        t, s = net.maskNet(T(c["template"]).to(dev), T(c["source"]).to(dev))
    return t.cpu().numpy(), s.cpu().numpy()


def check_forward(net, c, dev, what):
    """MaskNet2.forward of a B = 1 case: the masks within the bar, index sets ascending and equal to the fp64 sets outside the tau
    band, masked clouds = cloud[idx]"""
    template, source = T(c["template"]).to(dev), T(c["source"]).to(dev)
    with torch.no_grad():
        masked_t, masked_s, mask_t, mask_s = net(template, source)
    ratios = mask_ratios(mask_t.cpu().numpy(), mask_s.cpu().numpy(), c)
    assert max(ratios) <= GAP_FACTOR, (what, ratios)
    for k, idx, masked, cloud in (("t", net.template_idx, masked_t, template), ("s", net.source_idx, masked_s, source)):
        idx, masked, cloud = idx.cpu().numpy(), masked.cpu().numpy(), cloud.cpu().numpy()
        assert idx.dtype == np.int64 and idx.ndim == 2 and idx.shape[0] == 1
        assert bool((np.diff(idx[0]) > 0).all()), what + ": the indices are not ascending"
        assert np.array_equal(masked[0], cloud[0][idx[0]]), what + ": the masked cloud is not cloud[idx]"
        far = np.abs(c[k + "_mask64"][0] - 0.5) > float(c[k + "_tau"])
        got, want = np.zeros(cloud.shape[1], bool), np.zeros(cloud.shape[1], bool)
        got[idx[0]] = True
        want[c[k + "_idx64"][0]] = True
        assert np.array_equal(got[far], want[far]), what + ": another set outside the tau band"
    return ratios


def mish_model(x):
    """x tanh(softplus(x)) in fp64; -0 where e^x is 0 in the limit (x = -inf), NaN for NaN"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.where(x > 20.0, x, x * np.tanh(np.log1p(np.exp(np.minimum(x, 20.0)))))
    return np.where(np.isneginf(x), -0.0, y)


def outer_softmax_mix_model(px, py, beta):
    """l3d_outer_softmax_mix in fp64: px, py [B,C] -> (outx, outy)
    outx_i = px_i + beta sum_j softmax_j(px_i py_j) px_j,  outy_j = py_j + beta sum_i softmax_i(px_i py_j) py_i"""
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    e = px[:, :, None] * py[:, None, :]                               # [B,i,j]
    pj = np.exp(e - e.max(axis=2, keepdims=True))
    pj /= pj.sum(axis=2, keepdims=True)
    pi = np.exp(e - e.max(axis=1, keepdims=True))
    pi /= pi.sum(axis=1, keepdims=True)
    return px + beta * np.einsum("bij,bj->bi", pj, px), py + beta * np.einsum("bij,bi->bj", pi, py)


def find_mask_restated(pm, sf, tf):
    """find_mask with the repeat counts corrected: each cloud's points meet the OTHER cloud's global feature"""
    g = lambda f: torch.cat([f.max(dim=2)[0], f.mean(dim=2)], dim=1).unsqueeze(2)      # noqa: E731
    a, b = g(sf), g(tf)
    for layer in (pm.global_feat_1, pm.global_feat_2, pm.global_feat_3):
        a, b = layer(a, b)
    x = pm.h3(torch.cat([tf, a.expand(-1, -1, tf.shape[2])], dim=1))
    y = pm.h3(torch.cat([sf, b.expand(-1, -1, sf.shape[2])], dim=1))
    return x.flatten(1), y.flatten(1)


# ---------------------------------------------------------------------------------------------------------------
def test_models_are_exported():
    import learning3d_amd.models as M
    from learning3d_amd.models import masknet2
    assert M.MaskNet2.__name__ == "MaskNet2"
    for name in ("Mish", "BasicConv1D", "Self_Attn", "PointNet", "self_attention_fc", "PointNetMask", "MaskNet2"):
        assert isinstance(getattr(masknet2, name), type), name
    a, b = M.MaskNet2(), M.MaskNet2()
    assert a.maskNet.feature_model is not b.maskNet.feature_model          # a fresh feature model per instance
    assert masknet2.PointNetMask().feature_model is not masknet2.PointNetMask().feature_model
    assert a.is_training and a.maskNet.feature_model.use_bn and a.maskNet.feature_model.emb_dims == 224
    assert callable(M.MaskNet2.index_points) and masknet2.FUSED is True
    assert all(float(m.beta.detach()) == 0.0 for m in a.modules() if hasattr(m, "beta"))


def test_state_dict_keys_match_the_reference(golden):
    z = golden("masknet2_seeded")
    net, _ = build_masknet2(z, "a")
    assert len(z["state_keys"]) == 76 and list(net.state_dict().keys()) == list(z["state_keys"])
    state = {k: torch.zeros_like(v) for k, v in net.state_dict().items()}
    net.load_state_dict({str(k): state[str(k)] for k in z["state_keys"]}, strict=True)


@pytest.mark.parametrize("name", CASES)
def test_cpu_masks_against_fp64(golden, name):
    net, c = build_masknet2(golden("masknet2_seeded"), name)
    ratios = mask_ratios(*run_masks(net, c), c)
    print(f"MaskNet2 case {name} on the CPU: error / gap template {ratios[0]:.2f}, source {ratios[1]:.2f} (bar {GAP_FACTOR})")
    assert max(ratios) <= GAP_FACTOR


def test_cpu_forward_selects_the_fp64_sets(golden):
    net, c = build_masknet2(golden("masknet2_seeded"), "c")
    ratios = check_forward(net, c, "cpu", "case c")
    print(f"MaskNet2.forward case c on the CPU: error / gap {ratios[0]:.2f}, {ratios[1]:.2f}; selected "
          f"{net.template_idx.shape[1]} and {net.source_idx.shape[1]} points")


def test_forward_takes_one_pair(golden):
    net, c = build_masknet2(golden("masknet2_seeded"), "a")
    with pytest.raises(ValueError, match="B == 1"):
        net(T(c["template"]), T(c["source"]))


def test_unequal_sizes_against_restated_find_mask(golden):
    """Nt 96, Ns 64: the reference raises here (its repeat counts are swapped); ours against an fp64 restatement of find_mask with the
    counts corrected.  Bar: 4 x the largest fp32-to-fp64 gap the reference itself shows on the fixture's cases -- the same weights and
    the same depth, on fewer points (shorter sums)."""
    z = golden("masknet2_seeded")
    net, c = build_masknet2(z, "a")
    template, source = T(c["template"])[:, :96].contiguous(), T(c["source"])[:, :64].contiguous()
    with torch.no_grad():
        mt, ms = net.maskNet(template, source)
        net64 = copy.deepcopy(net).double()
        fm = net64.maskNet.feature_model
        wt, ws = find_mask_restated(net64.maskNet, fm(source.double()), fm(template.double()))
    assert tuple(mt.shape) == (2, 96) and tuple(ms.shape) == (2, 64)
    gap = max(float(z[f"{n}_{k}_gap"]) for n in CASES for k in "ts")
    err = max(float((mt.double() - wt).abs().max()), float((ms.double() - ws).abs().max()))
    print(f"unequal sizes: error {err:.2e} = {err / gap:.2f} gaps (bar {GAP_FACTOR})")
    assert err <= GAP_FACTOR * gap


def test_header_table():
    from learning3d_amd import _lib
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    want = {"l3d_mish": [P, L, P, P],
            "l3d_self_attention_shared": [P, P, I, I, I, P, P],
            "l3d_outer_softmax_mix": [P, P, P, I, I, P, P, P]}
    assert {n: _lib.SIGNATURES[n] for n in want} == want
    assert all(_lib.PROTOTYPES[n].restype is I for n in want)
    par = {n: [(p.ctype, p.name) for p in _lib.PROTOTYPES[n].params] for n in want}
    assert par["l3d_mish"] == [("const float *", "x"), ("long", "count"), ("float *", "y"), ("l3d_stream_t", "stream")]
    assert par["l3d_self_attention_shared"] == [("const float *", "q"), ("const float *", "beta"), ("int", "B"), ("int", "D"), ("int", "N"),
                                                ("float *", "out"), ("l3d_stream_t", "stream")]
    assert par["l3d_outer_softmax_mix"] == [("const float *", "px"), ("const float *", "py"), ("const float *", "beta"), ("int", "B"),
                                            ("int", "C"), ("float *", "outx"), ("float *", "outy"), ("l3d_stream_t", "stream")]
    assert _lib.L3D_SELF_ATTN_TQ % 32 == 0 and _lib.L3D_SELF_ATTN_TK % 32 == 0
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(handle, n) for n in want)
    _lib.lib()
    assert all(n in _lib._CALLS for n in want)
    with pytest.raises(_lib.L3DError, match="float32"):                  # the one typed path serves them, too
        _lib.call("l3d_mish", torch.zeros(4, dtype=torch.float64), 4, torch.zeros(4))


def test_numpy_models():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1000, generator=g, dtype=torch.float64) * 6
    want = (x * torch.tanh(torch.nn.functional.softplus(x))).numpy()
    assert np.allclose(mish_model(x.numpy()), want, rtol=1e-14, atol=0)
    edge = mish_model(np.array([-np.inf, np.inf, np.nan, 0.0, -0.0, 25.0]))
    assert edge[0] == 0 and np.signbit(edge[0]) and edge[1] == np.inf and np.isnan(edge[2]) and edge[3] == 0 and edge[5] == 25.0
    # the mix against the reference's own op sequence (our mirror of it), in fp64
    from learning3d_amd.models.masknet2 import self_attention_fc
    px, py = torch.randn(3, 37, generator=g, dtype=torch.float64) * 3, torch.randn(3, 37, generator=g, dtype=torch.float64) * 3
    layer = self_attention_fc(8, 37).double()
    layer.query_conv = torch.nn.Identity()
    with torch.no_grad():
        layer.beta.fill_(0.5)
        ox, oy = layer(px.unsqueeze(2), py.unsqueeze(2))
    mx, my = outer_softmax_mix_model(px.numpy(), py.numpy(), 0.5)
    assert np.allclose(mx, ox[:, :, 0].numpy(), rtol=1e-12, atol=1e-13) and np.allclose(my, oy[:, :, 0].numpy(), rtol=1e-12, atol=1e-13)


# ---------------------------------------------------------------------------------------------------------------
def mfma_32x32x2(a, b, c):
    """v_mfma_f32_32x32x2_f32 lane by lane: lane l supplies A[l % 32][l // 32] and B[l // 32][l % 32]; register r of lane l of the
    accumulator is D[(r % 4) + 8 (r // 4) + 4 (l // 32)][l % 32]"""
    A, Bm = np.zeros((32, 2)), np.zeros((2, 32))
    for l in range(64):
        A[l & 31, l >> 5], Bm[l >> 5, l & 31] = a[l], b[l]
    Dm, out = A @ Bm, c.copy()
    for l in range(64):
        for r in range(16):
            out[l, r] += Dm[(r & 3) + 8 * (r >> 2) + 4 * (l >> 5), l & 31]
    return out


def self_attention_wave_model(q, beta, i0, stride=33):
    """One wave of masknet2.hip's self_attn_kernel in numpy, with the kernel's own index maps: the key tile [D][32] at row stride 33,
    read along keys for S^T and along channels for O^T; the probabilities taken from the S^T accumulators as the B operand of k-step r.
    q [D,N] -> {(channel, query): out}"""
    D, N = q.shape
    lanes = np.arange(64)
    m, h = lanes & 31, lanes >> 5
    qf = [q[2 * s + h, np.minimum(i0 + m, N - 1)] for s in range(D // 2)]
    o = [np.zeros((64, 16)) for _ in range(D // 32)]
    m_run, l_run = np.full(64, -np.inf), np.zeros(64)
    for j0 in range(0, N, 32):
        sK = np.zeros(D * stride)
        for t in range(256):
            for i in range(D // 8):
                sK[((t >> 5) + 8 * i) * stride + (t & 31)] = q[(t >> 5) + 8 * i, min(j0 + (t & 31), N - 1)]
        s = np.zeros((64, 16))
        for ks in range(D // 2):
            s = mfma_32x32x2(sK[(h + 2 * ks) * stride + m], qf[ks], s)
        valid = (j0 + 4 * h)[:, None] + (8 * (np.arange(16) >> 2) + (np.arange(16) & 3))[None, :] < N
        mx = np.where(valid, s, -np.inf).max(axis=1)
        m_new = np.maximum(m_run, np.maximum(mx, mx[lanes ^ 32]))
        with np.errstate(invalid="ignore"):
            alpha = np.exp(m_run - m_new)
        m_run = m_new
        p = np.where(valid, np.exp(s - m_new[:, None]), 0.0)
        l_run = l_run * alpha + p.sum(axis=1)
        for dt in range(D // 32):
            o[dt] *= alpha[:, None]
            for r in range(16):
                o[dt] = mfma_32x32x2(sK[(m + 32 * dt) * stride + 4 * h + 8 * (r >> 2) + (r & 3)], p[:, r], o[dt])
    total = l_run + l_run[lanes ^ 32]
    out = {}
    for l in range(64):
        if i0 + m[l] < N:
            for dt in range(D // 32):
                for r in range(16):
                    c = 32 * dt + 8 * (r >> 2) + 4 * h[l] + (r & 3)
                    out[(c, i0 + m[l])] = q[c, i0 + m[l]] + beta * o[dt][l, r] / total[l]
    return out


@pytest.mark.parametrize("D,N", [(32, 1), (64, 33), (32, 77)])
def test_self_attention_lane_model(D, N):
    """the lane maps the kernel is written on (operand and accumulator layout of the 32x32x2 MFMA, the key slots of each k-step, the
    ragged last tile) give the attention: every output written once, within fp64 rounding of the plain formula"""
    q = np.random.default_rng(D + N).standard_normal((D, N)) * 0.5
    s = q.T @ q
    p = np.exp(s - s.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    want = q + 0.37 * (p @ q.T).T
    got = np.full((D, N), np.nan)
    for i0 in range(0, N, 32):
        for (c, i), v in self_attention_wave_model(q, 0.37, i0).items():
            assert np.isnan(got[c, i])
            got[c, i] = v
    assert float(np.abs(got - want).max()) < 1e-13
    # both read patterns of the tile touch 32 distinct banks per 32-lane half (ds_read_b32: bank = word address % 32)
    m = np.arange(32)
    assert len(set((33 * 5 + m) % 32)) == 32 and len(set((33 * (32 + m) + 13) % 32)) == 32
