"""DeepGMR without a GPU: the public names, the reference's 44 backbone state_dict keys, the op-sequence forward and backward against
the reference's fp64 values (tests/golden/make_golden_deepgmr.py), the torch restatement of get_rri against the reference's output,
use_rri=False / use_tnet=True against an fp64 restatement written here, and the header table of the three new entry points.

Bars: a quantity of the whole model is held to 4 x the reference's own fp32-to-fp64 gap on the same input (GAP_FACTOR, the project's
bar for whole models: test_masknet_cpu.py); features per column kind, outside the fixture's masks (entries within tau of the 2 pi
wrap; points whose neighbour order hangs on rounding)."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from seeded import seeded_params      # noqa: E402
import deepgmr_fixture as fx          # noqa: E402

GAP_FACTOR = 4.0
CASES = ("a", "b", "c")
KINDS = ("rp", "rq", "theta", "phi")


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deepgmr_seeded.npz")))


def case_shape(z, name):
    B, N, k, J, d = (int(v) for v in z["case_shapes"][list(z["cases"]).index(name)])
    return B, N, k, J, d, str(z["case_inputs"][list(z["cases"]).index(name)])


def build_deepgmr(z, name):
    """our DeepGMR with the weights of fixture case `name` (eval mode), and the case's arrays"""
    from learning3d_amd.models import DeepGMR
    c = fx.load_case(z, name)
    B, N, k, J, d, fmt = case_shape(z, name)
    net = DeepGMR(use_rri=True, nearest_neighbors=k, d_model=d, n_clusters=J)
    seeded_params(net.backbone, int(c["seed"]))
    with torch.no_grad():
        for v in net.backbone.state_dict().values():
            if v.dim() == 3:
                v.mul_(float(c["factor"]))
    return net.eval(), c


def case_inputs(z, name, c, source="s_cloud", source_feat="s_feat32"):
    """(template, source) in the case's input format: [B,N,3+4k] with the reference's fp32 features, or [B,N,3]"""
    if case_shape(z, name)[5] == "points":
        return T(c["t_cloud"]), T(c[source])
    return torch.cat([T(c["t_cloud"]), T(c["t_feat32"])], dim=2), torch.cat([T(c[source]), T(c[source_feat])], dim=2)


def model_quantities(net):
    out = {"est_T": net.est_T, "est_T_inverse": net.est_T_inverse}
    for cn, name in (("t", "template"), ("s", "source")):
        for q in ("gamma", "pi", "mu", "sigma"):
            out[f"{cn}_{q}"] = getattr(net, f"{name}_{q}")
    return {k: v.detach().cpu().double().numpy() for k, v in out.items()}


def gap_ratios(got, c):
    """max |quantity - fp64| over the reference's own fp32-to-fp64 gap, per quantity"""
    return {k: float(np.abs(v - c[k + "64"]).max()) / float(c[k + "_gap"]) for k, v in got.items()}


def feature_ratios(feat, c, cn, skip_points=False):
    """per column kind: max |feat - fp64| over the kind's gap, outside the unstable-phi mask (and the unstable points)"""
    B, N, k4 = feat.shape
    d = np.abs(np.asarray(feat, dtype=np.float64) - c[f"{cn}_feat64"]).reshape(B, N, k4 // 4, 4)
    keep = np.ones((B, N, k4 // 4), dtype=bool)
    if skip_points:
        keep &= ~c[f"{cn}_point_unstable"][:, :, None]
    out = [float(d[..., i][keep].max()) / float(c[f"{cn}_feat_gap"][i]) for i in range(3)]
    out.append(float(d[..., 3][keep & ~c[f"{cn}_phi_unstable"]].max()) / float(c[f"{cn}_feat_gap"][3]))
    return dict(zip(KINDS, out))


def test_public_names_and_state_keys(fixture):
    import learning3d_amd.models as Mo
    from learning3d_amd.models import deepgmr as G
    from learning3d_amd import data_utils
    for name in ("gmm_params", "gmm_register", "Conv1dBNReLU", "FCBNReLU", "TNet", "PointNet", "DeepGMR", "FUSED"):
        assert hasattr(G, name), name
    assert Mo.DeepGMR is G.DeepGMR and hasattr(data_utils, "rri_features") and hasattr(data_utils, "get_rri")
    want = [str(k) for k in fixture["state_keys"]]
    assert len(want) == 44
    net = G.PointNet(use_rri=True)
    assert list(net.state_dict().keys()) == want
    assert net.encoder[0][0].weight.shape == (64, 80, 1) and net.decoder[0][0].weight.shape == (512, 2048, 1)      # the paper's defaults
    assert net.decoder[3].weight.shape == (16, 128, 1)
    model = G.DeepGMR()
    assert list(model.state_dict().keys()) == ["backbone." + k for k in want]
    # strict load both ways: a state_dict with exactly the reference's keys into ours, and ours into a second instance
    shaped = {k: torch.zeros_like(v) for k, v in net.state_dict().items()}
    assert set(shaped) == set(want)
    net.load_state_dict(shaped, strict=True)
    G.DeepGMR().load_state_dict(model.state_dict(), strict=True)
    with_tnet = G.PointNet(use_rri=False, use_tnet=True, d_model=64, n_clusters=4)
    assert [k for k in with_tnet.state_dict() if not k.startswith("tnet.")] == want
    assert sum(k.startswith("tnet.") for k in with_tnet.state_dict()) == 3 * 6 + 2 * 6 + 2


def test_feature_model_none_builds_a_backbone():
    from learning3d_amd.models.deepgmr import DeepGMR, PointNet
    a, b = DeepGMR(feature_model=None, nearest_neighbors=8, d_model=64, n_clusters=4), DeepGMR(nearest_neighbors=8, d_model=64, n_clusters=4)
    assert isinstance(a.backbone, PointNet) and a.backbone is not b.backbone
    assert a.backbone.encoder[0][0].weight.shape == (64, 32, 1) and a.backbone.decoder[3].weight.shape == (4, 128, 1)
    given = PointNet(use_rri=False, d_model=64, n_clusters=4)
    assert DeepGMR(use_rri=False, feature_model=given).backbone is given
    with pytest.raises(ValueError, match="two clouds of one size"):
        DeepGMR(use_rri=False, feature_model=given).eval()(torch.rand(1, 40, 3), torch.rand(1, 30, 3))


@pytest.mark.parametrize("name", CASES)
def test_op_sequence_matches_reference_fp64(fixture, name):
    """fp32 on the CPU within GAP_FACTOR gaps of the reference's fp64 for the logits, gamma, pi, mu, sigma and both T; the model in
    fp64 reproduces the reference's fp64 gamma, pi, mu, sigma and T to 1e-12 in every case (case c computes its features from the
    stored cloud, centred in fp64 on both sides), and the logits to the 1/8192 of their gap they are stored to"""
    net, c = build_deepgmr(fixture, name)
    B, N, k, J, d, fmt = case_shape(fixture, name)
    template, source = case_inputs(fixture, name, c)
    with torch.no_grad():
        out = net(template, source)
    assert set(out) == {"est_R", "est_t", "est_R_inverse", "est_t_inverese", "est_T", "est_T_inverse", "r", "transformed_source"}
    assert out["est_R"].shape == (B, 3, 3) and out["est_t"].shape == (B, 3) and out["est_T_inverse"].shape == (B, 4, 4)
    assert out["r"].shape == (B, 4 * k, N) and out["transformed_source"].shape == (B, N, 3)
    assert net.template_sigma.shape == (B, J, 3, 3) and net.source_gamma.shape == (B, N, J) and not hasattr(net, "igt")
    assert torch.equal(out["est_t_inverese"], net.est_T_inverse[:, :3, 3]) and torch.equal(out["est_R"], net.est_T[:, :3, :3])
    want = torch.matmul(net.est_T[:, :3, :3], net.source.transpose(1, 2)).transpose(1, 2) + net.est_T[:, None, :3, 3]
    assert torch.allclose(out["transformed_source"], want, atol=1e-6)
    ratios = gap_ratios(model_quantities(net), c)
    print(name, "fp32 op sequence, error / gap:", {k: round(v, 2) for k, v in ratios.items()})
    assert max(ratios.values()) <= GAP_FACTOR, ratios
    # the planted motion: template = source * est_T, source = template * igt
    assert float((net.est_T.double() - T(c["igt"]).double().inverse()).abs().max()) < 1e-4

    net64 = copy.deepcopy(net).double()
    with torch.no_grad():
        net64(template.double(), source.double())
    got = model_quantities(net64)
    for key, v in got.items():
        err = float(np.abs(v - c[key + "64"]).max())
        assert err <= 1e-12, (key, err)
    for cn, cloud in (("t", template), ("s", source)):
        with torch.no_grad():
            l32 = net.backbone(net._features(cloud).transpose(1, 2)).double().numpy()
            l64 = net64.backbone(net64._features(cloud.double()).transpose(1, 2)).numpy()
        gap = float(c[f"{cn}_logits_gap"])
        assert float(np.abs(l32 - c[f"{cn}_logits64"]).max()) <= GAP_FACTOR * gap
        assert float(np.abs(l64 - c[f"{cn}_logits64"]).max()) <= 1e-12 + gap / 8192
    assert net64.est_T.dtype == torch.float64 and net64.template_sigma.dtype == torch.float64


@pytest.mark.parametrize("name", CASES)
def test_rri_features_cpu_match_get_rri(fixture, name):
    """the torch restatement on the reference's centred clouds: in fp64 it reproduces get_rri's fp64 output on the stable points
    (outside the phi mask: to the 1/8192 of a gap the fixture stores, the neighbours equal to the k-d tree's); in fp32 it stays within
    GAP_FACTOR gaps per column kind; both layouts hold the same numbers"""
    from learning3d_amd.data_utils import get_rri, rri_features
    from learning3d_amd.data_utils.rri import knn_idx, rri_from_idx
    c = fx.load_case(fixture, name)
    k = case_shape(fixture, name)[2]
    for cn in "ts":
        centred = T(c[f"{cn}_centred"])
        stable = ~c[f"{cn}_point_unstable"]
        idx = knn_idx(centred.double(), k).numpy()
        assert np.array_equal(idx[stable], c[f"{cn}_idx"][stable])
        f64 = rri_features(centred.double(), k, center=False)
        assert f64.dtype == torch.float64
        r64 = feature_ratios(f64.numpy(), c, cn, skip_points=True)
        assert max(r64.values()) <= 1.0 / 4096, r64
        f32 = rri_from_idx(centred, T(c[f"{cn}_idx"]))
        r32 = feature_ratios(f32.numpy(), c, cn)
        print(name, cn, "fp32 restatement, error / gap:", {k_: round(v, 2) for k_, v in r32.items()})
        assert f32.dtype == torch.float32 and max(r32.values()) <= GAP_FACTOR, r32
        assert torch.equal(rri_from_idx(centred, T(c[f"{cn}_idx"]), channel_first=True), f32.transpose(1, 2))
        one = get_rri(c[f"{cn}_centred"][0].astype(np.float64), k)
        assert one.dtype == np.float64 and np.array_equal(one, f64[0].numpy())
        # center=True subtracts the centroid: the same features from a shifted cloud, up to the rounding of the shift
        here, moved = rri_features(centred.double(), k), rri_features(centred.double() + 0.25, k)
        assert float((moved - here).abs()[T(stable)].max()) < 1e-9


def test_backward_matches_reference_fp64(fixture):
    """mse(est_T @ igt, I) + mse(est_T_inverse @ igt^-1, I) on the fixture's jittered pair: every parameter's gradient within
    GAP_FACTOR x the reference's own fp32-to-fp64 gap of that parameter, at the stored entries flat[::stride]"""
    net, c = build_deepgmr(fixture, "b")
    template, source = case_inputs(fixture, "b", c, source="bw_source", source_feat="bw_s_feat32")
    igt = T(c["igt"])
    eye = torch.eye(4).expand_as(igt)
    out = net(template, source)
    loss = torch.nn.functional.mse_loss(out["est_T"] @ igt, eye) + torch.nn.functional.mse_loss(out["est_T_inverse"] @ igt.inverse(), eye)
    assert abs(float(loss.detach()) - float(c["grad_loss64"])) <= GAP_FACTOR * max(abs(float(c["grad_loss32"]) - float(c["grad_loss64"])), 2.0 ** -24 * float(c["grad_loss64"]))
    loss.backward()
    params = dict(net.backbone.named_parameters())
    names = [str(n) for n in c["grad_names"]]
    assert names == list(params)
    worst = {}
    for i, n in enumerate(names):
        g = params[n].grad.reshape(-1)[::int(c["grad_stride"][i])].double().numpy()
        assert g.shape == c[f"grad64_{i}"].shape
        worst[n] = float(np.abs(g - c[f"grad64_{i}"]).max()) / float(c["grad_gap"][i])
    print("gradient error / gap, largest:", sorted(worst.items(), key=lambda kv: -kv[1])[:3])
    assert max(worst.values()) <= GAP_FACTOR, worst


def _restated_fp64(net, template, source):
    """DeepGMR.forward for use_rri=False restated in fp64 from the state_dict alone: -> gamma (template, source), est_T, est_T_inverse"""
    sd = {k: v.double() for k, v in net.backbone.state_dict().items()}
    eps = 1e-5

    def bn(y, p):
        shape = (1, -1, 1) if y.dim() == 3 else (1, -1)
        return ((y - sd[p + ".running_mean"].view(shape)) / torch.sqrt(sd[p + ".running_var"].view(shape) + eps)
                * sd[p + ".weight"].view(shape) + sd[p + ".bias"].view(shape))

    def conv_bn_relu(x, p):
        return torch.relu(bn(torch.einsum("oc,bcn->bon", sd[p + ".0.weight"][:, :, 0], x), p + ".1"))

    def fc_bn_relu(x, p):
        return torch.relu(bn(x @ sd[p + ".0.weight"].t(), p + ".1"))

    def backbone(x):
        if net.backbone.use_tnet:
            f = x
            for i in range(3):
                f = conv_bn_relu(f, f"tnet.encoder.{i}")
            f = f.max(dim=2)[0]
            f = fc_bn_relu(fc_bn_relu(f, "tnet.decoder.0"), "tnet.decoder.1")
            f = f @ sd["tnet.decoder.2.weight"].t() + sd["tnet.decoder.2.bias"]
            r1 = f[:, :3] / f[:, :3].norm(dim=1, keepdim=True)
            v = f[:, 3:] - (r1 * f[:, 3:]).sum(dim=1, keepdim=True) * r1
            r2 = v / v.norm(dim=1, keepdim=True)
            x = torch.stack([r1, r2, torch.linalg.cross(r1, r2)], dim=2) @ x
        for i in range(4):
            x = conv_bn_relu(x, f"encoder.{i}")
        x = torch.cat([x, x.max(dim=2, keepdim=True)[0].expand_as(x)], dim=1)
        for i in range(3):
            x = conv_bn_relu(x, f"decoder.{i}")
        return torch.einsum("oc,bcn->bno", sd["decoder.3.weight"][:, :, 0], x) + sd["decoder.3.bias"]

    fit = []
    for cloud in (template.double(), source.double()):
        feats = cloud - cloud.mean(dim=2, keepdim=True)                      # over the COORDINATE axis, as the reference writes it
        gamma = torch.softmax(backbone(feats.transpose(1, 2)), dim=2)
        npi = gamma.sum(dim=1)
        mu = torch.einsum("bnj,bnc->bjc", gamma, cloud) / npi[:, :, None]
        var = (gamma * ((cloud[:, :, None, :] - mu[:, None]) ** 2).sum(-1)).sum(dim=1) / npi
        fit.append((gamma, npi / cloud.shape[1], mu, var))

    def register(pi, mu_s, mu_t, var_t):
        cs, ct = (pi[:, :, None] * mu_s).sum(1), (pi[:, :, None] * mu_t).sum(1)
        Ms = torch.einsum("bj,bjr,bjc->brc", pi / var_t, mu_s - cs[:, None], mu_t - ct[:, None])
        U, _, Vh = torch.linalg.svd(Ms)
        V = Vh.transpose(1, 2)
        S = torch.eye(3, dtype=torch.float64).repeat(pi.shape[0], 1, 1)
        S[:, 2, 2] = torch.det(V @ U.transpose(1, 2))
        R = V @ S @ U.transpose(1, 2)
        out = torch.eye(4, dtype=torch.float64).repeat(pi.shape[0], 1, 1)
        out[:, :3, :3], out[:, :3, 3] = R, ct - (R @ cs[:, :, None])[:, :, 0]
        return out

    (gt, pt, mt, vt), (gs, ps, ms, vs) = fit
    return (gt, gs), register(ps, ms, mt, vt), register(pt, mt, ms, vs)


@pytest.mark.parametrize("use_tnet", [False, True])
def test_without_rri_and_with_tnet_against_fp64_restatement(use_tnet):
    """use_rri=False (the coordinate-axis mean of the reference) with and without the TNet: the model in fp64 equals the restatement
    above to 1e-9 (the same arithmetic in another order); in fp32 its gamma, a softmax whose logits of order one carry a few hundred
    fp32 roundings (<= 2e-5), stays within 1e-4"""
    from learning3d_amd.models.deepgmr import DeepGMR, PointNet
    B, N = 2, 96
    net = DeepGMR(use_rri=False, feature_model=seeded_params(PointNet(use_rri=False, use_tnet=use_tnet, d_model=128, n_clusters=6), 77)).eval()
    with torch.no_grad():
        for k, v in net.backbone.state_dict().items():
            if v.dim() == 3 and not k.startswith("tnet."):
                v.mul_(2.0)
    g = torch.Generator().manual_seed(5)
    template = torch.rand((B, N, 3), generator=g) * 2 - 1
    ang = torch.tensor(0.4)
    R = torch.tensor([[ang.cos(), -ang.sin(), 0.0], [ang.sin(), ang.cos(), 0.0], [0.0, 0.0, 1.0]])
    source = template @ R.t() + 0.2
    (gt, gs), est_T, est_T_inverse = _restated_fp64(net, template, source)
    with torch.no_grad():
        out32 = net(template, source)
        g32 = (net.template_gamma.double(), net.source_gamma.double())
        net64 = copy.deepcopy(net).double()
        out64 = net64(template.double(), source.double())
    assert out32["r"].shape == (B, 3, N) and out32["transformed_source"].shape == (B, N, 3)
    assert float((net64.template_gamma - gt).abs().max()) < 1e-9 and float((net64.source_gamma - gs).abs().max()) < 1e-9
    assert float((out64["est_T"] - est_T).abs().max()) < 1e-9 and float((out64["est_T_inverse"] - est_T_inverse).abs().max()) < 1e-9
    assert float((g32[0] - gt).abs().max()) < 1e-4 and float((g32[1] - gs).abs().max()) < 1e-4
    # not the centroid: a network fed the centred cloud gives other assignments
    centred = (template - template.mean(dim=1, keepdim=True)).double()
    with torch.no_grad():
        other = torch.softmax(net64.backbone(centred.transpose(1, 2)), dim=2)
    assert float((other - gt).abs().max()) > 1e-3


def test_new_entry_points_are_read_from_their_header():
    """include/models/l3d_deepgmr.h through the same parser: argument tables, constants, and the status codes that need no device
    (null pointers -> -1; k 1, k 65, J 65 -> -2: both are decided before any launch)"""
    from learning3d_amd import _lib
    P, I = ctypes.c_void_p, ctypes.c_int
    want = {"l3d_rri_features": [P, P, I, I, I, I, P, P],
            "l3d_gmm_params": [P, P, I, I, I, P, P, P, P, P],
            "l3d_gmm_register": [P, P, P, P, I, I, P, P]}
    assert _lib.MODEL_SIGNATURES == want
    assert all(_lib.MODEL_PROTOTYPES[n].restype is I for n in want) and not set(want) & set(_lib.SIGNATURES)
    par = [(p.ctype, p.name) for p in _lib.MODEL_PROTOTYPES["l3d_rri_features"].params]
    assert par[1] == ("const int64_t *", "idx") and par[-1] == ("l3d_stream_t", "stream")
    assert (_lib.L3D_RRI_MAX_K, _lib.L3D_GMM_MAX_J) == (64, 64)
    l = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, P)
    assert l.l3d_rri_features(None, p, 1, 8, 4, 0, p, None) == -1 and l.l3d_rri_features(p, p, 1, 0, 4, 0, p, None) == -1
    assert l.l3d_rri_features(p, p, 1, 8, 1, 0, p, None) == -2 and l.l3d_rri_features(p, p, 1, 80, 65, 0, p, None) == -2
    assert l.l3d_gmm_params(p, p, 1, 4, 8, None, p, p, None, None) == -1 and l.l3d_gmm_params(p, p, 1, 0, 8, None, p, p, p, None) == -1
    assert l.l3d_gmm_params(p, p, 1, 65, 8, None, p, p, p, None) == -2
    assert l.l3d_gmm_register(p, p, p, None, 1, 4, p, None) == -1 and l.l3d_gmm_register(p, p, p, p, 1, 65, p, None) == -2
    with pytest.raises(_lib.L3DError, match=r"l3d_gmm_params: parameter `const float \*logits` takes a torch.float32 tensor"):
        _lib.call("l3d_gmm_params", torch.zeros(4, dtype=torch.float64), None, 1, 1, 1, None, None, None, None)
