"""RPMNet / PPFNet without a GPU: the Python surface, the op-sequence route on CPU tensors in fp32 and fp64, its gradients, the open
header table (include/ext/) and the statuses of the new entry points that need no device."""
import ctypes

import numpy as np
import pytest
import torch

import os
import sys

from learning3d_amd import _lib
from learning3d_amd.models import PPFNet, RPMNet, ppfnet, rpmnet

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import rpmnet_fixture as rf      # noqa: E402

NEW = ("l3d_ppf_group", "l3d_gn_conv", "l3d_gn_conv_workspace_bytes", "l3d_gn_affine", "l3d_sinkhorn_slack",
       "l3d_sinkhorn_workspace_bytes", "l3d_rigid_transform_weighted")


def _clouds(seed, B=2, N=96, J=80):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.cat([torch.rand((B, N // 2, 3), generator=g) * 0.35 - 0.175, torch.rand((B, N - N // 2, 3), generator=g) * 2 - 1], 1)
    nrm = torch.randn((B, N, 3), generator=g)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    t = torch.cat([xyz, nrm], -1)
    return t.contiguous(), (t[:, :J] + torch.tensor([0.1, 0.0, -0.1, 0.0, 0.0, 0.0])).contiguous()


def test_state_dict_keys_and_shapes():
    sd = PPFNet().state_dict()
    assert list(sd) == [f"{stack}.{i}.{p}" for stack, idx in (("prepool", (0, 1, 3, 4, 6, 7)), ("postpool", (0, 1, 3, 4, 6)))
                        for i in idx for p in ("weight", "bias")]
    assert tuple(sd["prepool.0.weight"].shape) == (96, 10, 1, 1) and tuple(sd["prepool.6.weight"].shape) == (192, 96, 1, 1)
    assert tuple(sd["postpool.0.weight"].shape) == (192, 192, 1) and tuple(sd["postpool.6.weight"].shape) == (96, 96, 1)
    assert tuple(PPFNet(features=["ppf", "dxyz"], emb_dims=64).state_dict()["prepool.0.weight"].shape) == (64, 7, 1, 1)
    keys = list(RPMNet().state_dict())
    assert len(keys) == 30 + 22 and keys[0] == "weights_net.prepool.0.weight" and keys[29] == "weights_net.postpool.6.bias"
    assert keys[30:] == ["feat_extractor." + k for k in sd]
    assert tuple(RPMNet().state_dict()["weights_net.postpool.6.weight"].shape) == (2, 256)


def test_default_models_do_not_share_a_feature_model():
    a, b = RPMNet(), RPMNet()
    assert a.feat_extractor is not b.feat_extractor
    assert a.feat_extractor.prepool[0].weight.data_ptr() != b.feat_extractor.prepool[0].weight.data_ptr()
    fx = PPFNet(num_neighbors=8)
    assert RPMNet(feature_model=fx).feat_extractor is fx
    assert a.add_slack is True and a.num_sk_iter == 5


def test_op_sequence_on_cpu_fp32_against_fp64_and_result_dict():
    import copy
    t, s = _clouds(1)
    net = RPMNet(feature_model=PPFNet(num_neighbors=8)).eval()
    with torch.no_grad():
        r32 = net(t, s, max_iterations=2)
        r64 = copy.deepcopy(net).double()(t.double(), s.double(), max_iterations=2)
    assert set(r32) == {"est_R", "est_t", "est_T", "transformed_source", "perm_matrices_init", "perm_matrices", "weighted_template",
                        "beta", "alpha", "transforms"}
    assert r32["beta"].shape == (2, 2) and isinstance(r32["alpha"], np.ndarray) and r64["beta"].dtype == np.float64
    assert len(r32["transforms"]) == 2 and tuple(r32["transforms"][0].shape) == (2, 3, 4) and tuple(r32["est_T"].shape) == (2, 4, 4)
    assert tuple(r32["perm_matrices"][1].shape) == (2, 80, 96) and tuple(r32["weighted_template"][0].shape) == (2, 80, 3)
    assert float((r32["perm_matrices"][1].double() - r64["perm_matrices"][1]).abs().max()) < 1e-5
    for attr in ("beta", "alpha", "feat_source", "feat_template", "affinity", "perm_matrix"):
        assert isinstance(getattr(net, attr), torch.Tensor)
    rows, cols = r64["perm_matrices"][1].sum(2), r64["perm_matrices"][1].sum(1)
    assert float(rows.max()) <= 1 + 1e-9 and float(cols.max()) <= 1 + 1e-9       # the slack keeps both at or below one
    xyz_only = net(t[:, :, :3], s[:, :, :3])                                   # clouds without normals
    assert bool(torch.isfinite(xyz_only["est_T"]).all())


def test_private_grouping_matches_the_definition():
    """the CPU ball query: the centre excluded, the first nsample indices in ascending order inside the radius, the centre as padding"""
    t, _ = _clouds(2)
    xyz = t[:, :, :3].double()
    B, N, _ = xyz.shape
    itself = torch.arange(N)[None].repeat(B, 1)
    idx = ppfnet._query_ball_point(0.3, 8, xyz, xyz, itself)
    d = ((xyz[:, :, None] - xyz[:, None]) ** 2).sum(-1)
    for b in range(B):
        for n in range(0, N, 7):
            inside = [j for j in range(N) if j != n and d[b, n, j] <= 0.09][:8]
            assert idx[b, n].tolist() == inside + [n] * (8 - len(inside))
    f = ppfnet._sample_and_group_multi(0.3, 8, xyz, t[:, :, 3:].double())
    pad = idx == torch.arange(N)[None, :, None]
    assert pad.any() and float(f["ppf"][pad].abs().max()) == 0.0 and float(f["dxyz"][pad].abs().max()) == 0.0


def test_sinkhorn_is_the_two_potential_form():
    """A - u - v with u, v from alternating logsumexp over the zero-padded matrix (the form the kernel computes), in fp64"""
    g = torch.Generator().manual_seed(3)
    for J, K in ((50, 70), (1, 1), (1, 64), (65, 1)):
        A = torch.randn((2, J, K), generator=g, dtype=torch.float64) * 3
        P = torch.nn.functional.pad(A, (0, 1, 0, 1))
        u, v = torch.zeros(2, J + 1, dtype=torch.float64), torch.zeros(2, K + 1, dtype=torch.float64)
        for _ in range(5):
            u[:, :J] = torch.logsumexp(P[:, :J, :] - v[:, None, :], dim=2)
            v[:, :K] = torch.logsumexp(P[:, :, :K] - u[:, :, None], dim=1)
        want = (P - u[:, :, None] - v[:, None, :])[:, :J, :K]
        assert float((rpmnet.sinkhorn(A, 5) - want).abs().max()) < 1e-12
        assert torch.equal(rpmnet.sinkhorn(A, 0), A)
    A = torch.randn((1, 6, 6), generator=g, dtype=torch.float64)
    out = rpmnet.sinkhorn(A, 50, slack=False).exp()
    assert float((out.sum(1) - 1).abs().max()) < 1e-9
    assert tuple(rpmnet.sinkhorn(A, 50, slack=True, eps=1e-3).shape) == (1, 6, 6)


def test_compute_rigid_transform_recovers_motions_and_never_reflects():
    g = torch.Generator().manual_seed(4)
    a = torch.rand((2, 40, 3), generator=g, dtype=torch.float64) * 2 - 1
    q = torch.linalg.qr(torch.randn((2, 3, 3), generator=g, dtype=torch.float64))[0]
    q = q * torch.det(q)[:, None, None]
    w = torch.rand((2, 40), generator=g, dtype=torch.float64) + 0.5
    T = rpmnet.compute_rigid_transform(a, a @ q.transpose(1, 2) + 0.3, w)
    assert float((T[:, :, :3] - q).abs().max()) < 1e-6 and float((T[:, :, 3] - 0.3).abs().max()) < 1e-5      # eps = 1e-5 in the weights
    mirror = torch.diag(torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64))
    T = rpmnet.compute_rigid_transform(a, a @ mirror, w)
    assert float((torch.det(T[:, :, :3]) - 1).abs().max()) < 1e-9
    moved, n = rpmnet.se3_transform(T, a, a)
    assert float((moved - (a @ T[:, :, :3].transpose(1, 2) + T[:, None, :, 3])).abs().max()) < 1e-12 and n.shape == a.shape


def test_gradients_flow_through_the_op_sequence():
    t, s = _clouds(5, B=1, N=64, J=48)
    net = RPMNet(feature_model=PPFNet(num_neighbors=8)).double()
    with torch.no_grad():
        net.weights_net.postpool[-1].bias[0] = 5.0
    res = net(t.double(), s.double(), max_iterations=2)
    loss = sum(((T[:, :, :3] - torch.eye(3, dtype=torch.float64)) ** 2).sum() + (T[:, :, 3] ** 2).sum() for T in res["transforms"])
    loss.backward()
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        # a convolution or linear bias directly in front of a GroupNorm is removed by the normalisation (its gradient is rounding
        # noise); every other parameter moves the output: weights, GroupNorm scales and shifts, the two bare last-layer biases
        stack, index, kind = name.split(".")[-3:]
        owner = net.get_submodule(name.rsplit(".", 2)[0])
        in_front_of_gn = kind == "bias" and int(index) + 1 < len(owner) and isinstance(owner[int(index) + 1], torch.nn.GroupNorm)
        if not in_front_of_gn:
            assert float(p.grad.abs().max()) > 0, name


def test_new_names_are_in_the_open_table_and_disjoint():
    for name in NEW:
        assert name in _lib.EXT_SIGNATURES and name in _lib.EXT_PROTOTYPES
        assert name not in _lib.SIGNATURES and name not in _lib.MODEL_SIGNATURES
    assert not set(_lib.EXT_CONSTANTS) & (set(_lib.CONSTANTS) | set(_lib.MODEL_CONSTANTS))
    assert _lib.L3D_PPF_MAX_K == 64 and _lib.L3D_GN_CONV_MAX_COUT == 256
    names = lambda n: [p.name for p in _lib.EXT_PROTOTYPES[n].params]           # noqa: E731
    assert names("l3d_ppf_group") == ["xyz", "normals", "idx", "B", "N", "K", "feat", "stream"]
    assert names("l3d_gn_conv") == ["x", "in_a", "in_s", "w", "bias", "B", "Cin", "Cout", "P", "pool", "y", "ymax", "ymin", "moments",
                                    "workspace", "stream"]
    assert names("l3d_gn_affine") == ["moments", "gamma", "beta", "B", "C", "groups", "count", "eps", "a", "s", "stream"]
    assert names("l3d_sinkhorn_slack") == ["log_alpha", "B", "J", "K", "n_iters", "xyz_ref", "eps", "log_perm", "perm", "rowsum",
                                           "weighted", "workspace", "stream"]
    assert names("l3d_rigid_transform_weighted") == ["a", "b", "weights", "B", "M", "eps", "T", "stream"]
    assert _lib.EXT_PROTOTYPES["l3d_gn_conv"].params[13].element == "double" and _lib.EXT_PROTOTYPES["l3d_ppf_group"].params[2].element == "int64_t"
    assert _lib.EXT_PROTOTYPES["l3d_sinkhorn_workspace_bytes"].restype is ctypes.c_size_t
    with pytest.raises(_lib.L3DError):
        _lib._declared("l3d_no_such_entry_point")
    assert _lib._declared("l3d_gmm_register")[0] is _lib.MODEL_PROTOTYPES["l3d_gmm_register"]


def test_null_and_unsupported_statuses_before_any_launch():
    """-1 for a null pointer or a non-positive size, -2 for a shape the kernels do not take: both are decided on the host"""
    h = _lib.lib()
    one = ctypes.c_void_p(16)                      # never dereferenced: every call below returns before a launch
    assert h.l3d_ppf_group(None, None, one, 1, 8, 4, one, None) == -1
    assert h.l3d_ppf_group(one, None, one, 1, 0, 4, one, None) == -1
    assert h.l3d_ppf_group(one, None, one, 1, 8, 65, one, None) == -2
    assert h.l3d_gn_conv(one, None, None, None, None, 1, 8, 16, 4, 0, one, None, None, one, one, None) == -1
    assert h.l3d_gn_conv(one, one, None, one, None, 1, 8, 16, 4, 0, one, None, None, one, one, None) == -1      # in_a without in_s
    assert h.l3d_gn_conv(one, None, None, one, None, 1, 8, 16, 4, 0, None, None, None, one, one, None) == -1    # pool = 0 needs y
    assert h.l3d_gn_conv(one, None, None, one, None, 1, 8, 16, 4, 2, None, one, None, one, one, None) == -1     # pooled needs both extremes
    assert h.l3d_gn_conv(one, None, None, one, None, 1, 8, 16, 5, 2, None, one, one, one, one, None) == -1      # P % pool
    assert h.l3d_gn_conv(one, None, None, one, None, 1, 8, 40, 4, 0, one, None, None, one, one, None) == -2     # Cout % 16
    assert h.l3d_gn_conv(one, None, None, one, None, 1, 8, 272, 4, 0, one, None, None, one, one, None) == -2
    assert h.l3d_gn_affine(one, one, one, 1, 12, 8, 4, ctypes.c_float(1e-5), one, one, None) == -2
    assert h.l3d_gn_affine(None, one, one, 1, 16, 8, 4, ctypes.c_float(1e-5), one, one, None) == -1
    assert h.l3d_sinkhorn_slack(one, 1, 4, 4, 5, None, ctypes.c_float(1e-5), None, None, None, None, one, None) == -1   # no output
    assert h.l3d_sinkhorn_slack(one, 1, 4, 4, 5, None, ctypes.c_float(1e-5), None, None, None, one, one, None) == -1    # weighted without xyz_ref
    assert h.l3d_sinkhorn_slack(one, 1, 4, 4, -1, None, ctypes.c_float(1e-5), one, None, None, None, one, None) == -2
    assert h.l3d_rigid_transform_weighted(one, one, None, 1, 4, ctypes.c_float(1e-5), one, None) == -1
    assert h.l3d_rigid_transform_weighted(one, one, one, 70000, 4, ctypes.c_float(1e-5), one, None) == -2
    assert h.l3d_gn_conv_workspace_bytes(2, 96, 2560) == 2 * 96 * 40 * 16 and h.l3d_gn_conv_workspace_bytes(2, 96, 10 ** 6) == 2 * 96 * 64 * 16
    assert h.l3d_gn_conv_workspace_bytes(0, 96, 10) == 0
    assert h.l3d_sinkhorn_workspace_bytes(2, 5, 7) == 2 * 12 * 8 and h.l3d_sinkhorn_workspace_bytes(2, 0, 7) == 0


def test_call_names_the_parameter_of_a_wrong_dtype():
    x = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(_lib.L3DError, match=r"l3d_ppf_group: parameter `const float \*xyz` takes a torch.float32 tensor, got torch.float64"):
        _lib.call("l3d_ppf_group", x, None, x, 1, 1, 1, x)
    f = torch.zeros(4)
    with pytest.raises(_lib.L3DError, match=r"parameter `double \*moments` takes a torch.float64 tensor"):
        _lib.call("l3d_gn_conv", f, None, None, f, None, 1, 1, 16, 1, 0, f, None, None, f, f)
    with pytest.raises(_lib.L3DError, match=r"parameter `const int64_t \*idx`"):
        _lib.call("l3d_ppf_group", f, None, f, 1, 1, 1, f)


# ------------------------------------------------------------------------------------------------------------------------------
# against the fixture from the reference (tests/golden/make_golden_rpmnet.py)
def test_fixture_conditions_and_state_lists():
    fx = rf.load()
    assert float(fx["a_perm_max"]) >= 0.5 and float(fx["a_rowsum_min"]) <= 0.85
    print(f"case a: permutation maximum {float(fx['a_perm_max']):.3f}, row-sum minimum {float(fx['a_rowsum_min']):.3f}")
    for cloud in (fx["template"], fx["source"]):
        x = torch.from_numpy(cloud[:, :, :3]).double()
        n2 = (x ** 2).sum(-1)
        d = n2[:, :, None] + n2[:, None, :] - 2 * x @ x.transpose(1, 2)
        assert bool(((d - float(fx["radius"]) ** 2).abs() > 32 * 2.0 ** -24 * (n2[:, :, None] + n2[:, None, :])).all())
        cnt = (d <= float(fx["radius"]) ** 2).sum(-1)
        assert bool(((cnt > 17).any(1) & (cnt < 16).any(1) & (cnt == 1).any(1)).all())
    sd = PPFNet().state_dict()
    assert list(sd) == list(fx["ppfnet_state_keys"]) and [str(tuple(v.shape)) for v in sd.values()] == list(fx["ppfnet_state_shapes"])
    sd = RPMNet().state_dict()
    assert list(sd) == list(fx["rpmnet_state_keys"]) and [str(tuple(v.shape)) for v in sd.values()] == list(fx["rpmnet_state_shapes"])


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_op_sequence_reproduces_the_fixture(name):
    """fp64 on the CPU within 1e-9 of every stored fp64 value (whole tensors and samples); fp32 within 4 x the reference's own gap"""
    fx = rf.load()
    K, iters, _ = rf.cases()[name]
    r64 = rf.reference64(name)
    close = lambda a, key: float((torch.as_tensor(a).double().reshape(-1) - rf.stored(key).reshape(-1)).abs().max())     # noqa: E731
    worst = max(close(r64[q], f"{name}_{q}_64") for q in ("est_T", "beta", "alpha"))
    for i in range(iters):
        worst = max(worst, close(r64["transforms"][i], f"{name}_transforms{i}_64"), close(r64["weighted_template"][i], f"{name}_weighted_template{i}_64"),
                    close(rf.sampled(r64["perm_matrices"][i]), f"{name}_perm_matrices{i}_s64"))
        init, want = rf.sampled(r64["perm_matrices_init"][i]), rf.stored(f"{name}_perm_matrices_init{i}_s64")
        worst = max(worst, float(((init - want) / want).abs().max()))
    print(f"case {name}: fp64 op sequence against the stored fp64: {worst:.1e}")
    assert worst <= 1e-9
    t, s = rf.inputs(name)
    with torch.no_grad():
        errs = rf.model_errors(rf.build(name)(t, s, iters), name)
    for q, e in errs.items():
        gap = rf.pooled_gap(q)
        print(f"case {name} {q}: fp32 error {e:.2e}, gap {gap:.2e}, ratio {e / gap:.2f}")
        assert e <= rf.GAP_FACTOR * gap, (q, e, gap)


def test_grouping_and_prepool_layers_reproduce_the_fixture():
    fx = rf.load()
    t = torch.from_numpy(fx["template"])
    net64 = rf.build("a").double()
    for name, normals in (("a", True), ("c", False)):
        xyz = t[:, :, :3].double().contiguous()
        nrm = t[:, :, 3:].double().contiguous() if normals else torch.zeros_like(xyz)
        idx = ppfnet._query_ball_point(float(fx["radius"]), 16, xyz, xyz, torch.arange(xyz.shape[1])[None].repeat(xyz.shape[0], 1))
        assert torch.equal(idx, rf.stored(f"group_{name}_idx").long())
        f = ppfnet._sample_and_group_multi(float(fx["radius"]), 16, xyz, nrm)
        for q in ("dxyz", "ppf"):
            assert float((rf.sampled(f[q]) - rf.stored(f"group_{name}_{q}_s64")).abs().max()) <= 1e-12
        if name == "a":
            x = torch.cat([f["xyz"][:, :, None, :].expand(-1, -1, 16, -1), f["dxyz"], f["ppf"]], -1).permute(0, 3, 2, 1)
            with torch.no_grad():
                for i, m in enumerate(net64.feat_extractor.prepool):
                    x = m(x)
                    if i in (0, 3, 6):
                        assert float((rf.sampled(x) - rf.stored(f"layer{i // 3}_s64")).abs().max()) <= 1e-9, i


def test_sinkhorn_and_rigid_transform_against_every_fixture_case():
    fx = rf.load()
    names = [str(n) for n in fx["sinkhorn_cases"]]
    for kind in ([n for n in names if n != "wide"], ["wide"]):
        gap = max(float(fx[f"sk_{n}_gap"]) for n in kind)
        for n in kind:
            x, want = rf.stored(f"sk_{n}_in"), rf.stored(f"sk_{n}_64")
            assert float((rpmnet.sinkhorn(x.double(), 5) - want).abs().max()) <= 1e-9
            assert float((rpmnet.sinkhorn(x, 5).double() - want).abs().max()) <= rf.GAP_FACTOR * gap
            assert torch.equal(rpmnet.sinkhorn(x, 0), x)
    names = [str(n) for n in fx["kabsch_cases"]]
    gap = max(float(fx[f"kab_{n}_gap"]) for n in names)
    for n in names:
        a, b, w, want = (rf.stored(f"kab_{n}_{q}") for q in ("a", "b", "w", "64"))
        assert float((rpmnet.compute_rigid_transform(a.double(), b.double(), w.double()) - want).abs().max()) <= 1e-9, n
        assert float((rpmnet.compute_rigid_transform(a, b, w).double() - want).abs().max()) <= rf.GAP_FACTOR * gap, n
