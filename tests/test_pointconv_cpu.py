"""PointConv without a GPU: the model's surface, its state_dict against the reference's key lists, the op sequence on the CPU
against the fixture from the reference (tests/golden/pointconv_seeded.npz, make_golden_pointconv.py; read through
golden/pointconv_fixture.py), one backward, the new header and the host-side status codes of l3d_pointconv_aggregate.

fp32 on the CPU is held to GAP_FACTOR = 4 x the reference's own fp32-to-fp64 gap of each quantity; fp64 on the CPU to 1e-9 of
everything stored, which is what lets the GPU tests use this package's fp64 op sequence as the whole fp64 tensors."""
import copy
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import pointconv_fixture as pf     # noqa: E402

from learning3d_amd import _lib                                   # noqa: E402
from learning3d_amd.models import create_pointconv                # noqa: E402
from learning3d_amd.models.pointconv import PointConvDensityClsSsg    # noqa: E402
from learning3d_amd.utils import pointconv_util                   # noqa: E402

GAP_FACTOR = pf.GAP_FACTOR
NAME = "l3d_pointconv_aggregate"


def _stored_close(key, v64, tol=1e-9):
    """v64 (this package, fp64) against the stored fp64 value of `key`, whole or sampled"""
    fx = pf.load()
    if key + "_64" in fx:
        want = pf.stored(key + "_64")
        assert tuple(want.shape) == tuple(v64.shape), key
        got = v64
    else:
        want, got = pf.stored(key + "_s64"), pf.sampled(v64)
    e = float((got.detach().double() - want).abs().max())
    assert e <= tol * max(1.0, float(want.abs().max())), (key, e)


def _held(what, error, gap):
    print(f"{what}: error {error:.2e}, gap {gap:.2e}, ratio {error / gap:.2f}")
    assert gap > 0 and error <= GAP_FACTOR * gap, (what, error, gap)


def test_constructor_surface_and_input_shapes():
    Net = create_pointconv()
    assert issubclass(Net, PointConvDensityClsSsg)
    net = Net()
    assert (net.emb_dims, net.input_shape, net.input_channel_dim, net.classifier) == (1024, "bnc", 3, False)
    assert not hasattr(net, "fc1") and [net.sa1.npoint, net.sa2.npoint, net.sa3.npoint] == [512, 128, 1]
    assert (net.sa1.nsample, net.sa2.nsample, net.sa3.nsample, net.sa3.group_all) == (32, 64, None, True)
    assert (net.sa1.bandwidth, net.sa2.bandwidth, net.sa3.bandwidth) == (0.1, 0.2, 0.4)
    head = Net(emb_dims=256, input_channel_dim=6, classifier=True, num_classes=10)
    assert head.fc3.out_features == 10 and head.sa3.linear.out_features == 256 and head.sa1.mlp_convs[0].in_channels == 6
    with pytest.raises(ValueError):
        Net(input_shape="nbc")
    a, b = pf.model("m1"), pf.model("m1", input_shape="bcn")
    x = pf.model_input("m1")
    with torch.no_grad():
        assert torch.equal(a(x), b(x.permute(0, 2, 1).contiguous()))


def test_pretrained_branches_work(tmp_path):
    """classifier with a checkpoint: the reference's class there cannot be instantiated, and PointConvDensityClsSsg ignores the
    path; here both load checkpoint['model_state_dict']"""
    src = pf.model("m2")
    path = str(tmp_path / "pointconv.pth")
    torch.save({"model_state_dict": src.state_dict()}, path)
    Net = create_pointconv(classifier=True, pretrained=path)
    net = Net(input_channel_dim=6, classifier=True, pretrained=path)
    assert isinstance(net.pointconv, PointConvDensityClsSsg)
    direct = PointConvDensityClsSsg(input_channel_dim=6, classifier=True, pretrained=path)
    for other in (net.pointconv, direct):
        for (k, v), (k2, v2) in zip(src.state_dict().items(), other.state_dict().items()):
            assert k == k2 and torch.equal(v, v2), k
    assert isinstance(create_pointconv(classifier=False, pretrained=path)(pretrained=path), PointConvDensityClsSsg)


@pytest.mark.parametrize("name", ["m1", "m2"])
def test_state_dict_keys_are_the_references(name):
    fx = pf.load()
    net = pf.model(name)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in fx[f"{name}_state_keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in fx[f"{name}_state_shapes"]]
    dim, classifier = next(c[1:] for c in pf.MODEL_CASES if c[0] == name)
    fresh = PointConvDensityClsSsg(input_channel_dim=dim, classifier=classifier)
    fresh.load_state_dict(sd, strict=True)
    assert all(k.split(".")[0] in ("sa1", "sa2", "sa3", "fc1", "fc2", "fc3", "bn1", "bn2") for k in sd)


def test_fixture_conditions():
    fx = pf.load()
    gaps = {k: float(v) for k, v in fx.items() if k.endswith("_gap")}
    assert gaps and all(g > 0 for g in gaps.values()), [k for k, g in gaps.items() if not g > 0]
    assert float(fx["conv_factor"]) == pf.CONV_FACTOR and float(fx["dn_bias"]) == pf.DN_BIAS
    assert [str(c) for c in fx["model_cases"]] == [c[0] for c in pf.MODEL_CASES]
    assert [str(c) for c in fx["layer_cases"]] == [c[0] for c in pf.LAYER_CASES]
    assert torch.equal(pf.stored("cloud"), pf.model_cloud(pf.seed()))
    assert os.path.getsize(os.path.join(pf.HERE, "pointconv_seeded.npz")) < (1 << 20)
    for name in ("m1", "m2"):
        for q in ("l1", "l2", "l3"):
            assert float((pf.model_reference64(name)[q] > 0).double().mean()) >= 0.25, (name, q)


@pytest.mark.parametrize("name", [c[0] for c in pf.LAYER_CASES])
def test_layer_op_sequence_reproduces_the_fixture(name):
    xyz, pts = pf.layer_inputs(name, pf.seed())
    ref = pf.layer_reference64(name)
    _stored_close(f"{name}_xyz", ref[0])
    _stored_close(f"{name}_points", ref[1])
    with torch.no_grad():
        got = pf.layer(name)(xyz, pts)
    assert got[0].dtype == torch.float32 and got[1].shape == ref[1].shape
    _held(f"layer {name} points, CPU fp32", pf.err(got[1], ref[1]), pf.gap(f"{name}_points"))
    if f"{name}_xyz_gap" in pf.load():
        _held(f"layer {name} xyz, CPU fp32", pf.err(got[0], ref[0]), pf.gap(f"{name}_xyz"))
    else:
        assert torch.equal(got[0].double(), ref[0])


@pytest.mark.parametrize("name", ["m1", "m2"])
def test_model_op_sequence_reproduces_the_fixture(name):
    ref = pf.model_reference64(name)
    with torch.no_grad():
        got = pf.run_model(pf.model(name), pf.model_input(name))
    assert set(got) == set(ref)
    for q in pf.MODEL_QUANTITIES:
        if q in ref:
            _stored_close(f"{name}_{q}", ref[q])
            _held(f"model {name} {q}, CPU fp32", pf.err(got[q], ref[q]), pf.gap(f"{name}_{q}"))
    if "logp" in ref:
        assert torch.equal(got["logp"].argmax(-1), ref["logp"].argmax(-1))
        assert float((got["logp"].exp().sum(-1) - 1).abs().max()) < 1e-5


def test_backward_of_a_small_layer():
    name = pf.BACKWARD_CASE
    fx = pf.load()
    xyz, pts = pf.layer_inputs(name, pf.seed())
    net = pf.layer(name)
    net64 = copy.deepcopy(net).double()
    out = net(xyz, pts)[1]
    wts = pf.loss_weights(out.shape, pf.seed())
    (out * wts).sum().backward()
    (net64(xyz.double(), pts.double())[1] * wts.double()).sum().backward()
    names = [k for k, _ in net.named_parameters()]
    assert names == [str(k) for k in fx["grad_names"]]
    worst = 0.0
    for (k, p), (_, p64) in zip(net.named_parameters(), net64.named_parameters()):
        _stored_close(f"grad_{k}", p64.grad)
        ratio = pf.err(p.grad, p64.grad) / pf.gap(f"grad_{k}")
        worst = max(worst, ratio)
        assert ratio <= GAP_FACTOR, (k, ratio)
    print(f"backward of {name}: largest error / gap over {len(names)} parameters {worst:.2f}")


def test_torch_forms_of_the_helpers_match_their_definitions():
    g = torch.Generator().manual_seed(3)
    xyz = torch.rand((2, 50, 3), generator=g, dtype=torch.float64)
    fps = pointconv_util._t_farthest_point_sample(xyz, 9)
    assert fps.dtype == torch.int64 and bool((fps[:, 0] == 0).all()) and len(set(fps[0].tolist())) == 9
    d = ((xyz[:, :, None] - xyz[:, None]) ** 2).sum(-1)
    assert float((pointconv_util._t_square_distance(xyz, xyz) - d).abs().max()) < 1e-12
    idx = pointconv_util._knn(4, xyz, xyz[:, :7])
    assert torch.equal(idx, d[:, :7].topk(4, dim=-1, largest=False)[1])
    dens = pointconv_util._density(xyz, 0.3)
    assert float((dens - (torch.exp(-d / (2 * 0.09)) / 0.75).mean(-1)).abs().max()) < 1e-12
    assert torch.equal(pointconv_util._index(xyz, idx), torch.stack([xyz[b][idx[b]] for b in range(2)]))


def test_new_name_is_in_the_open_table_and_disjoint():
    assert NAME in _lib.EXT_SIGNATURES and NAME in _lib.EXT_PROTOTYPES
    assert NAME not in _lib.SIGNATURES and NAME not in _lib.MODEL_SIGNATURES
    assert not set(_lib.EXT_CONSTANTS) & (set(_lib.CONSTANTS) | set(_lib.MODEL_CONSTANTS))
    assert (_lib.L3D_POINTCONV_MAX_C, _lib.L3D_POINTCONV_WN_FLOATS, _lib.L3D_POINTCONV_DN_FLOATS) == (1024, 248, 177)
    proto = _lib.EXT_PROTOTYPES[NAME]
    assert [p.name for p in proto.params] == ["feat", "gxyz", "ginv", "wn", "dn", "B", "C", "K", "S", "out", "stream"]
    assert [p.ctype.startswith("const") for p in proto.params[:5]] == [True] * 5 and not proto.params[9].ctype.startswith("const")
    assert proto.restype is ctypes.c_int and all(p.element == "float" for p in proto.params[:5])
    assert _lib._declared(NAME)[0] is proto


def test_packed_parameter_blocks_have_the_headers_sizes():
    net = pf.layer("d0")
    wn, dn = pointconv_util._packed_net(net.weightnet), pointconv_util._packed_net(net.densitynet)
    assert wn.numel() == _lib.L3D_POINTCONV_WN_FLOATS and dn.numel() == _lib.L3D_POINTCONV_DN_FLOATS
    assert pointconv_util._packed_net(net.weightnet) is wn                              # cached
    with torch.no_grad():
        net.weightnet.mlp_bns[1].running_var.mul_(2.0)
    again = pointconv_util._packed_net(net.weightnet)
    assert again is not wn and not torch.equal(again, wn)
    x = torch.rand((1, 3, 1, 1), generator=torch.Generator().manual_seed(0)) - 0.5
    h = x.view(3)
    for lo, cin, cout in ((0, 3, 8), (32, 8, 8), (104, 8, 16)):
        h = torch.relu(again[lo:lo + cin * cout].view(cout, cin) @ h + again[lo + cin * cout:lo + cin * cout + cout])
    with torch.no_grad():
        assert float((net.weightnet(x).view(16) - h).abs().max()) < 1e-6


def test_null_and_unsupported_statuses_before_any_launch():
    """-1 for a null pointer or a non-positive size, -2 for a shape the kernel does not take: both are decided on the host"""
    f = getattr(_lib.lib(), NAME)
    one = ctypes.c_void_p(16)                      # never dereferenced: every call below returns before a launch
    assert f(None, one, one, one, one, 1, 16, 4, 4, one, None) == -1
    assert f(one, None, one, one, one, 1, 16, 4, 4, one, None) == -1
    assert f(one, one, one, None, one, 1, 16, 4, 4, one, None) == -1
    assert f(one, one, one, one, one, 1, 16, 4, 4, None, None) == -1
    assert f(one, one, one, one, None, 1, 16, 4, 4, one, None) == -1          # ginv without DensityNet's parameters
    for B, Cc, K, S in ((0, 16, 4, 4), (1, 0, 4, 4), (1, 16, 0, 4), (1, 16, 4, 0), (1, 16, -3, 4)):
        assert f(one, one, None, one, None, B, Cc, K, S, one, None) == -1
    for B, Cc in ((1, 8), (1, 24), (1, 40), (1, 1040), (65536, 16)):
        assert f(one, one, None, one, None, B, Cc, 4, 4, one, None) == -2
