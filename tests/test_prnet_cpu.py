"""PRNet without a device: the public surface, the state_dict keys, the op-sequence route on the CPU in fp32 and fp64 against the
fixture (tests/golden/prnet_seeded.npz, made from the reference by make_golden_prnet.py; cases, clouds and rescaling in
golden/prnet_fixture.py), the two loss signatures, keypoint order, one backward, head='mlp', the new header and the host-side
status codes of the two entry points."""
import copy
import ctypes
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import prnet_fixture as pf     # noqa: E402
from seeded import seeded_params    # noqa: E402

from learning3d_amd import _lib                      # noqa: E402
from learning3d_amd.models import PRNet              # noqa: E402
from learning3d_amd.models import prnet as P         # noqa: E402

GAP_FACTOR = pf.GAP_FACTOR
CASE_NAMES = [c[0] for c in pf.CASES]
KP, PAIR = "l3d_prnet_keypoints", "l3d_soft_correspondence_pair"


def test_exports_and_constructor_defaults():
    for name in ("pairwise_distance", "cycle_consistency", "PointNet", "DGCNN", "MLPHead", "TemperatureNet", "SVDHead", "KeyPointNet", "PRNet"):
        assert hasattr(P, name), name
    sig = inspect.signature(PRNet.__init__)
    want = dict(emb_nn='dgcnn', attention='transformer', head='svd', emb_dims=512, num_keypoints=512, num_subsampled_points=768,
                num_iters=3, cycle_consistency_loss=0.1, feature_alignment_loss=0.1, discount_factor=0.9, input_shape='bnc')
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == want
    assert list(sig.parameters)[1:] == list(want)
    net = PRNet(emb_dims=64, num_keypoints=16, num_subsampled_points=32)
    assert isinstance(net.keypointnet, P.KeyPointNet) and net.temp_net.temp_factor == 100 and net.head.cat_sampler == 'softmax'
    assert type(PRNet(emb_dims=64, num_keypoints=32, num_subsampled_points=32).keypointnet).__name__ == "Identity"
    for fn in ("spam", "predict_embedding", "predict_keypoint_correspondence"):
        assert callable(getattr(net, fn))
    assert ACT_LRELU_UNCHANGED()
    with pytest.raises(Exception):
        PRNet(emb_nn='other')


def ACT_LRELU_UNCHANGED():
    return P.EDGE_GATHER_MAX_N == 32768 and P.ACT_LRELU == 0x3E4CCCCD and callable(P.DGCNN._layer_params)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_state_dict_keys_are_the_references(name):
    keys, shapes = [str(k) for k in pf.load()[f"{name}_state_keys"]], [str(s) for s in pf.load()[f"{name}_state_shapes"]]
    net = pf.model(name)
    sd = net.state_dict()
    assert list(sd.keys()) == keys and [str(tuple(v.shape)) for v in sd.values()] == shapes
    net.load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()}, strict=True)
    for prefix in ("emb_nn.", "temp_net.nn.0.", "temp_net.nn.9.", "head.reflect", "head.temperature"):
        assert any(k.startswith(prefix) for k in keys), prefix
    if pf.case(name)[1][2] == "transformer":
        assert any(k.startswith("attention.model.") for k in keys)


def _ratios(name, got, label):
    worst = {}
    for q in pf.quantities(name):
        if got.get(q) is None:
            continue
        worst[q] = pf.err(got[q], pf.truth(name, q)) / pf.gap(f"{name}_{q}")
    print(f"{label} {name}: error / gap " + " ".join(f"{q} {r:.2f}" for q, r in worst.items()))
    return worst


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fp64_op_sequence_reproduces_what_the_reference_computes_in_fp64(name):
    """1e-9 against the reference's own fp64 predict_embedding, every iteration; the head and loop truths then lean on this run"""
    q, log, _ = pf.reference64(name)
    iters = pf.case(name)[1][6]
    for key in ["temperature", "disparity"] + [f"temperature_it{i}" for i in range(iters)]:
        assert pf.err(pf.sampled(q[key]), pf.stored(f"{name}_{key}_64")) < 1e-9, key
    if q["emb_k_src"] is not None:
        assert pf.err(pf.sampled(q["emb_k_src"]), pf.stored(f"{name}_emb_k_src_64")) < 1e-9
        assert torch.equal(log[0][0], pf.stored(f"{name}_kp_src")) and torch.equal(log[0][1], pf.stored(f"{name}_kp_tgt"))
    for key in pf.HEAD0 + pf.FINAL:                       # (self-consistency of the file: these were written from this very run)
        if f"{name}_{key}_64" in pf.load():
            assert pf.err(pf.sampled(q[key]), pf.stored(f"{name}_{key}_64")) < 1e-9, key


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fp32_op_sequence_within_the_references_own_gap(name):
    net = pf.model(name)
    with torch.no_grad():
        got, _ = pf.run(net, name, *pf.inputs(name))
    worst = _ratios(name, got, "cpu fp32")
    assert worst and max(worst.values()) <= GAP_FACTOR, worst
    for q in pf.quantities(name):                         # and the stored reference values are what the gap says
        ref32 = pf.stored(f"{name}_{q}_ref32")
        assert pf.err(ref32, pf.sampled(pf.truth(name, q))) <= pf.gap(f"{name}_{q}") * (1 + 1e-12)


def test_three_and_four_input_forward_give_the_same_loss():
    name = "m4"
    src, tgt, Rab, tab = pf.inputs(name)
    net = pf.model(name)
    igt = torch.eye(4).repeat(src.shape[0], 1, 1)
    igt[:, :3, :3], igt[:, :3, 3] = Rab, tab
    with torch.no_grad():
        a, b, c = net(src, tgt, Rab, tab), net(src, tgt, igt), net(src, tgt)
    assert torch.equal(a["loss"], b["loss"]) and a["loss"].dim() == 0 and "loss" not in c
    assert set(a) == {"est_R", "est_t", "est_T", "transformed_source", "loss"}
    assert torch.equal(a["est_R"], c["est_R"]) and a["est_T"].shape == (2, 4, 4) and a["transformed_source"].shape == src.shape
    assert torch.equal(a["est_T"][:, :3, :3], a["est_R"]) and torch.equal(a["est_T"][:, :3, 3], a["est_t"])
    bcn = pf.build_model(PRNet, name, pf.seed(), input_shape="bcn")
    with torch.no_grad():
        d = bcn(src.permute(0, 2, 1), tgt.permute(0, 2, 1), Rab, tab)
    assert torch.equal(d["loss"], a["loss"]) and torch.equal(d["transformed_source"], a["transformed_source"].permute(0, 2, 1))


def test_keypoints_come_in_ascending_order_with_ties_at_the_kth_value():
    g = torch.Generator().manual_seed(3)
    Bn, C, N, K = 2, 16, 40, 13
    emb = torch.rand((Bn, C, N), generator=g)
    order = (emb ** 2).sum(1).argsort(dim=1, descending=True)
    for b in range(Bn):                                   # the K-th and (K+1)-th largest columns become one duplicated point
        emb[b, :, order[b, K]] = emb[b, :, order[b, K - 1]]
    xyz = torch.rand((Bn, 3, N), generator=g)
    kp = P.KeyPointNet(K)
    sk, tk, se, te = kp(xyz, xyz, emb, emb)
    si, ti = kp.idx
    assert si.shape == (Bn, K) and bool((si[:, 1:] > si[:, :-1]).all()) and torch.equal(si, ti)
    for b in range(Bn):
        assert torch.equal(sk[b], xyz[b][:, si[b]]) and torch.equal(se[b], emb[b][:, si[b]])
        sq = (emb[b] ** 2).sum(0)
        assert float(sq[si[b]].min()) >= float(sq.sort(descending=True)[0][K - 1])      # a valid top-K set, whichever twin it holds


def test_backward_of_the_loss_against_the_references_fp32_backward():
    name = str(pf.load()["grad_case"])
    names = [str(k) for k in pf.load()["grad_names"]]
    src, tgt, Rab, tab = pf.inputs(name)
    net = pf.model(name)
    net(src, tgt, Rab, tab)["loss"].backward()
    net64 = copy.deepcopy(pf.model(name)).double()
    net64(src.double(), tgt.double(), Rab.double(), tab.double())["loss"].backward()
    p32, p64 = dict(net.named_parameters()), dict(net64.named_parameters())
    worst = {}
    for k in names:
        assert pf.err(pf.sampled(p64[k].grad), pf.stored(f"grad_{k}_64")) < 1e-9, k
        worst[k] = pf.err(p32[k].grad, p64[k].grad) / pf.gap(f"grad_{k}")
    print("backward: error / gap " + " ".join(f"{k} {r:.2f}" for k, r in worst.items()))
    assert len(names) >= 20 and max(worst.values()) <= GAP_FACTOR, worst


def test_mlp_head_builds_and_runs_and_train_mode_counts_iterations():
    net = seeded_params(PRNet(emb_nn='pointnet', attention='identity', head='mlp', emb_dims=64, num_keypoints=16,
                              num_subsampled_points=32, num_iters=2), 5).eval()
    g = torch.Generator().manual_seed(1)
    src, tgt = torch.rand((3, 32, 3), generator=g), torch.rand((3, 32, 3), generator=g)
    with torch.no_grad():
        out = net(src, tgt)
    R = out["est_R"]
    assert R.shape == (3, 3, 3) and float((R @ R.transpose(1, 2) - torch.eye(3)).abs().max()) < 1e-5
    assert float((torch.det(R) - 1).abs().max()) < 1e-5
    q = torch.tensor([[0.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 0.0]])           # (x, y, z, w): identity; half a turn about x
    assert torch.equal(P.quat2mat(q)[0], torch.eye(3)) and torch.equal(P.quat2mat(q)[1], torch.diag(torch.tensor([1.0, -1.0, -1.0])))
    svd = PRNet(emb_nn='pointnet', attention='identity', emb_dims=64, num_keypoints=16, num_subsampled_points=32, num_iters=2)
    assert float(svd.head.my_iter) == 1
    svd.train()(src, tgt)
    assert float(svd.head.my_iter) == 1 + 2 * 2                            # two head calls per iteration
    svd.eval()(src, tgt)
    assert float(svd.head.my_iter) == 5


def test_new_names_are_in_the_open_table_and_disjoint():
    for name in (KP, PAIR, PAIR + "_workspace_bytes"):
        assert name in _lib.EXT_SIGNATURES and name in _lib.EXT_PROTOTYPES
        assert name not in _lib.SIGNATURES and name not in _lib.MODEL_SIGNATURES
    assert not set(_lib.EXT_CONSTANTS) & (set(_lib.CONSTANTS) | set(_lib.MODEL_CONSTANTS))
    assert (_lib.L3D_PRNET_MAX_N, _lib.L3D_SOFTCORR_PAIR_MAX_C) == (16384, 512)
    kp, pair = _lib.EXT_PROTOTYPES[KP], _lib.EXT_PROTOTYPES[PAIR]
    assert [p.name for p in kp.params] == ["emb", "emb_p", "xyz", "B", "C", "N", "K", "idx", "xyz_k", "emb_k", "mean", "stream"]
    assert [p.name for p in pair.params] == ["src_emb", "tgt_emb", "src", "tgt", "temperature", "B", "C", "N", "M", "workspace", "corr_ab",
                                             "corr_ba", "stream"]
    assert [p.ctype.startswith("const") for p in kp.params[:3]] == [True] * 3 and kp.params[7].element == "int64_t"
    assert [p.ctype.startswith("const") for p in pair.params[:5]] == [True] * 5
    assert not any(p.ctype.startswith("const") for p in kp.params[7:11] + pair.params[9:12])
    assert kp.restype is ctypes.c_int and pair.restype is ctypes.c_int
    assert _lib.EXT_PROTOTYPES[PAIR + "_workspace_bytes"].restype is ctypes.c_size_t


def test_null_and_unsupported_statuses_before_any_launch():
    """-1 for a null pointer, a non-positive size or K > N, -2 for a shape the kernels do not take: decided on the host"""
    lib = _lib.lib()
    kp, pair = getattr(lib, KP), getattr(lib, PAIR)
    one = ctypes.c_void_p(16)                      # never dereferenced: every call below returns before a launch
    assert kp(None, one, one, 1, 16, 8, 4, one, one, one, one, None) == -1
    assert kp(one, one, one, 1, 16, 8, 4, one, one, one, None, None) == -1           # the means are not optional
    assert kp(one, one, None, 1, 16, 8, 4, one, one, one, one, None) == -1           # xyz_k without xyz
    for Bn, C, N, K in ((0, 16, 8, 4), (1, 0, 8, 4), (1, 16, 0, 4), (1, 16, 8, 0), (1, 16, 8, 9)):
        assert kp(one, None, one, Bn, C, N, K, None, None, None, one, None) == -1
    for Bn, N in ((1, 16385), (65536, 8)):
        assert kp(one, None, one, Bn, 16, N, 4, None, None, None, one, None) == -2
    args = lambda **kw: [kw.get("se", one), kw.get("te", one), kw.get("s", one), kw.get("t", one), kw.get("temp", one), kw.get("B", 1),
                         kw.get("C", 16), kw.get("N", 4), kw.get("M", 4), None, kw.get("ab", one), kw.get("ba", one), None]
    for bad in (dict(se=None), dict(te=None), dict(temp=None), dict(ab=None, ba=None), dict(t=None), dict(s=None), dict(B=0), dict(C=0),
                dict(N=0), dict(M=-1)):
        assert pair(*args(**bad)) == -1, bad
    for bad in (dict(C=8), dict(C=24), dict(C=528), dict(B=65536)):
        assert pair(*args(**bad)) == -2, bad
    assert lib.l3d_soft_correspondence_pair_workspace_bytes(32, 512, 512) == lib.l3d_soft_correspondence_pair_workspace_bytes(1, 1, 1) >= 0
