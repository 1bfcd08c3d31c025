"""PRNet on the device: the two new entry points alone, the fused tail from the fixture's fp64 keypoint embeddings, the whole model
on both routes against the fixture's fp64 truth (tests/golden/prnet_seeded.npz), route selection, the folded-weight caches, graph
replay and the memory contract.  GAP_FACTOR = 4 is the project's standing bar; every test prints its ratios."""
import copy
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import memory_contract as mc     # noqa: E402
import prnet_fixture as pf       # noqa: E402

pytestmark = pytest.mark.gpu
GAP_FACTOR = pf.GAP_FACTOR
DEV = "cuda"
KP, PAIR = "l3d_prnet_keypoints", "l3d_soft_correspondence_pair"
OUTPUTS = ("est_R", "est_t", "transformed_source", "loss")


def _mods():
    from learning3d_amd import _lib
    from learning3d_amd.models import prnet
    return _lib, prnet


def _ratio(what, error, gap, factor=GAP_FACTOR):
    print(f"{what}: error {error:.2e}, gap {gap:.2e}, ratio {error / gap if gap else float('inf'):.2f}")
    assert gap > 0 and error <= factor * gap, (what, error, gap)


class _Ratios:
    """every figure of a test printed before the first one is held to its bar"""

    def __init__(self):
        self.rows = []

    def add(self, what, error, gap, factor=GAP_FACTOR):
        print(f"{what}: error {error:.2e}, gap {gap:.2e}, ratio {error / gap if gap else float('inf'):.2f}, bar {factor:g}")
        self.rows.append((what, error, gap, factor))

    def hold(self):
        bad = [(w, e / g if g else float("inf"), f) for w, e, g, f in self.rows if not (g > 0 and e <= f * g)]
        assert not bad, bad


def _logged(fn, fused=True, grad=False):
    """-> (fn(), the C-ABI calls it made) with prnet.FUSED = fused"""
    _lib, P = _mods()
    P.FUSED = fused
    _lib.LAUNCH_LOG = log = []
    try:
        with torch.set_grad_enabled(grad):
            res = fn()
    finally:
        P.FUSED = True
        _lib.LAUNCH_LOG = None
    return res, log


def _dev(ts):
    return [None if t is None else t.to(DEV) for t in ts]


# ------------------------------------------------------------------------------------------------------------------------------
# l3d_prnet_keypoints alone
def _keys_cpu(emb, emb_p):
    """the header's key: e = emb + emb_p, key += e * e in ascending c, every operation rounded to fp32"""
    e = emb + emb_p if emb_p is not None else emb.clone()
    key = torch.zeros(e.shape[0], e.shape[2])
    for c in range(e.shape[1]):
        key = key + e[:, c] * e[:, c]
    return e, key


def _select_cpu(key, K):
    """the header's rank rule: greater key first, equal keys by lower index; the chosen indices ascending"""
    order = torch.sort(key, dim=1, descending=True, stable=True)[1]
    return order[:, :K].sort(dim=1)[0]


def _kp_operands(seed, B, C, N, with_p=True, ties=0, K=0):
    g = torch.Generator().manual_seed(seed)
    emb = torch.rand((B, C, N), generator=g) * 2 - 1
    emb_p = (torch.rand((B, C, N), generator=g) * 2 - 1) if with_p else None
    xyz = torch.rand((B, 3, N), generator=g) - 0.5
    if ties:
        # `ties` copies of the column of rank K - 1 at scattered places, some before and some behind it: exact ties straddle rank K
        _, key = _keys_cpu(emb, emb_p)
        order = torch.sort(key, dim=1, descending=True, stable=True)[1]
        for b in range(B):
            at = order[b, K - 1]
            for dst in order[b, K + 1:K + 1 + ties]:
                emb[b, :, dst] = emb[b, :, at]
                if emb_p is not None:
                    emb_p[b, :, dst] = emb_p[b, :, at]
    return emb, emb_p, xyz


@pytest.mark.parametrize("B,C,N,K,with_p,ties", [(3, 16, 100, 37, True, 0), (2, 64, 257, 256, True, 0), (2, 48, 70, 70, True, 0),
                                                  (2, 16, 1, 1, True, 0), (3, 16, 100, 37, False, 0), (2, 32, 1500, 700, True, 0),
                                                  (2, 16, 16384, 8000, True, 0),      # 82 KiB of LDS: the raised limit
                                                  (1, 16, 9000, 4500, False, 0),      # keys longer than the gather tiles' area
                                                  (3, 16, 100, 37, True, 5)])
def test_keypoints_kernel(B, C, N, K, with_p, ties):
    _, P = _mods()
    emb, emb_p, xyz = _kp_operands(B * 1000 + N + K, B, C, N, with_p, ties, K)
    e, key = _keys_cpu(emb, emb_p)
    want = _select_cpu(key, K)
    if ties:
        kth = torch.gather(key, 1, torch.sort(key, dim=1, descending=True, stable=True)[1][:, K - 1:K])
        n_eq = (key == kth).sum(dim=1)
        assert bool((n_eq >= ties + 1).all())
        assert all(int((key[b][want[b]] == kth[b]).sum()) < int(n_eq[b]) for b in range(B))       # some twins stay out: lowest index wins
    idx, xyz_k, emb_k, mean = P.keypoints(*_dev([emb, emb_p, xyz]), K, want_idx=True)
    torch.cuda.synchronize()
    assert torch.equal(idx.cpu(), want)
    ix = want[:, None, :]
    e_k = torch.gather(e, 2, ix.expand(-1, C, -1))
    assert torch.equal(emb_k.cpu(), e_k) and torch.equal(xyz_k.cpu(), torch.gather(xyz, 2, ix.expand(-1, 3, -1)))
    m64 = e_k.double().mean(dim=2)
    if K == 1:
        assert torch.equal(mean.cpu(), e_k[:, :, 0])                                   # one term: no rounding on either side
    else:
        _ratio(f"mean B {B} C {C} N {N} K {K}", float((mean.cpu().double() - m64).abs().max()), float((e_k.mean(dim=2).double() - m64).abs().max()))
    # every optional output absent: the means alone, the same bits
    only = torch.empty_like(mean)
    _lib, _ = _mods()
    _lib.call(KP, *_dev([emb, emb_p, xyz]), B, C, N, K, None, None, None, only)
    assert torch.equal(only, mean)


# ------------------------------------------------------------------------------------------------------------------------------
# l3d_soft_correspondence_pair alone
def _pair_ops(se, te, src, tgt, temp):
    """the head's op sequence for both directions (models/prnet.py SVDHead) -> corr_ab [B,3,N], corr_ba [B,3,M]"""
    scores = torch.matmul(se.transpose(2, 1).contiguous(), te) / math.sqrt(se.shape[1])
    scaled = temp.view(-1, 1, 1) * scores
    ab = torch.matmul(tgt, torch.softmax(scaled, dim=2).transpose(2, 1).contiguous())
    ba = torch.matmul(src, torch.softmax(scaled, dim=1))
    return ab, ba, float((temp.view(-1, 1, 1) * scores).abs().max())


def _pair_operands(seed, B, C, N, M):
    g = torch.Generator().manual_seed(seed)
    se, te = (torch.rand((B, C, N), generator=g) * 2 - 1) * 1.5, (torch.rand((B, C, M), generator=g) * 2 - 1) * 1.5
    src, tgt = torch.rand((B, 3, N), generator=g) - 0.5, torch.rand((B, 3, M), generator=g) - 0.5
    temp = torch.tensor([0.01, 1.0, 100.0])[:B].clone()
    return se, te, src, tgt, temp


@pytest.mark.parametrize("C,N,M", [(16, 70, 37), (64, 64, 64), (512, 256, 192), (48, 37, 130), (16, 200, 150), (16, 333, 530)])
def test_soft_correspondence_pair_kernel(C, N, M):
    """per-cloud temperatures 0.01, 1 and 100 in one batch (a kernel reading temperature[0] for every cloud fails), logits up to
    a few hundred; C 16 with three and more key tiles in both directions and ragged last query blocks is the shape at which a tile has
    ONE staged chunk, so the next tile's values are put while a slower wave may still read the previous tile's; per direction 4 x
    the gap of torch's fp32 op sequence against fp64 on the same operands"""
    _, P = _mods()
    B = 3
    ops = _pair_operands(C + N + M, B, C, N, M)
    ab32, ba32, top = _pair_ops(*ops)
    ab64, ba64, _ = _pair_ops(*[t.double() for t in ops])
    print(f"C {C} N {N} M {M}: largest |logit| {top:.0f}")
    assert top > 100
    dev = _dev(ops)
    ab, ba = P.soft_correspondence_pair(*dev)
    torch.cuda.synchronize()
    for b in range(B):
        print(f"  cloud {b} (temperature {float(ops[4][b])}): ab error {pf.err(ab[b], ab64[b]):.2e} torch {pf.err(ab32[b], ab64[b]):.2e}, "
              f"ba error {pf.err(ba[b], ba64[b]):.2e} torch {pf.err(ba32[b], ba64[b]):.2e}")
    _ratio(f"corr_ab C {C} N {N} M {M}", pf.err(ab, ab64), pf.err(ab32, ab64))
    _ratio(f"corr_ba C {C} N {N} M {M}", pf.err(ba, ba64), pf.err(ba32, ba64))
    # one output NULL: the other one's bits do not change
    _lib, _ = _mods()
    one_ab, one_ba = torch.empty_like(ab), torch.empty_like(ba)
    _lib.call(PAIR, *dev, B, C, N, M, None, one_ab, None)
    _lib.call(PAIR, *dev, B, C, N, M, None, None, one_ba)
    assert torch.equal(one_ab, ab) and torch.equal(one_ba, ba)


# ------------------------------------------------------------------------------------------------------------------------------
# the fused tail and the whole model on the fixture
@pytest.mark.parametrize("name", ["m1", "m3", "m4"])
def test_fused_tail_from_the_fixtures_keypoint_embeddings(name):
    """temperature head -> pair kernel -> Kabsch from the fp64 keypoint embeddings of iteration 0, rounded to fp32"""
    from learning3d_amd.utils.svd import kabsch
    _, P = _mods()
    q64, _, (se, te, src, tgt, temp64) = pf.reference64(name)
    net = pf.model(name).to(DEV)
    se, te, src, tgt = _dev([t.float() for t in (se, te, src, tgt)])
    Bn, C, K = se.shape
    with torch.no_grad():
        _, _, _, ms = P.keypoints(se, None, src, K)                    # K == N: the means alone matter here
        _, _, _, mt = P.keypoints(te, None, tgt, K)
        temperature = net.temp_net.rows(torch.abs(ms - mt))
        ab, ba = P.soft_correspondence_pair(se, te, src, tgt, temperature)
        Rab, tab = kabsch(src, ab)
        Rba, tba = kabsch(tgt, ba)
    _ratio(f"{name} temperature", pf.err(temperature, temp64.reshape(-1)), pf.gap(f"{name}_temperature"))
    for key, got in (("R_ab0", Rab), ("t_ab0", tab), ("R_ba0", Rba), ("t_ba0", tba)):
        _ratio(f"{name} {key}", pf.err(got, q64[key]), pf.gap(f"{name}_{key}"))


def _run_model(net, ins):
    net.keypoint_log = []
    out = net(*[t for t in ins if t is not None])
    return out, net.keypoint_log


# Bars of the whole-model quantities, in gaps.  4 unless the device op-sequence route -- which runs none of the new kernels -- itself
# measures above 4 on that quantity: then the bar on BOTH routes is twice that route's measured ratio (LABLOG R21.1).
#        (case, quantity): (op-sequence route's measured ratio, bar)
BARS = {("m1", "est_R"): (12.97, 25.94), ("m1", "est_t"): (14.91, 29.82), ("m1", "transformed_source"): (11.06, 22.12)}
# (m1 on the fused route measured 0.45 / 0.45 / 0.33; every other case and quantity measured 0.13-2.25 on both routes.  On m1 the
# op-sequence route's head is as exact on the device as on the CPU, call by call, and no keypoint set differs from the fp64 run's; the
# error enters with the embedding of the transformed source in iteration 1, code both routes share.)


def _bar(name, q):
    return BARS.get((name, q), (None, GAP_FACTOR))[1]


@pytest.mark.parametrize("name", [c[0] for c in pf.CASES])
def test_whole_model_both_routes_on_the_fixture(name):
    net = pf.model(name).to(DEV)
    ins = _dev(pf.inputs(name))
    ranked = pf.case(name)[1][4] != pf.case(name)[1][5]
    r = _Ratios()
    for route, fused in (("fused", True), ("op sequence", False)):
        (out, kp), log = _logged(lambda: _run_model(net, ins), fused=fused)
        new = [c for c in log if c.startswith(KP) or c.startswith(PAIR)]
        assert bool(new) == fused, (route, sorted(set(log)))
        if fused:
            iters = pf.case(name)[1][6]
            assert len([c for c in new if c.startswith(KP)]) == 2 * iters and len([c for c in new if c.startswith(PAIR)]) == iters
        if ranked:
            assert torch.equal(kp[0][0].cpu(), pf.stored(f"{name}_kp_src")) and torch.equal(kp[0][1].cpu(), pf.stored(f"{name}_kp_tgt"))
        for q in OUTPUTS:
            if q in out:
                r.add(f"{name} {route} {q}", pf.err(out[q], pf.truth(name, q)), pf.gap(f"{name}_{q}"), _bar(name, q))
        T = out["est_T"]
        assert torch.equal(T[:, :3, :3], out["est_R"]) and torch.equal(T[:, :3, 3], out["est_t"])
    r.hold()


# ------------------------------------------------------------------------------------------------------------------------------
# routing and contract
def _against_cpu(name, what, prepare, ins_of=lambda ins: ins, grad=False, bar=None):
    """the module `prepare` makes of the case's model, on the device and on the CPU, on the same inputs: none of the new entry
    points run, and the device run is within 4 gaps of the CPU run"""
    cpu = prepare(pf.model(name))
    dev = copy.deepcopy(cpu).to(DEV)
    ins = [t for t in pf.inputs(name) if t is not None]
    with torch.set_grad_enabled(grad):
        want = cpu(*ins_of([t.clone() for t in ins]))
    got, log = _logged(lambda: dev(*ins_of(_dev(ins))), grad=grad)
    assert not [c for c in log if c.startswith(KP) or c.startswith(PAIR)], (what, sorted(set(log)))
    r = _Ratios()
    for q in OUTPUTS:
        if q in got:
            r.add(f"{name} {what} {q}", pf.err(got[q], want[q].detach().double()), pf.gap(f"{name}_{q}"), bar or _bar(name, q))
    r.hold()


def test_route_fp64():
    def ins_of(ins):
        return [t.double() for t in ins]
    _against_cpu("m1", "fp64", lambda net: net.double(), ins_of, bar=GAP_FACTOR)       # (not m1's whole-model bars)


def test_route_requires_grad():
    def ins_of(ins):
        return [ins[0].requires_grad_(True)] + ins[1:]
    _against_cpu("m4", "requires_grad", lambda net: net, ins_of, grad=True)


def test_route_train_mode_batchnorm():
    _against_cpu("m4", "train mode", lambda net: net.train())


def test_route_gumbel_softmax(monkeypatch):
    """The CPU and the device generators draw different streams, so both runs take the sampler's noise from one seeded CPU generator
    (the hard one-hot of F.gumbel_softmax: arg-max of (logits + Gumbel noise) / tau).  m3: one iteration at emb 512, the case whose
    correspondences are best conditioned; with the noise left out nearly every point of a seeded model picks the same partner and H
    is close to rank one (measured on m4: the two runs' est_R 1.98 apart)."""
    import torch.nn.functional as F
    gens = []

    def seeded_noise(logits, tau=1, hard=False, eps=1e-10, dim=-1):
        u = torch.rand(logits.shape, generator=gens[-1]).clamp_min(1e-20)
        y = (logits + (-torch.log(-torch.log(u))).to(logits)) / tau
        return torch.zeros_like(y).scatter_(dim, y.argmax(dim, keepdim=True), 1.0)
    monkeypatch.setattr(F, "gumbel_softmax", seeded_noise)

    def prepare(net):
        net.head.cat_sampler = 'gumbel_softmax'
        return net

    def ins_of(ins):
        gens.append(torch.Generator().manual_seed(77))             # the same stream for the CPU run and the device run
        return ins
    _against_cpu("m3", "gumbel_softmax", prepare, ins_of)


def _truth_of(net, ins):
    with torch.no_grad():
        return copy.deepcopy(net).cpu().double()(*[t.cpu().double() for t in ins])


def test_folded_weight_caches_follow_load_state_dict_and_in_place_edits():
    name = "m1"
    net = pf.model(name).to(DEV)
    ins = [t for t in _dev(pf.inputs(name)) if t is not None]
    outs, r = [], _Ratios()

    def check(what):
        out, _ = _logged(lambda: net(*ins))
        want = _truth_of(net, ins)
        for q in ("est_R", "est_t"):
            r.add(f"{name} {what} {q}", pf.err(out[q], want[q]), pf.gap(f"{name}_{q}"), GAP_FACTOR)      # (not m1's whole-model bars)
        if outs:
            moved = pf.err(out["est_R"], outs[-1]["est_R"].cpu().double()) / pf.gap(f"{name}_est_R")
            print(f"{what}: est_R moved by {moved:.0f} gaps")
            assert moved > 100
        outs.append(out)
    check("as built")
    state = {k: v.clone() for k, v in net.state_dict().items()}
    state["temp_net.nn.9.bias"] += 4.0
    net.load_state_dict(state, strict=True)
    check("after load_state_dict")
    with torch.no_grad():
        net.temp_net.nn[7].weight.mul_(1.5)                    # a BatchNorm scale inside a folded layer of the temperature head
        net.temp_net.nn[9].bias.add_(6.0)
    check("after an in-place edit")
    r.hold()


def _capture(run, keys):
    """run() eagerly, once on a side stream as a warm-up, then captured into one graph on one stream and replayed twice over stale
    outputs -> the launch log of the capture; every replay gives the eager bits"""
    _lib, _ = _mods()
    with torch.no_grad():
        first = run()
        eager = [first[k].clone() for k in keys]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()                                                        # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        _lib.LAUNCH_LOG = log = []
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                res = run()
        finally:
            _lib.LAUNCH_LOG = None
        out = [res[k] for k in keys]
        for replay in range(2):
            for v in out:
                v.fill_(7)                                               # stale values must not survive a replay
            graph.replay()
            torch.cuda.synchronize()
            for k, a, b in zip(keys, out, eager):
                assert torch.equal(a, b), (replay, k)
    return log


def _every_point_a_keypoint():
    """PointNet, Identity attention, emb 64, 64 points, K == N, two iterations, seeded and rescaled like case m4"""
    _, P = _mods()
    net = P.PRNet(emb_nn="pointnet", attention="identity", emb_dims=64, num_keypoints=64, num_subsampled_points=64, num_iters=2)
    return pf.rescale(pf.seeded_params(net, pf.seed() + 3), 20.0).eval()


@pytest.mark.parametrize("name", ["m3", "m4", "K == N"])
def test_forward_fused_replays_from_one_graph(name):
    """the whole fused forward captured into one graph on one stream and replayed twice gives the eager bits: no host read.  m3:
    DGCNN, pointer network, ranked keypoints; m4: PointNet, Identity attention, the loss; K == N: the keypoint kernel's copy route"""
    if name == "K == N":
        net, ins = _every_point_a_keypoint().to(DEV), _dev(pf.clouds("m4", pf.seed())[:2])
    else:
        net, ins = pf.model(name).to(DEV), [t for t in _dev(pf.inputs(name)) if t is not None]
    keys = ("est_R", "est_t", "est_T", "transformed_source") + (("loss",) if len(ins) == 4 else ())
    log = _capture(lambda: net(*ins), keys)
    assert any(c.startswith(KP) for c in log) and any(c.startswith(PAIR) for c in log)


def test_keypoints_above_64_kib_of_lds_capture_into_a_graph():
    """N 16384, K 8000 needs 82 KiB of dynamic LDS: the entry point raises the kernel's limit (hipFuncSetAttribute) on every such
    call, also while a stream is capturing"""
    _, P = _mods()
    B, C, N, K = 2, 16, 16384, 8000
    ops = _dev(_kp_operands(21, B, C, N))

    def run():
        idx, xyz_k, emb_k, mean = P.keypoints(*ops, K, want_idx=True)
        return dict(idx=idx, xyz_k=xyz_k, emb_k=emb_k, mean=mean)
    assert [c for c in _capture(run, ("idx", "xyz_k", "emb_k", "mean")) if c.startswith(KP)]


def test_fused_forward_on_clouds_of_different_sizes():
    """N 64 against M 50 with every point a keypoint (K == N, K == M): two emb_nn calls, keypoint launches of two sizes, a pair launch
    with N != M and two Kabsch launches per iteration; against the CPU fp64 run of the same module, in gaps of case m4 (the same
    embedding, attention, width and temperature bias)"""
    name = "m4"
    cpu = _every_point_a_keypoint()
    src, tgt, _, _ = pf.clouds(name, pf.seed())
    tgt = tgt[:, :50].contiguous()
    with torch.no_grad():
        want = copy.deepcopy(cpu).double()(src.double(), tgt.double())
    dev = copy.deepcopy(cpu).to(DEV)
    r = _Ratios()
    for route, fused in (("fused", True), ("op sequence", False)):
        out, log = _logged(lambda: dev(src.to(DEV), tgt.to(DEV)), fused=fused)
        if fused:
            assert len([c for c in log if c.startswith(KP)]) == 4 and len([c for c in log if c.startswith(PAIR)]) == 2
            assert len([c for c in log if c.startswith("l3d_kabsch")]) == 4
        else:
            assert not [c for c in log if c.startswith(KP) or c.startswith(PAIR)]
        assert out["transformed_source"].shape == src.shape
        for q in ("est_R", "est_t", "transformed_source"):
            r.add(f"N 64, M 50 {route} {q}", pf.err(out[q], want[q]), pf.gap(f"{name}_{q}"), GAP_FACTOR)
    r.hold()


_SCRATCH = {PAIR: {"workspace": mc.Spec("scratch", "workspace: l3d_soft_correspondence_pair_workspace_bytes(B,N,M) bytes of scratch",
                                        size=(PAIR + "_workspace_bytes", lambda v: (v["B"], v["N"], v["M"]), 1))}}


@pytest.mark.parametrize("K", [37, 70])
def test_memory_contract_keypoints(K):
    """guards, two fills, const inputs unchanged; tails in N, K and C, ranked and K == N, with and without the optional outputs"""
    _lib, P = _mods()
    B, C, N = 2, 24, 70
    emb, emb_p, xyz = _dev(_kp_operands(5, B, C, N))
    got = mc.check(KP, lambda ar: [emb, emb_p, xyz, B, C, N, K, ar.out(torch.int64, B, K), ar.f32(B, 3, K), ar.f32(B, C, K), ar.f32(B, C)],
                   proto=_lib.EXT_PROTOTYPES[KP])
    idx, xyz_k, emb_k, mean = P.keypoints(emb, emb_p, xyz, K, want_idx=True)
    assert torch.equal(got["idx"], idx) and torch.equal(got["xyz_k"], xyz_k) and torch.equal(got["emb_k"], emb_k) and torch.equal(got["mean"], mean)
    alone = mc.check(KP, lambda ar: [emb, None, xyz, B, C, N, K, None, None, None, ar.f32(B, C)], proto=_lib.EXT_PROTOTYPES[KP])
    assert alone["mean"].shape == mean.shape


@pytest.mark.parametrize("outputs", ["both", "ab", "ba"])
def test_memory_contract_soft_correspondence_pair(outputs):
    _lib, P = _mods()
    B, C, N, M = 2, 48, 70, 37
    ops = _dev(_pair_operands(11, B, C, N, M))
    nbytes = int(_lib.lib().l3d_soft_correspondence_pair_workspace_bytes(B, N, M))

    def build(ar):
        return [*ops, B, C, N, M, ar.bytes(nbytes) if nbytes else None, ar.f32(B, 3, N) if outputs != "ba" else None,
                ar.f32(B, 3, M) if outputs != "ab" else None]
    got = mc.check(PAIR, build, proto=_lib.EXT_PROTOTYPES[PAIR], contract=_SCRATCH)
    ab, ba = P.soft_correspondence_pair(*ops)
    assert outputs == "ba" or torch.equal(got["corr_ab"], ab)
    assert outputs == "ab" or torch.equal(got["corr_ba"], ba)
