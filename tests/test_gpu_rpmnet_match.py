"""RPMNet's matching stage on HIP, on the GPU (models/rpmnet.py RPMNet._Match, rpmnet_match.hip, include/ext/l3d_rpmnet_match.h).

1. the kernels at their edges against the fp64 statement of the formulas (golden/rpmnet_match_fixture.py, which the CPU tests hold
   to torch.autograd): J around the four rows of a workgroup, K around a wave and the 64 columns of a column workgroup, n_iters
   0, 1, 2, 5, pointers on and one element off a 16-byte boundary, each cotangent alone and all four, with and without the fold.
2. RPMNet._Match's gradients of dist, beta, alpha against the CPU fp64 op sequence.
3. RPMNet's plumbing: two iterations, the bench's loss, every parameter gradient against the CPU fp64 one and against the
   MATCH_HIP = False run of the same build; the launch log of both.
4. route and state.  5. the peak allocation of the stage against the op sequence's.  6. the memory contract."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import memory_contract as mc            # noqa: E402
import rpmnet_match_fixture as mf       # noqa: E402
import rpmnet_train_fixture as tf       # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEW = ("l3d_sinkhorn_slack_keep", "l3d_sinkhorn_slack_backward")
ULP = 2.0 ** -23
GIVEN = [(c,) for c in mf.COTANGENTS] + [mf.COTANGENTS]


def _mods():
    from learning3d_amd import _lib
    from learning3d_amd.models import _fused, rpmnet
    return _lib, _fused, rpmnet


class _log:
    def __enter__(self):
        _lib = _mods()[0]
        _lib.LAUNCH_LOG = self.log = []
        return self.log

    def __exit__(self, *exc):
        _mods()[0].LAUNCH_LOG = None
        return False


class _switch:
    """`with _switch(False):` -- rpmnet.MATCH_HIP for the calls inside"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        rpmnet = _mods()[2]
        self.prev, rpmnet.MATCH_HIP = rpmnet.MATCH_HIP, self.value

    def __exit__(self, *exc):
        _mods()[2].MATCH_HIP = self.prev
        return False


def _offset(t):
    """the same values at a data pointer one element past a 16-byte boundary"""
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert flat.data_ptr() % 16 == 0
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


def _rounded_once(got, want64, what, floor=0.0):
    """2^-23 |want| + 1e-12 max |want| per element; floor: see test_kernels_at_their_edges -> (error, bar) at the worst element"""
    err = (got.double() - want64).abs()
    bar = ULP * want64.abs() + max(1e-12 * float(want64.abs().max()), floor)
    assert bool((err <= bar).all()), (what, float(err.max()), float(want64.abs().max()), floor)
    return float((err - ULP * want64.abs()).max())


# ------------------------------------------------------------------------------------------------------------------------------
# (J, K, B): J around the 4 rows of a workgroup, K around a wave's 64 lanes / a column workgroup's 64 columns, K % 4 == 0 and not
SHAPES = {0: [(1, 1, 2), (4, 64, 3), (5, 65, 2), (9, 130, 2)],
          1: [(1, 63, 2), (3, 64, 3), (4, 65, 2), (5, 130, 2), (9, 1, 3), (9, 64, 2)],
          2: [(1, 130, 2), (3, 1, 2), (4, 63, 3), (5, 64, 2), (9, 65, 2)],
          5: [(1, 64, 2), (3, 65, 2), (4, 130, 3), (5, 63, 2), (9, 64, 2), (4, 1, 2), (3, 128, 2)]}


@pytest.mark.parametrize("n", [0, 1, 2, 5])
def test_kernels_at_their_edges(n):
    """keep's four outputs are l3d_sinkhorn_slack's bits, its potentials the fixture's to 2^-50 of their largest value, and d_out,
    d_beta, d_alpha one rounding of the fixture's fp64 values: 2^-23 |want| + max(1e-12 max |want|, floor) per element.
    The floor.  The kernels and the fixture add the same fp64 terms in different orders, and where the terms cancel (a row whose mass
    sits on one entry near +200: G's terms, the reverse sweep's and the sums behind d_alpha cancel to a small share of their size)
    1e-12 of the result is less than 2^-53 of the terms.  That gap is measured without the kernels, by evaluating the fixture twice,
    its sums once as torch takes them and once as running sums from the far end, the three-term sums in the exponents associated
    the other way round (rpmnet_match_fixture.reordered64, in fp64 torch on the device the test runs on), per case and per tensor;
    the floor is 16 times it.  A reordering cannot see that two exponential routines differ in the last bit of every term, and on a
    shape with nothing to reorder (J = K = 1) it measures exactly zero: the gap is therefore taken as no less than 2^-53 of the
    largest sum of absolute terms behind an element (backward64(terms=True)), one fp64 rounding of what was added.  Affinities reach -200 in half of the cases and
    +-200 in the other half; with n_iters = 0 they reach +-70, because P = exp(affinity) itself must stay inside fp32's range for
    the forward's perm and for d_out.
    Measured on an MI355X (LABLOG.md R24.1), relative to the largest sum of absolute terms behind an element of the tensor, for n_iters
    0, 1, 2, 5: the fixture's largest reordering gap 1.8e-16, 1.3e-15, 1.0e-15, 1.1e-15; the kernels' largest error beyond one fp32
    rounding of the value 8.1e-17, 5.0e-17, 1.4e-17, 2.4e-17 (the test prints both).  With the gap from reordering the reductions
    alone and no 2^-53 term, d_alpha missed the bar in four cases of the +-200 family: errors of 6e-18 to 1e-14 on values below
    2e-7, where that reordering measured 0 to 4e-15."""
    _lib, _, rpmnet = _mods()
    worst_gap = worst_excess = 0.0
    for i, (J, K, B) in enumerate(SHAPES[n]):
        both = bool(i % 2)
        case = mf.match_case(7000 + 100 * n + i, B, J, K, amax=60.0 if n == 0 else 200.0, both_signs=both, dev=DEV)
        A, x = mf.affinity32(case).contiguous(), case["xyz_ref"]
        ws = torch.empty(_lib.lib().l3d_sinkhorn_workspace_bytes(B, J, K) // 8, dtype=torch.float64, device=DEV)
        ref = [torch.empty_like(A), torch.empty_like(A), torch.empty((B, J), device=DEV), torch.empty((B, J, 3), device=DEV)]
        _lib.call("l3d_sinkhorn_slack", A, B, J, K, n, x, mf.EPS, *ref, ws)
        pots = []
        for shift in (False, True):
            AA = _offset(A) if shift else A
            out = [torch.full_like(t, float("nan")) for t in ref]
            pot = torch.full((n, B, J + K), float("nan"), dtype=torch.float64, device=DEV)
            _lib.call("l3d_sinkhorn_slack_keep", AA, B, J, K, n, x, mf.EPS, *out, pot if n else None)
            assert all(torch.equal(a, b) for a, b in zip(out, ref)), ("keep's outputs", J, K, n, shift)
            pots.append(pot)
        assert torch.equal(pots[0], pots[1])
        pot = pots[0]
        want_pot = mf.forward64(A, n)[0]
        if n:
            assert float((pot - want_pot).abs().max()) <= 2.0 ** -50 * float(want_pot.abs().max()), ("potentials", J, K, n)
        perm, rowsum, weighted, pot2 = rpmnet.sinkhorn_slack_keep(A, n, x)
        assert torch.equal(perm, ref[1]) and torch.equal(rowsum, ref[2]) and torch.equal(weighted, ref[3]) and torch.equal(pot2, pot)
        for given in GIVEN:
            kw = {c: case[c] for c in given}
            want_dA, mag = mf.backward64(A, pot, x, terms=True, **kw)
            other = mf.reordered64(A, pot, x, **kw)
            want = {False: (want_dA, None, None), True: mf.fold64(want_dA, case["dist"], case["beta"], case["alpha"])}
            gap = {False: (want_dA - other, None, None),
                   True: [a - b for a, b in zip(want[True], mf.reordered_fold64(other, case["dist"], case["beta"], case["alpha"]))]}
            terms = {False: (mag, None, None), True: mf.fold_terms64(mag, case["dist"], case["beta"], case["alpha"])}
            for fold in (False, True):
                trio = {c: case[c] for c in ("dist", "beta", "alpha")} if fold else {}
                for shift in (False, True):
                    kk = {c: _offset(t) if (shift and t.dim() == 3 and t.shape[2] == K) else t for c, t in {**kw, **trio}.items()}
                    got = rpmnet.sinkhorn_slack_backward(_offset(A) if shift else A, pot, x, mf.EPS, want_beta=fold, want_alpha=fold, **kk)
                    for what, g, w, d, m in zip(("d_out", "d_beta", "d_alpha"), got, want[fold], gap[fold], terms[fold]):
                        if w is None:
                            assert g is None
                            continue
                        scale = float(m.max())                                  # the largest sum of absolute terms
                        g16 = 16.0 * max(float(d.abs().max()), 2.0 ** -53 * scale)
                        excess = _rounded_once(g, w, (what, J, K, B, n, given, fold, shift, both), floor=g16)
                        worst_gap, worst_excess = max(worst_gap, g16 / 16.0 / scale), max(worst_excess, excess / scale)
    print(f"\nn_iters {n}: relative to the largest sum of absolute terms behind an element, the fixture's largest reordering gap "
          f"{worst_gap:.1e}, the kernels' largest error beyond one fp32 rounding {worst_excess:.1e}")


def test_d_out_at_an_offset_output_and_optional_fold_outputs():
    """d_out itself off a 16-byte boundary (the output pass's scalar route), and the trio with d_beta alone, d_alpha alone, neither:
    d_out is the same bits, the fold output that is asked for too"""
    _lib, _, rpmnet = _mods()
    B, J, K, n = 2, 5, 64, 2
    case = mf.match_case(11, B, J, K, dev=DEV)
    A, x = mf.affinity32(case).contiguous(), case["xyz_ref"]
    pot = rpmnet.sinkhorn_slack_keep(A, n, x)[3]
    kw = {c: case[c] for c in mf.COTANGENTS}
    trio = {c: case[c] for c in ("dist", "beta", "alpha")}
    full = rpmnet.sinkhorn_slack_backward(A, pot, x, mf.EPS, want_beta=True, want_alpha=True, **kw, **trio)
    for wb, wa in ((True, False), (False, True), (False, False)):
        got = rpmnet.sinkhorn_slack_backward(A, pot, x, mf.EPS, want_beta=wb, want_alpha=wa, **kw, **trio)
        assert torch.equal(got[0], full[0]) and (got[1] is None) == (not wb) and (got[2] is None) == (not wa)
        assert (not wb or torch.equal(got[1], full[1])) and (not wa or torch.equal(got[2], full[2]))
    ws = torch.empty(_lib.lib().l3d_sinkhorn_backward_workspace_bytes(B, J, K, n) // 8, dtype=torch.float64, device=DEV)
    d_off = _offset(torch.empty_like(A))
    _lib.call("l3d_sinkhorn_slack_backward", A, pot, B, J, K, n, x, mf.EPS, kw["d_perm"], kw["d_rowsum"], kw["d_weighted"], kw["d_affinity"],
              trio["dist"], trio["beta"], trio["alpha"], d_off, None, None, ws)
    want = mf.fold64(mf.backward64(A, pot, x, **kw), case["dist"], case["beta"], case["alpha"])[0]
    _rounded_once(d_off, want, "d_out off a 16-byte boundary")
    _rounded_once(full[0], want, "d_out")


# ------------------------------------------------------------------------------------------------------------------------------
def _exact_case(seed, B=2, J=50, K=64):
    """a case whose fp32 affinity is exact: dist and alpha multiples of 2^-10 in [0, 4], beta a power of two.  -beta (dist - alpha)
    then has no rounding in fp32, so RPMNet._Match (which differentiates the fp64 function of the fp32 affinity) and the fp64 op
    sequence (which forms the affinity in fp64) differentiate the same function, and the kernels' own error is all that is left"""
    g = torch.Generator().manual_seed(seed)
    q = lambda t: torch.round(t * 1024.0) / 1024.0                               # noqa: E731
    dist = q((1.0 + 0.25 * torch.randn((B, J, K), generator=g)).clamp_(0.0, 4.0))
    beta = torch.tensor([4.0, 8.0])[:B].clone()
    alpha = q(0.9 + 0.2 * torch.rand((B,), generator=g))
    case = {"dist": dist, "beta": beta, "alpha": alpha, "xyz_ref": torch.rand((B, K, 3), generator=g) * 2 - 1,
            "d_perm": torch.randn((B, J, K), generator=g), "d_rowsum": torch.randn((B, J), generator=g),
            "d_weighted": torch.randn((B, J, 3), generator=g), "d_affinity": torch.randn((B, J, K), generator=g)}
    assert torch.equal(mf.affinity32(case).double(), -beta.double()[:, None, None] * (dist.double() - alpha.double()[:, None, None]))
    return case


def test_match_function_against_the_fp64_op_sequence():
    _lib, _, rpmnet = _mods()
    case = _exact_case(3)
    want = mf.autograd64(case, 5, mf.COTANGENTS, fold=True)
    leaves = [case[n].to(DEV).requires_grad_() for n in ("dist", "beta", "alpha")]
    with _log() as log:
        outs = rpmnet.RPMNet._Match.apply(*leaves, case["xyz_ref"].to(DEV), 5)
        names = ("d_affinity", "d_perm", "d_rowsum", "d_weighted")
        got = torch.autograd.grad(sum((o * case[c].to(DEV)).sum() for o, c in zip(outs, names)), leaves)
    assert log == list(NEW)
    assert torch.equal(outs[0], mf.affinity32(case).to(DEV))
    print("\nRPMNet._Match, B 2, J 50, K 64, 5 iterations: max |gradient - fp64 op sequence| / max |fp64|")
    for what, g, w in zip(("dist", "beta", "alpha"), got, want):
        print(f"  {what:<6} {float((g.cpu().double() - w).abs().max()) / float(w.abs().max()):.2e}")
    err = float((got[0].cpu().double() - want[0]).abs().max()) / float(want[0].abs().max())
    assert err <= mf.TIER, ("dist", err)
    _rounded_once(got[1].cpu(), want[1], "beta")
    _rounded_once(got[2].cpu(), want[2], "alpha")


# ------------------------------------------------------------------------------------------------------------------------------
def test_rpmnet_trains_through_the_matching_unit():
    _lib, _fused, rpmnet = _mods()
    cpu_net, t, s, igt = tf.plumbing_case()
    n64, dnet = copy.deepcopy(cpu_net).double(), copy.deepcopy(cpu_net).to(DEV)
    g64 = tf.plumbing_gradients(n64, t.double(), s.double(), igt.double())
    td, sd, igtd = t.to(DEV), s.to(DEV), igt.to(DEV)
    with _log() as log:
        hip = tf.plumbing_gradients(dnet, td, sd, igtd)
    assert log.count("l3d_sinkhorn_slack_keep") == 2 and log.count("l3d_sinkhorn_slack_backward") == 2
    assert "l3d_sinkhorn_slack" not in log and "l3d_rigid_transform_weighted" not in log
    with _switch(False), _log() as log_seq:
        seq = tf.plumbing_gradients(dnet, td, sd, igtd)
    assert not any(name in log_seq for name in NEW) and "l3d_gn_backward_apply" in log_seq
    failed = []
    print("\nRPMNet, 2 iterations: max |gradient - fp64| / max |fp64|")
    print(f"  {'tensor':<34} {'MATCH_HIP':>10} {'off':>11} {'on - off':>10} {'gap':>10} {'bar':>10}")
    for n, want in g64.items():
        scale = float(want.abs().max())
        gap = tf.PLUMBING_GAPS[n]
        bar = max(tf.GAP_FACTOR * gap, tf.TIER)
        e_hip = float((hip[n].cpu().double() - want).abs().max()) / scale
        e_seq = float((seq[n].cpu().double() - want).abs().max()) / scale
        between = float((hip[n].double() - seq[n].double()).abs().max()) / scale
        print(f"  {n:<34} {e_hip:>10.2e} {e_seq:>11.2e} {between:>10.2e} {gap:>10.2e} {bar:>10.1e}")
        if not (e_hip <= bar and between <= bar):
            failed.append((n, e_hip, e_seq, between, gap, bar))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------------------------
def _stage(net, dist, beta, alpha, x, weights):
    """forward and backward of the matching stage on leaves -> (outputs, gradients of dist, beta, alpha)"""
    leaves = [t.detach().clone().requires_grad_(r) for t, r in zip((dist, beta, alpha), weights)]
    aff, perm, rowsum, wt = net.match_stage(leaves[0], leaves[1], leaves[2], x)
    rows = rowsum if rowsum is not None else torch.sum(perm, dim=2)
    loss = perm.sum(2).mean() + (wt * wt).sum() + rows.sum() * 0.5
    grads = torch.autograd.grad(loss, [l for l in leaves if l.requires_grad])
    return (aff.detach(), perm.detach(), wt.detach()), list(grads)


def test_route_and_state(monkeypatch):
    _lib, _fused, rpmnet = _mods()
    net = rpmnet.RPMNet()
    asked, real = [], rpmnet.sinkhorn_slack_backward
    monkeypatch.setattr(rpmnet, "sinkhorn_slack_backward",
                        lambda *a, **k: (asked.append((k["want_beta"], k["want_alpha"], [g is not None for g in a[4:8]])), real(*a, **k))[1])
    case = mf.match_case(21, 2, 50, 64, amax=20.0, dev=DEV)
    args = (case["dist"], case["beta"], case["alpha"], case["xyz_ref"])
    with _log() as log:
        out1, g1 = _stage(net, *args, (True, True, True))
    assert log == list(NEW), "one forward launch list and ONE backward call: the stride-0 d_perm, d_rowsum and d_weighted together"
    torch.empty(1 << 20, device=DEV).fill_(float("nan"))                         # stale workspaces for the repeat
    out2, g2 = _stage(net, *args, (True, True, True))
    assert all(torch.equal(a, b) for a, b in zip(out1 + tuple(g1), out2 + tuple(g2))), "repeat forward and backward: the same bits"
    want = rpmnet.sinkhorn_slack(out1[0], net.num_sk_iter, xyz_ref=case["xyz_ref"], want_log=False, want_perm=True)
    assert torch.equal(out1[1], want[1]) and torch.equal(out1[2], want[3]), "the forward is the fused route's Sinkhorn, bit for bit"
    # a frozen parameter network: beta and alpha need no gradient -> no fold outputs, the same gradient of dist
    with _log() as log:
        _, g3 = _stage(net, *args, (True, False, False))
    assert log == list(NEW) and len(g3) == 1 and torch.equal(g3[0], g1[0])
    _, g4 = _stage(net, *args, (False, True, False))
    assert len(g4) == 1 and torch.equal(g4[0], g1[1])
    # (want_beta, want_alpha, [d_perm, d_rowsum, d_weighted, d_affinity given]) of the four backward calls so far
    assert asked == [(True, True, [True, True, True, False])] * 2 + [(False, False, [True, True, True, False]),
                                                                      (True, False, [True, True, True, False])]
    # a transposed-view dist, bit for bit and launch for launch against its contiguous clone
    view = case["dist"].transpose(1, 2).contiguous().transpose(1, 2)
    assert not view.is_contiguous()
    with _log() as log:
        out5, g5 = _stage(net, view, *args[1:], (True, True, True))
    assert log == list(NEW) and all(torch.equal(a, b) for a, b in zip(out1 + tuple(g1), out5 + tuple(g5)))
    # a stride-0 d_perm against its contiguous clone
    leaves = [t.detach().clone().requires_grad_() for t in args[:3]]
    outs = rpmnet.RPMNet._Match.apply(*leaves, args[3], 5)
    g = torch.randn((1, 1, 1), device=DEV).expand(2, 50, 64)
    a = torch.autograd.grad(outs[1], leaves, g, retain_graph=True)
    b = torch.autograd.grad(outs[1], leaves, g.contiguous())
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    # what the gate sends to the op sequence
    with _log() as log:
        _stage(net, *args[:3], args[3].clone().requires_grad_(), (True, True, True))
        with torch.no_grad():
            net.match_stage(*args)
        with _switch(False):
            _stage(net, *args, (True, True, True))
        _fused.TRAIN_HIP = False
        try:
            _stage(net, *args, (True, True, True))
        finally:
            _fused.TRAIN_HIP = True
    assert not any(name in log for name in NEW)


def test_a_template_that_requires_a_gradient_and_an_optimizer_step():
    _lib, _fused, rpmnet = _mods()
    cpu_net, t, s, igt = tf.plumbing_case()
    net, td, sd, igtd = cpu_net.to(DEV), t.to(DEV), s.to(DEV), igt.to(DEV)
    with _log() as log:
        tf.bench_loss(net(td.clone().requires_grad_(), sd, 1), igtd).backward()
    assert not any(name in log for name in NEW), "xyz_template.requires_grad_() sends the pair to the op sequence"
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    net.zero_grad(set_to_none=True)
    with _log() as log:
        first = net(td, sd, 1)
        tf.bench_loss(first, igtd).backward()
    assert log.count(NEW[0]) == 1 and log.count(NEW[1]) == 1
    opt.step()
    second = net(td, sd, 1)
    assert not torch.equal(second["perm_matrices"][0], first["perm_matrices"][0]) and not torch.equal(second["est_T"], first["est_T"])


def test_peak_allocation_is_below_the_op_sequence():
    _lib, _fused, rpmnet = _mods()
    net = rpmnet.RPMNet()
    case = mf.match_case(41, 2, 256, 256, amax=20.0, dev=DEV)
    args = (case["dist"], case["beta"], case["alpha"], case["xyz_ref"])
    peaks = {}
    for hip in (True, False, True):
        with _switch(hip):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            _stage(net, *args, (True, True, True))
            torch.cuda.synchronize()
            peaks[hip] = torch.cuda.max_memory_allocated() - base
    print(f"\nmatching stage forward + backward at B 2, J = K = 256: peak {peaks[True] / 2 ** 20:.2f} MiB on the HIP route, "
          f"{peaks[False] / 2 ** 20:.2f} MiB on the op sequence")
    assert peaks[True] < peaks[False]


# ------------------------------------------------------------------------------------------------------------------------------
_SCRATCH = {
    "l3d_sinkhorn_slack_backward": {"workspace": mc.Spec(
        "scratch", "`workspace`: SCRATCH of l3d_sinkhorn_backward_workspace_bytes(B, J, K, n_iters) bytes",
        size=("l3d_sinkhorn_backward_workspace_bytes", lambda v: (v["B"], v["J"], v["K"], v["n_iters"]), 1))},
}


def _contract(name, build):
    _lib = _mods()[0]
    return mc.check(name, build, proto=_lib.EXT_PROTOTYPES[name], contract=_SCRATCH)


@pytest.mark.parametrize("B,J,K,n", [(2, 5, 64, 2), (2, 9, 65, 2), (1, 4, 130, 0), (3, 3, 8, 0), (2, 70, 63, 2)])
def test_memory_contract(B, J, K, n):
    """the entry points: guards, two fills, const inputs unchanged, the workspace by its size function, potentials written in full.
    K a multiple of 4 (the 16-byte route) and not, n_iters 0 and 2, every subset of outputs the header allows"""
    _lib = _mods()[0]
    case = mf.match_case(60 + J, B, J, K, amax=20.0, dev=DEV)
    A, x = mf.affinity32(case).contiguous(), case["xyz_ref"]
    out = _contract("l3d_sinkhorn_slack_keep", lambda ar: [A, B, J, K, n, x, mf.EPS, ar.f32(B, J, K), ar.f32(B, J, K), ar.f32(B, J),
                                                           ar.f32(B, J, 3), ar.out(torch.float64, n, B, J + K)])
    pot = out["potentials"].clone()
    assert bool(torch.isfinite(pot).all()) and bool(torch.isfinite(out["perm"]).all())
    _contract("l3d_sinkhorn_slack_keep", lambda ar: [A, B, J, K, n, None, mf.EPS, None, ar.f32(B, J, K), None, None,
                                                     ar.out(torch.float64, n, B, J + K)])
    ws_bytes = _lib.lib().l3d_sinkhorn_backward_workspace_bytes(B, J, K, n)
    cot = [case[c] for c in mf.COTANGENTS]
    trio = [case["dist"], case["beta"], case["alpha"]]
    got = _contract("l3d_sinkhorn_slack_backward", lambda ar: [A, pot, B, J, K, n, x, mf.EPS, *cot, *trio, ar.f32(B, J, K), ar.f32(B), ar.f32(B),
                                                               ar.bytes(ws_bytes)])
    want = mf.fold64(mf.backward64(A, pot, x, **dict(zip(mf.COTANGENTS, cot))), *trio)
    for what, w in zip(("d_out", "d_beta", "d_alpha"), want):
        _rounded_once(got[what], w, (what, B, J, K, n))
    _contract("l3d_sinkhorn_slack_backward", lambda ar: [A, pot, B, J, K, n, x, mf.EPS, *cot, *trio, ar.f32(B, J, K), None, None,
                                                         ar.bytes(ws_bytes)])
    _contract("l3d_sinkhorn_slack_backward", lambda ar: [A, pot, B, J, K, n, None, mf.EPS, cot[0], None, None, None, None, None, None,
                                                         ar.f32(B, J, K), None, None, ar.bytes(ws_bytes)])
