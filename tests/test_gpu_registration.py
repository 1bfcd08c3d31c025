"""PointNetLK / iPCRNet on the MI355X, fused route (registration.hip) against the reference's fp64 results
(tests/golden/make_golden_registration.py) and against the op-sequence route of the same model."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_registration_cpu import T, close, seeded_ipcrnet, trained_pnlk      # noqa: E402

pytestmark = pytest.mark.gpu
SERIES_GAP_FACTOR = 4.0       # bar on est_T_series[i]: this many times the reference's own fp32-to-fp64 gap at step i


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def fused(net, fn):
    """run fn() and return (result, C-ABI calls made)"""
    from learning3d_amd import _lib
    _lib.LAUNCH_LOG = []
    try:
        with torch.no_grad():
            out = fn()
        return out, list(_lib.LAUNCH_LOG)
    finally:
        _lib.LAUNCH_LOG = None


def test_pointnetlk_trained_against_fp64(golden, dev):
    """Measured on the MI355X (LABLOG.md, registration): the largest ratio of our est_T_series error to the reference's own
    fp32-to-fp64 gap per step is printed below; the bar is 4."""
    z = golden("pnlk_trained")
    net = trained_pnlk(golden).to(dev)
    res, calls = fused(net, lambda: net(T(z["template"]).to(dev), T(z["source"]).to(dev), maxiter=10))
    assert calls.count("l3d_reg_iclk_step") == 10 and calls.count("l3d_reg_jac_pinv") == 1
    assert res['est_T_series'].is_cuda and isinstance(res['itr'], int)
    for k in ("est_T", "est_R", "est_t", "transformed_source"):
        close(res[k].cpu(), z["f64." + k], 1e-5, what="fused " + k)
    close(res['r'].cpu(), z["f64.r"], 1e-5, rtol=1e-4, what="fused r")
    ours = res['est_T_series'].cpu().numpy().astype(np.float64)
    worst = 0.0
    for i in range(11):
        gap = np.abs(z["f32.est_T_series"][i].astype(np.float64) - z["f64.est_T_series"][i]).max()
        err = np.abs(ours[i] - z["f64.est_T_series"][i]).max()
        ratio = err / gap if gap > 0 else (0.0 if err == 0 else np.inf)
        print(f"est_T_series[{i}]: ours vs fp64 {err:.3e}, reference fp32 vs fp64 {gap:.3e}, ratio {ratio:.2f}")
        worst = max(worst, ratio)
    print(f"largest series-error ratio {worst:.2f} (bar {SERIES_GAP_FACTOR})")
    assert worst <= SERIES_GAP_FACTOR


def test_pointnetlk_itr_and_frozen_state(golden, dev):
    z = golden("pnlk_trained")
    want_itr = int(z["f64.xtol3.itr"])
    net = trained_pnlk(golden, xtol=1e-3).to(dev)
    tpl, src = T(z["template"]).to(dev), T(z["source"]).to(dev)
    res, _ = fused(net, lambda: net(tpl, src, maxiter=10))
    assert res['itr'] == want_itr and net.last_err is None
    close(res['est_T'].cpu(), z["f64.xtol3.est_T"], 1e-5, what="xtol 1e-3 est_T")
    short, _ = fused(net, lambda: net(tpl, src, maxiter=want_itr))
    assert short['itr'] == want_itr
    assert torch.equal(short['est_T'], res['est_T']), "launches after the stop changed est_T"
    tail = res['est_T_series'][want_itr:]
    assert torch.equal(tail, res['est_T'].unsqueeze(0).expand_as(tail))


def test_pointnetlk_identical_and_singular(golden, dev):
    z = golden("pnlk_cases")
    net = trained_pnlk(golden).to(dev)
    res, _ = fused(net, lambda: net(T(z["same.template"]).to(dev), T(z["same.source"]).to(dev)))
    assert res['itr'] == 1 and net.last_err == 0 and float(res['r'].abs().max()) == 0.0
    close(res['est_T'].cpu(), z["same.f64.est_T"], 1e-6, what="identical clouds est_T")
    close(res['est_T_series'].cpu(), z["same.f64.est_T_series"], 1e-6, what="identical clouds series")
    res, calls = fused(net, lambda: net(T(z["point.template"]).to(dev), T(z["point.source"]).to(dev)))
    assert "l3d_reg_jac_pinv" in calls
    assert res['r'] is None and res['itr'] == 1 and isinstance(net.last_err, RuntimeError)
    for k in ("est_T", "est_R", "est_t", "est_T_series", "transformed_source"):
        close(res[k].cpu(), z["point.f64." + k], 1e-6, what="singular " + k)


def test_pointnetlk_small_and_uncentred(golden, dev):
    z = golden("pnlk_cases")
    net = trained_pnlk(golden).to(dev)
    res, calls = fused(net, lambda: net(T(z["ragged.template"]).to(dev), T(z["ragged.source"]).to(dev)))
    assert "l3d_pointwise_conv[maxpool]" not in calls and "l3d_reg_iclk_step" in calls          # N = 96: the un-pooled conv5 route
    for k in ("est_T", "transformed_source"):
        close(res[k].cpu(), z["ragged.f64." + k], 1e-5, what="ragged " + k)
    net = trained_pnlk(golden, p0_zero_mean=False, p1_zero_mean=False).to(dev)
    res, _ = fused(net, lambda: net(T(z["nomean.template"]).to(dev), T(z["nomean.source"]).to(dev)))
    for k in ("est_T", "transformed_source"):
        close(res[k].cpu(), z["nomean.f64." + k], 1e-5, what="uncentred " + k)


def test_pointnetlk_loop_in_one_graph(golden, dev):
    from learning3d_amd.ops import data_utils
    z = golden("pnlk_trained")
    net = trained_pnlk(golden).to(dev)
    tpl, src = T(z["template"]).to(dev), T(z["source"]).to(dev)
    eager, _ = fused(net, lambda: net(tpl, src, maxiter=10))
    with torch.no_grad():
        t, s, _, _ = data_utils.mean_shift(tpl, src, True, True)
        ctx = net.fused_setup(t, s, 10)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            net.fused_loop(ctx)                                  # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            net.fused_loop(ctx)
        for _ in range(2):
            ctx["est_T"].fill_(7.0)                              # stale state must not leak into a replay
            ctx["r"].fill_(7.0)
            graph.replay()
            torch.cuda.synchronize()
            got = net.fused_result(ctx)
            assert got['itr'] == eager['itr']
            assert torch.equal(got['est_T'][:, :3, :3], eager['est_R']) and torch.equal(got['est_T'][:, :3, 3], eager['est_t'])
            assert torch.equal(got['r'], eager['r']) and torch.equal(got['transformed_source'], eager['transformed_source'])


def test_pointnetlk_routes_agree_and_train_mode(golden, dev):
    from learning3d_amd.models import pointnetlk
    z = golden("pnlk_trained")
    net = trained_pnlk(golden).to(dev)
    tpl, src = T(z["template"]).to(dev), T(z["source"]).to(dev)
    a, calls = fused(net, lambda: net(tpl, src, maxiter=10))
    assert "l3d_reg_iclk_step" in calls
    pointnetlk.FUSED_LOOP = False
    try:
        b, calls = fused(net, lambda: net(tpl, src, maxiter=10))
    finally:
        pointnetlk.FUSED_LOOP = True
    assert "l3d_reg_iclk_step" not in calls
    for k in ("est_T", "est_T_series", "transformed_source"):
        close(a[k].cpu(), b[k].cpu(), 1e-5, what="fused vs op-sequence " + k)
    net.feature_model.train()
    before = int(net.feature_model.bn1.num_batches_tracked)
    c, calls = fused(net, lambda: net(tpl, src, maxiter=2))
    assert "l3d_reg_iclk_step" not in calls, "train-mode BatchNorm must take the op-sequence route"
    assert net.feature_model.training and int(net.feature_model.bn1.num_batches_tracked) == before + 2   # template and source, once each


@pytest.mark.parametrize("iters", [8, 1])
def test_ipcrnet_against_fp64(golden, dev, iters):
    z8 = golden("ipcrnet_seeded")
    z = z8 if iters == 8 else golden("ipcrnet_seeded_it1")
    net = seeded_ipcrnet(golden).to(dev)
    res, calls = fused(net, lambda: net(T(z8["template"]).to(dev), T(z8["source"]).to(dev), max_iteration=iters))
    assert calls.count("l3d_reg_quat_update") == iters and calls.count("l3d_linear_rows") == 6 * iters
    assert res['est_t'].shape == (8, 1, 3)
    for k in ("est_T", "est_R", "est_t", "transformed_source"):
        close(res[k].cpu(), z["f64." + k], 1e-5, what=f"iPCRNet[{iters}] {k}")
    close(res['r'].cpu(), z["f64.r"], 1e-5, rtol=1e-4, what=f"iPCRNet[{iters}] r")


def test_pinv_kernel_against_numpy(golden, dev):
    from learning3d_amd.models import _registration as reg
    z = golden("pnlk_pinv")
    f0, f, dt = z["f0"].astype(np.float64), z["f"].astype(np.float64), z["dt"].astype(np.float64)
    J = (f0[:, None, :] - f) / dt[None, :, None]                               # [B,6,K]
    want = np.linalg.inv(J @ J.transpose(0, 2, 1)) @ J
    sing = torch.zeros(1 + f0.shape[0], dtype=torch.int32, device=dev)
    got = reg.jac_pinv(T(z["f0"]).to(dev), T(z["f"]).to(dev).reshape(-1, f0.shape[1]).contiguous(), T(z["dt"]).to(dev), sing)
    assert int(sing.sum()) == 0
    ours = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
    ref = np.abs(z["pinv32"] - want).max() / np.abs(want).max()
    print(f"pinv relative error: ours {ours:.3e}, the reference's fp32 pinv {ref:.3e}")
    assert ours <= ref
