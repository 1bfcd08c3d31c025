"""The yardstick of ParameterPredictionNet's HIP routes, checked without a GPU (tests/golden/rpmnet_param_fixture.py):

1. the fixture's fp64 backward of a conv -> GroupNorm -> ReLU -> maximum over all positions layer equals torch.autograd in fp64
   through group_norm -> relu -> AdaptiveMaxPool1d, to 1e-12 of scale, and its channel sums S1 = g, S2 = g zhat(ext) equal the
   sums over all positions of the dense statement (rpmnet_train_fixture.gn_relu_backward64, pooled form with K = P).
2. the condition under which "the fp64 op sequence on the branches the forward took" is a fair reference: on every module case the
   forward's winner rule picks torch's own max-pool index on all but at most 1 % of the (cloud, channel) pairs that carry a gradient.
3. the fixture's mirror of the module is the module: in fp64, on its own branches, outputs and all 30 parameter gradients agree with
   the module's autograd.
4. the declarations: the header's entry points and constants are in the open table, the switch exists, and no gate opens for CPU
   tensors."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import rpmnet_param_fixture as pf       # noqa: E402
import rpmnet_train_fixture as tf       # noqa: E402


def _close(got, want, what, bar=1e-12):
    scale = float(want.abs().max()) or 1.0
    err = float((got - want).abs().max())
    assert err <= bar * scale, (what, err, scale)


@pytest.mark.parametrize("C", [16, 48])
@pytest.mark.parametrize("P", [1, 65, 150])
def test_layer_backward64_is_autograd(C, P):
    B, groups = 3, pf.groups_of(C)
    y = tf.layer_case(300 + C + P, B, C, P)[0]
    gamma, beta, du = pf.layer_case(400 + C + P, B, C)
    mean, rstd = tf.group_stats64(y, groups)
    a, s = tf.affine64(gamma, beta, mean, rstd, groups)
    ext, pw = pf.winners_of(y, a)
    dz, dgamma, dbeta, S, M = pf.gpool_backward64(du, y, ext, pw, a, s, mean, rstd, gamma, groups)
    assert bool((S[..., 0] == 0).any()) and bool((S[..., 0] != 0).any()), "channels with and without a gradient"
    # the maximum as a gather at the rule's winners: every output, the zero-weight channel's dgamma included
    want_dz, want_dg, want_db, pooled, arg = pf.gpool_autograd64(du, y, gamma, beta, groups, pw=pw)
    _close(dz, want_dz, "dz")
    _close(dgamma, want_dg, "dgamma")
    _close(dbeta, want_db, "dbeta")
    _close(torch.relu(a * ext.double() + s), pooled, "pooled")
    # torch's own pooling: it differs from the rule only where every position ties (gamma = 0), which moves that channel's dgamma alone
    want_dz, want_dg, want_db, pooled, arg = pf.gpool_autograd64(du, y, gamma, beta, groups)
    live = (gamma != 0)
    _close(dz, want_dz, "dz against AdaptiveMaxPool1d")
    _close(dbeta, want_db, "dbeta against AdaptiveMaxPool1d")
    _close(dgamma[live], want_dg[live], "dgamma against AdaptiveMaxPool1d")
    carries = (pooled > 0) & live[None]
    assert bool((arg == pw)[carries].all())
    # S1 = g, S2 = g zhat(ext) are the dense statement's sums over all positions with the gradient scattered to the winner
    d_dz, d_dg, d_db, d_S, d_M = tf.gn_relu_backward64(du[:, :, None], y, a, s, mean, rstd, gamma, groups, K=P, widx=pw[:, :, None])
    for got, want, what in ((S, d_S, "S"), (M, d_M, "M"), (dz, d_dz, "dz"), (dgamma, d_dg, "dgamma"), (dbeta, d_db, "dbeta")):
        _close(got, want, what + " against the dense statement")


@pytest.mark.parametrize("B,J,K", pf.MODULE_CASES)
def test_winner_rule_is_torchs_pooling_index(B, J, K):
    net, src, ref = pf.param_case(60 + J, B, J, K)
    beta, alpha, y5, a5, pooled, idx = pf.op_sequence_branches(net, src, ref)
    differ, counted = pf.winner_mismatches(y5, a5, pooled, idx)
    norm = net.prepool[-2]
    mean, rstd = tf.group_stats64(y5, norm.num_groups, eps=norm.eps)
    a, s = tf.affine64(norm.weight.detach(), norm.bias.detach(), mean, rstd, norm.num_groups)
    ext, _ = pf.winners_of(y5, a5)
    by_rule = torch.relu(a * ext.double() + s)
    gap = float((by_rule - pooled.double()).abs().max()) / float(pooled.abs().max())
    print(f"\n(B, J, K) = ({B}, {J}, {K}): {differ} of {counted} pairs differ; pooled values agree to {gap:.1e} of scale")
    assert counted > 500 and bool((a5 == 0).any()) and bool((a5 < 0).any())
    assert differ <= 0.01 * counted
    assert gap <= tf.TIER


def _record64(net64, src, ref):
    """the masks and winners of the fp64 module's own forward"""
    with torch.no_grad():
        h = pf.param_input(src, ref)
        pre, masks = net64.prepool, []
        for i in range(0, len(pre) - 3, 3):
            h = pre[i + 2](pre[i + 1](pre[i](h)))
            masks.append(h > 0)
        u = pre[-1](pre[-2](pre[-3](h)))
        pooled, idx = torch.nn.functional.adaptive_max_pool1d(u, 1, return_indices=True)
        h = pooled.squeeze(2)
        masks.append(h > 0)
        post = net64.postpool
        for i in (0, 3):
            h = post[i + 2](post[i + 1](post[i](h)))
            masks.append(h > 0)
    return masks, idx.squeeze(2)


def test_mirror_is_the_module_in_fp64():
    net, src, ref = pf.param_case(81, 2, 40, 27)
    net64, src, ref = net.double(), src.double(), ref.double()
    masks, pw = _record64(net64, src, ref)
    beta, alpha = net64([src, ref])
    pf.head_loss(beta, alpha).backward()
    p = {n: v.detach().clone().requires_grad_() for n, v in net64.named_parameters()}
    b2, a2 = pf.param_mirror(p, src, ref, masks, pw)
    pf.head_loss(b2, a2).backward()
    _close(b2.detach(), beta.detach(), "beta", 1e-10)
    _close(a2.detach(), alpha.detach(), "alpha", 1e-10)
    assert len(p) == 30
    for n, v in net64.named_parameters():
        _close(p[n].grad, v.grad, n, 1e-9)


def test_declarations_and_gates():
    from learning3d_amd import _lib
    from learning3d_amd.models import _fused, rpmnet
    for name in ("l3d_gn_conv_gpool", "l3d_gn_conv_gpool_workspace_bytes", "l3d_gn_gpool_backward"):
        assert name in _lib.EXT_PROTOTYPES
    assert _lib.L3D_GN_GPOOL_MAX_COUT >= 1024 and _lib.L3D_GN_GPOOL_MAX_COUT % 16 == 0
    assert rpmnet.PARAM_HIP is True and _fused.TRAIN_HIP is True
    net, src, ref = pf.param_case(5, 2, 9, 7)
    assert net._kernels_take() and len(net._parameters_in_order()) == 20
    assert not net.trains_on_hip(src, ref) and not net.fused_takes(src, ref), "CPU tensors take the op sequence"
    with torch.no_grad():
        assert not net.fused_takes(src, ref)
    beta, alpha = net([src, ref])                                      # the op sequence, under autograd
    assert beta.shape == alpha.shape == (2,) and beta.requires_grad
    wide = rpmnet.ParameterPredictionNet(weights_dim=[0])
    wide.prepool[12] = torch.nn.Conv1d(128, 1000, 1)                   # not a multiple of 16: the kernels refuse it
    wide.prepool[13] = torch.nn.GroupNorm(8, 1000)
    assert not wide._kernels_take()
