"""What the tests of ParameterPredictionNet's HIP routes share (tests/test_rpmnet_param_cpu.py, tests/test_gpu_rpmnet_param.py):

  * conv_case: the operands of one conv (-> GroupNorm -> ReLU -> maximum over all positions) layer built so that a leaked padding
    column would be an extreme and each extreme is attained twice; layer_case: the layer's GroupNorm (gamma with zeros and
    negatives) and the gradient du [B,C] at the pooled value.
  * gpool_backward64: the layer's backward at the convolution output y as include/ext/l3d_rpmnet_param.h states it, in plain torch
    and fp64 from a given y.  The CPU test holds it to torch.autograd through GroupNorm -> ReLU -> AdaptiveMaxPool1d; the GPU test
    holds the kernel to it.  gpool_autograd64 is that autograd statement.
  * param_case / param_mirror: a seeded ParameterPredictionNet with perturbed GroupNorm weights (some zero, some negative), a pair
    of clouds, and the reference's op sequence (models/rpmnet.py:28-75 of the reference: pad, cat, Conv1d / GroupNorm / ReLU five
    times, the maximum over all positions, Linear / GroupNorm / ReLU twice, Linear, softplus) in any dtype on recorded branches --
    each layer's ReLU mask and the pooling winners -- by the method of tests/test_gpu_grad_modules.py.
  * winners_of / winner_mismatches: the forward's winner rule and the count of (cloud, channel) pairs on which it differs from
    torch's own max-pool index: the condition that keeps "on the branches the forward took" from hiding a wrong winner."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from seeded import seeded_params                                   # noqa: E402
from rpmnet_train_fixture import EPS, GAP_FACTOR, TIER, group_stats64, affine64      # noqa: E402,F401

MODULE_CASES = [(4, 717, 1024), (3, 40, 27), (2, 1, 1)]            # (B, J, K) of the winner condition
HEAD_WEIGHTS = (0.7, -1.3)                                         # the fixed weights of (sum beta, sum alpha) in the module loss


def groups_of(C):
    """the layer cases' group count: 8 as the stack's narrow layers where it divides C into more than one channel, else 4"""
    return 8 if C % 8 == 0 and C > 8 else 4


# ------------------------------------------------------------------------------------------------------------------------------
def conv_case(seed, B, Cin, Cout, P, affine, dev="cpu"):
    """-> x [B,Cin,P], in_a, in_s [B,Cin] (None without `affine`), w [Cout,Cin], bias [Cout].
    x > 0 and every weight of a channel has the channel's sign, so y - bias has one sign per channel over all real positions and a
    padding column that leaked (as the bare bias, or as zero against biases of +-50) would be an extreme.  Columns 1 and P - 2 hold
    the same large input and columns P // 2 and P - 1 the same small one (P >= 6): extremes attained twice, in different tiles
    once P > 64.  in_a has a zero (channel 0) and negatives."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, Cin, P), generator=g) + 0.25
    if P >= 6:
        x[:, :, 1] = x[:, :, 1] * 3.0
        x[:, :, P - 2] = x[:, :, 1]
        x[:, :, P // 2] = x[:, :, P // 2] * 0.01
        x[:, :, P - 1] = x[:, :, P // 2]
    sign = torch.where(torch.rand((Cout, 1), generator=g) < 0.5, -1.0, 1.0)
    w = (torch.rand((Cout, Cin), generator=g) + 0.1) * 0.05 * sign
    bias = torch.where(torch.arange(Cout) % 2 == 0, 50.0, -50.0)
    in_a = in_s = None
    if affine:
        in_a = torch.rand((B, Cin), generator=g) * 2 - 0.6
        in_a[:, 0] = 0.0
        in_a[:, 1] = -0.5
        in_s = torch.rand((B, Cin), generator=g) - 0.3
    return tuple(None if t is None else t.to(dev).contiguous() for t in (x, in_a, in_s, w, bias))


def layer_case(seed, B, C, dev="cpu"):
    """-> gamma [C] with a zero (channel 1) and negatives (channel 2 and at random), beta [C] (large enough that the pooled value of a
    good share of the channels is positive), du [B,C] the gradient at the pooled value"""
    g = torch.Generator().manual_seed(seed)
    gamma = torch.rand((C,), generator=g) * 2 - 0.7
    gamma[1], gamma[2] = 0.0, -0.8
    beta = torch.rand((C,), generator=g) - 0.3
    beta[1] = 0.2                                                   # the zero-weight channel is constant and positive
    beta[4], beta[5] = -40.0, -40.0                                 # below any a y: the ReLU closes these channels, g = 0
    du = torch.randn((B, C), generator=g)
    return tuple(t.to(dev) for t in (gamma, beta, du))


def extremes_of(y):
    """y [B,C,P] -> ymax, ymin [B,C] and the lowest position attaining each (torch.max / torch.min do not promise the first index on
    ties on every device: the first p equal to the extreme does)"""
    P = y.shape[2]
    p = torch.arange(P, device=y.device).view(1, 1, P)
    ymax, ymin = y.amax(2), y.amin(2)
    pmax = torch.where(y == ymax[:, :, None], p, P).amin(2)
    pmin = torch.where(y == ymin[:, :, None], p, P).amin(2)
    return ymax, ymin, pmax, pmin


def winners_of(y, a):
    """the forward's rule: the winning extreme of y [B,C,P] and its position, the maximum where a [B,C] >= 0, the minimum else"""
    ymax, ymin, pmax, pmin = extremes_of(y)
    up = a >= 0
    return torch.where(up, ymax, ymin), torch.where(up, pmax, pmin)


def gpool_backward64(du, y, ext, pw, a, s, mean, rstd, gamma, groups, mask=None):
    """The header's statement from a given y [B,C,P]: du [B,C] the gradient at the pooled value, ext / pw [B,C] the winning extreme
    and its position, a, s [B,C] the layer's GroupNorm as a scale and shift, mean, rstd [B,groups], gamma [C]; mask [B,C]: pooled > 0
    (None: from a ext + s in fp64).  Everything is taken to fp64.
    -> dz [B,C,P], dgamma [C], dbeta [C], S [B,C,2], M [B,groups,2]"""
    B, C, P = y.shape
    y, du, ext, gamma = y.double(), du.double(), ext.double(), gamma.double()
    cpg = C // groups
    mean_c, rstd_c = mean.double().repeat_interleave(cpg, 1), rstd.double().repeat_interleave(cpg, 1)
    if mask is None:
        mask = a.double() * ext + s.double() > 0
    g = du * mask
    S1, S2 = g, g * ((ext - mean_c) * rstd_c)                      # no pass over y: g lives at one position per (cloud, channel)
    n = cpg * P
    M1 = (gamma[None] * S1).view(B, groups, cpg).sum(2) / n
    M2 = (gamma[None] * S2).view(B, groups, cpg).sum(2) / n
    zhat = (y - mean_c[:, :, None]) * rstd_c[:, :, None]
    top = torch.zeros_like(y)
    inside = (pw >= 0) & (pw < P)
    top.scatter_(2, pw.long().clamp(0, P - 1)[:, :, None], (gamma[None] * g * inside)[:, :, None])
    dz = rstd_c[:, :, None] * (top - M1.repeat_interleave(cpg, 1)[:, :, None] - zhat * M2.repeat_interleave(cpg, 1)[:, :, None])
    return dz, S2.sum(0), S1.sum(0), torch.stack([S1, S2], -1), torch.stack([M1, M2], -1)


def gpool_autograd64(du, y, gamma, beta, groups, pw=None):
    """the same gradients from torch.autograd in fp64 through group_norm -> relu -> AdaptiveMaxPool1d(1); pw: the maximum as a gather
    at these positions instead (a channel with gamma = 0 is constant over p: every position ties, and the forward's rule picks the
    winner there, not torch's pooling).  -> dz, dgamma, dbeta, the pooled value, the positions torch's pooling chose"""
    y = y.double().clone().requires_grad_()
    gamma, beta = gamma.double().clone().requires_grad_(), beta.double().clone().requires_grad_()
    u = torch.relu(torch.nn.functional.group_norm(y, groups, gamma, beta, EPS))
    pooled, arg = torch.nn.functional.adaptive_max_pool1d(u, 1, return_indices=True)
    if pw is not None:
        pooled = torch.gather(u, 2, pw.long()[:, :, None])
    pooled = pooled.squeeze(2)
    (pooled * du.double()).sum().backward()
    return y.grad, gamma.grad, beta.grad, pooled.detach(), arg.squeeze(2)


# ------------------------------------------------------------------------------------------------------------------------------
def param_case(seed, B, J, K):
    """-> (ParameterPredictionNet fp32 on the CPU with seeded weights, every GroupNorm weight of order one with both signs and two
    zeros; src [B,J,3]; ref [B,K,3])"""
    from learning3d_amd.models.rpmnet import ParameterPredictionNet
    net = seeded_params(ParameterPredictionNet(weights_dim=[0]), seed)
    g = torch.Generator().manual_seed(seed + 500)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.GroupNorm):
                C = m.weight.shape[0]
                wt = torch.rand((C,), generator=g) * 2 - 0.5          # a quarter negative
                wt[3], wt[C // 2] = 0.0, 0.0
                m.weight.copy_(wt)
                m.bias.copy_(torch.rand((C,), generator=g) * 0.6 - 0.2)
    src = torch.rand((B, J, 3), generator=g) * 2 - 1
    ref = torch.rand((B, K, 3), generator=g) * 2 - 1
    return net, src.contiguous(), ref.contiguous()


def group_norm(z, groups, gamma, beta):
    """nn.GroupNorm(groups, C) by its definition on z [B,C,...]"""
    B, C = z.shape[:2]
    v = z.reshape(B, groups, -1)
    mean = v.mean(2, keepdim=True)
    var = ((v - mean) ** 2).mean(2, keepdim=True)
    zn = ((v - mean) / torch.sqrt(var + EPS)).reshape(z.shape)
    shape = (1, C) + (1,) * (z.dim() - 2)
    return zn * gamma.view(shape) + beta.view(shape)


PRE = ((0, 1, 8), (3, 4, 8), (6, 7, 8), (9, 10, 8), (12, 13, 16))    # (conv, norm, groups) of prepool
POST = ((0, 1, 16), (3, 4, 16))                                      # (linear, norm, groups) of postpool; postpool.6 is bare


def param_input(src, ref):
    """[B,J,3], [B,K,3] -> [B,4,J+K], the fourth channel 0 on the source and 1 on the reference"""
    src = torch.nn.functional.pad(src, (0, 1), mode='constant', value=0)
    ref = torch.nn.functional.pad(ref, (0, 1), mode='constant', value=1)
    return torch.cat([src, ref], dim=1).permute(0, 2, 1)


def param_mirror(p, src, ref, masks, pw):
    """The reference's ParameterPredictionNet.forward in the dtype of `p` (name -> parameter, the module's state_dict keys) on
    recorded branches: masks[0..3] the ReLU masks [B,C,P] of the first four layers, masks[4] [B,1024] that of the pooled value,
    masks[5], masks[6] [B,C] those of the head; pw int64 [B,1024] the pooling winners.  The ReLU is a product with the mask, the
    maximum a gather at the winner.  -> beta [B], alpha [B]"""
    dt = p["prepool.0.weight"].dtype
    h = param_input(src.to(dt), ref.to(dt))
    for i, (c, n, groups) in enumerate(PRE):
        w = p[f"prepool.{c}.weight"]
        z = torch.matmul(w.reshape(w.shape[0], -1), h) + p[f"prepool.{c}.bias"].view(1, -1, 1)
        z = group_norm(z, groups, p[f"prepool.{n}.weight"], p[f"prepool.{n}.bias"])
        if i < len(PRE) - 1:
            h = z * masks[i].to(dt)
        else:
            h = torch.gather(z, 2, pw[:, :, None]).squeeze(2) * masks[i].to(dt)
    for i, (c, n, groups) in enumerate(POST):
        z = h @ p[f"postpool.{c}.weight"].t() + p[f"postpool.{c}.bias"]
        h = group_norm(z, groups, p[f"postpool.{n}.weight"], p[f"postpool.{n}.bias"]) * masks[len(PRE) + i].to(dt)
    raw = h @ p["postpool.6.weight"].t() + p["postpool.6.bias"]
    return torch.nn.functional.softplus(raw[:, 0]), torch.nn.functional.softplus(raw[:, 1])


def head_loss(beta, alpha):
    """the softplus outputs summed with fixed weights"""
    return HEAD_WEIGHTS[0] * beta.sum() + HEAD_WEIGHTS[1] * alpha.sum()


def op_sequence_branches(net, src, ref):
    """the module's own torch op sequence under no_grad, layer by layer -> (beta, alpha, y5 [B,1024,P] the last convolution's output,
    a5 [B,1024] the last GroupNorm's scale per (cloud, channel), pooled [B,1024], idx [B,1024] torch's own max-pool index)"""
    with torch.no_grad():
        h = param_input(src, ref)
        pre = net.prepool
        for i in range(0, len(pre) - 3, 3):
            h = pre[i + 2](pre[i + 1](pre[i](h)))
        y5 = pre[-3](h)
        norm = pre[-2]
        B, C, P = y5.shape
        _, rstd = group_stats64(y5, norm.num_groups, eps=norm.eps)
        a5 = norm.weight.double()[None] * rstd.repeat_interleave(C // norm.num_groups, 1)
        u = pre[-1](norm(y5))
        pooled, idx = torch.nn.functional.adaptive_max_pool1d(u, 1, return_indices=True)
        raw = net.postpool(pooled.squeeze(2))
        sp = torch.nn.functional.softplus
        return sp(raw[:, 0]), sp(raw[:, 1]), y5, a5, pooled.squeeze(2), idx.squeeze(2)


def winner_mismatches(y5, a5, pooled, idx):
    """-> (pairs that differ, pairs counted): over the (cloud, channel) pairs with pooled > 0 and a != 0, those where the position the
    sign of a selects from argmax / argmin of the fp32 convolution output is not torch's own max-pool index.  Channels with a = 0 are
    left out: there every position ties and torch takes p = 0, and only dgamma of a zero-weight channel depends on the choice."""
    _, pw = winners_of(y5, a5)
    counted = (pooled > 0) & (a5 != 0)
    return int(((pw != idx) & counted).sum()), int(counted.sum())
