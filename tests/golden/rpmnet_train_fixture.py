"""What the tests of PPFNet's differentiable HIP route share (tests/test_rpmnet_train_cpu.py, tests/test_gpu_rpmnet_train.py):

  * gn_relu_backward64: the backward of conv output y -> GroupNorm -> ReLU (-> maximum over K) as include/ext/l3d_rpmnet_train.h
    states it, in plain torch and fp64.  The CPU test holds it to torch.autograd through nn.GroupNorm -> ReLU (-> max); the GPU test
    holds the kernels to it.
  * layer_case: one layer's inputs with a GroupNorm weight that is zero in one channel and negative in others.
  * ppfnet_case / ppfnet_mirror: a seeded PPFNet, clouds with short and full balls, and the reference's op sequence
    (models/ppfnet.py:52-92 of the reference: grouped features, Conv2d / GroupNorm / ReLU, max over the neighbours, Conv1d stack, division
    by the norm) in any dtype on recorded branches -- the ball-query idx, each layer's ReLU mask, the pooling winners.
  * plumbing_case / bench_loss: the RPMNet pair of the plumbing test and the loss of tools/rpmnet_train_bench.py.

PLUMBING_SEED was chosen on the CPU.  The condition on the inputs is that the op sequence's fp32 parameter gradients are within 1e-3
of scale of its fp64 ones on every tensor (no pooling winner or ball-query member flips between the precisions).  The fp32 op
sequence's distance from fp64 depends on its summation order, that is on the CPU's thread count: seed 0 measures 5.1e-05 with one
thread and 5.0e-04 with 4 or 16, seed 1 4.4e-05 and 1.4e-04.  Seed 2 is the first whose largest gap stays below a tenth of the
condition at 1, 4 and 16 threads (4.1e-05, 5.2e-05, 5.2e-05), so the condition holds with room on any machine
(tests/test_rpmnet_train_cpu.py asserts it where it runs).  PLUMBING_GAPS has, per tensor, the largest of the three measurements:
the parameter network's tensors between 1.8e-05 and 5.2e-05, the feature network's between 4.1e-06 and 1.4e-05.  The GPU test takes
its unit from this table, not from a run of its own: the unit must not depend on the machine the test runs on."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from seeded import seeded_params    # noqa: E402

GROUPS = 8
EPS = 1e-5
TIER = 1e-5
GAP_FACTOR = 4.0          # rpmnet_fixture.GAP_FACTOR
PLUMBING_SEED = 2
PLUMBING_CONDITION = 1e-3


# ------------------------------------------------------------------------------------------------------------------------------
def group_stats64(y, groups, eps=EPS):
    """y [B,C,P] -> (mean, rstd) fp64 [B,groups] of the GroupNorm over each group's channels and all positions"""
    B, C, P = y.shape
    v = y.double().reshape(B, groups, -1)
    mean = v.mean(2)
    var = (v * v).mean(2) - mean * mean
    return mean, 1.0 / torch.sqrt(var.clamp_min(0.0) + eps)


def gn_relu_backward64(du, y, a, s, mean, rstd, gamma, groups, K=0, widx=None):
    """du [B,C,P] (K == 0) or the gradient at the pooled value [B,C,P/K] with the winners widx [B,C,P/K] (p = k N' + n);
    y [B,C,P]; a, s [B,C] the GroupNorm as a scale and shift; mean, rstd [B,groups]; gamma [C].  Everything is taken to fp64.
    -> dz [B,C,P], dgamma [C], dbeta [C], S [B,C,2], M [B,groups,2]"""
    B, C, P = y.shape
    y, du, a, s, gamma = y.double(), du.double(), a.double(), s.double(), gamma.double()
    cpg = C // groups
    mean_c, rstd_c = mean.double().repeat_interleave(cpg, 1)[:, :, None], rstd.double().repeat_interleave(cpg, 1)[:, :, None]
    if K:
        NP = P // K
        dense = torch.zeros(B, C, K, NP, dtype=torch.float64, device=y.device)
        dense.scatter_(2, widx.long()[:, :, None, :], du[:, :, None, :])
        du = dense.view(B, C, P)
    h = a[:, :, None] * y + s[:, :, None]
    g = du * (h > 0)
    zhat = (y - mean_c) * rstd_c
    S1, S2 = g.sum(2), (g * zhat).sum(2)
    n = cpg * P
    M1 = (gamma[None] * S1).view(B, groups, cpg).sum(2) / n
    M2 = (gamma[None] * S2).view(B, groups, cpg).sum(2) / n
    dz = rstd_c * (gamma[None, :, None] * g - M1.repeat_interleave(cpg, 1)[:, :, None] - zhat * M2.repeat_interleave(cpg, 1)[:, :, None])
    return dz, S2.sum(0), S1.sum(0), torch.stack([S1, S2], -1), torch.stack([M1, M2], -1)


def gn_relu_autograd64(du, y, gamma, beta, groups, K=0, widx=None):
    """the same gradients from torch.autograd through nn.functional.group_norm -> relu (-> max over K) in fp64; pooled: du [B,C,P/K].
    widx: the max as a gather at these winners (a channel with gamma = 0 is constant over k: every k ties, and the forward's rule
    picks the winner there, not torch.max).  -> dz, dgamma, dbeta, the winners torch.max chose (or None)"""
    B, C, P = y.shape
    y = y.double().clone().requires_grad_()
    gamma, beta = gamma.double().clone().requires_grad_(), beta.double().clone().requires_grad_()
    u = torch.relu(torch.nn.functional.group_norm(y, groups, gamma, beta, EPS))
    arg = None
    if K:
        u = u.view(B, C, K, P // K)
        arg = u.max(2)[1]
        u = u.max(2)[0] if widx is None else torch.gather(u, 2, widx[:, :, None, :]).squeeze(2)
    (u * du.double()).sum().backward()
    return y.grad, gamma.grad, beta.grad, arg


def layer_case(seed, B, C, P, K=0, dev="cpu"):
    """y [B,C,P] fp32 with a mean and a spread per channel, gamma with a zero (channel 1) and negatives (channel 2 and at random),
    beta, the upstream gradient du [B,C,P] or [B,C,P/K]"""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn((B, C, P), generator=g) * (0.5 + torch.rand((1, C, 1), generator=g)) + torch.randn((1, C, 1), generator=g) * 0.3
    gamma = torch.rand((C,), generator=g) * 2 - 0.7
    gamma[1], gamma[2] = 0.0, -0.8
    beta = torch.rand((C,), generator=g) - 0.5
    du = torch.randn((B, C, P // K if K else P), generator=g)
    return tuple(t.to(dev) for t in (y, gamma, beta, du))


def affine64(gamma, beta, mean, rstd, groups):
    """l3d_gn_affine's a, s [B,C] in fp64 from (mean, rstd) [B,groups]"""
    cpg = gamma.shape[0] // groups
    a = gamma.double()[None] * rstd.repeat_interleave(cpg, 1)
    return a, beta.double()[None] - mean.repeat_interleave(cpg, 1) * a


def winners64(y, a, K):
    """the lowest k attaining the maximum of y over k where a >= 0, the minimum else: y [B,C,K N'] -> int64 [B,C,N']"""
    B, C, P = y.shape
    v = y.view(B, C, K, P // K)
    # torch.max / torch.min do not promise the first index on ties on every device: the first k equal to the extreme does
    ext = torch.where((a >= 0)[:, :, None], v.amax(2), v.amin(2))
    hit = v == ext[:, :, None, :]
    k = torch.arange(K, device=y.device).view(1, 1, K, 1).expand_as(hit)
    return torch.where(hit, k, torch.full_like(k, K)).amin(2)


# ------------------------------------------------------------------------------------------------------------------------------
def clouds(seed, B, N, dense=0.12):
    """half the points in a cube of side `dense` (their balls of radius 0.3 hold every one of them), half in [-1.5,1.5]^3 (short
    balls, many empty: padded slots, exact ties in the pool); unit normals"""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.cat([torch.rand((B, N // 2, 3), generator=g) * dense, torch.rand((B, N - N // 2, 3), generator=g) * 3 - 1.5], 1)
    xyz = xyz[:, torch.randperm(N, generator=g)]
    nrm = torch.randn((B, N, 3), generator=g)
    return xyz.contiguous(), (nrm / nrm.norm(dim=-1, keepdim=True)).contiguous()


def ppfnet_case(seed, emb_dims, K, N, B=2):
    """-> (PPFNet fp32 on the CPU with seeded weights, GroupNorm weights of both signs and order one; xyz; normals)"""
    from learning3d_amd.models import PPFNet
    net = seeded_params(PPFNet(emb_dims=emb_dims, num_neighbors=K), seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.mul_(10.0)
    xyz, nrm = clouds(seed + 1, B, N)
    return net, xyz, nrm


def _group_norm(z, gamma, beta):
    """nn.GroupNorm(8, C) by its definition on z [B,C,...]"""
    B, C = z.shape[:2]
    v = z.reshape(B, GROUPS, -1)
    mean = v.mean(2, keepdim=True)
    var = ((v - mean) ** 2).mean(2, keepdim=True)
    zn = ((v - mean) / torch.sqrt(var + EPS)).reshape(z.shape)
    shape = (1, C) + (1,) * (z.dim() - 2)
    return zn * gamma.view(shape) + beta.view(shape)


def ppfnet_mirror(p, xyz, normals, idx, masks, widx):
    """The reference's PPFNet.forward in the dtype of `p` (name -> parameter, the module's state_dict keys) on recorded branches:
    idx int64 [B,N,K] the ball query's members, masks[i] the ReLU mask of layer i (bool, [B,C,K N] for the first two, [B,C,N] behind the
    pool and after), widx int64 [B,C,N] the pooling winners.  The ReLU is a product with the mask, the max a gather at the winner."""
    from learning3d_amd.models import ppfnet
    dt = p["prepool.0.weight"].dtype
    xyz, normals = xyz.to(dt), normals.to(dt)
    B, N, K = idx.shape
    nr = normals[:, :, None, :]
    d = ppfnet._index_points(xyz, idx) - xyz.view(B, N, 1, 3)
    ni = ppfnet._index_points(normals, idx)
    angle = ppfnet.ppfnet_util.angle
    ppf = torch.stack([angle(nr, d), angle(ni, d), angle(nr, ni), torch.norm(d, dim=-1)], dim=-1)
    x = torch.cat([xyz[:, :, None, :].expand(-1, -1, K, -1), d, ppf], dim=-1).permute(0, 3, 2, 1)          # [B,10,K,N]

    def conv(h, name):
        w = p[name + ".weight"]
        z = torch.matmul(w.reshape(w.shape[0], -1), h.reshape(B, h.shape[1], -1)) + p[name + ".bias"].view(1, -1, 1)
        return z.view(B, w.shape[0], *h.shape[2:])

    h = x
    for i, (c, n) in enumerate(((0, 1), (3, 4))):
        h = _group_norm(conv(h, f"prepool.{c}"), p[f"prepool.{n}.weight"], p[f"prepool.{n}.bias"])
        h = h * masks[i].view(h.shape).to(dt)
    z = _group_norm(conv(h, "prepool.6"), p["prepool.7.weight"], p["prepool.7.bias"])                       # [B,C,K,N]
    h = torch.gather(z, 2, widx[:, :, None, :]).squeeze(2) * masks[2].to(dt)                                # [B,C,N]
    for i, (c, n) in enumerate(((0, 1), (3, 4))):
        h = _group_norm(conv(h, f"postpool.{c}"), p[f"postpool.{n}.weight"], p[f"postpool.{n}.bias"]) * masks[3 + i].to(dt)
    h = conv(h, "postpool.6").permute(0, 2, 1)
    return h / torch.norm(h, dim=-1, keepdim=True)


# ------------------------------------------------------------------------------------------------------------------------------
def plumbing_case(seed=PLUMBING_SEED, B=2, Nt=64, Ns=50, K=16):
    """-> (RPMNet fp32 on the CPU with a seeded PPFNet(num_neighbors=K), template [B,Nt,6], source [B,Ns,6], igt [B,4,4])"""
    from learning3d_amd.models import PPFNet, RPMNet
    net = seeded_params(RPMNet(feature_model=PPFNet(num_neighbors=K)), 100 + seed)
    with torch.no_grad():
        for m in net.feat_extractor.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.mul_(10.0)
    g = torch.Generator().manual_seed(1000 + seed)
    xyz = torch.rand((B, Nt, 3), generator=g) * 0.8 - 0.4
    nrm = torch.randn((B, Nt, 3), generator=g)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    c, s = 0.9553364891256060, 0.2955202066613396                                 # cos, sin of 0.3
    R = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    t = torch.tensor([0.05, -0.03, 0.04])
    src = xyz[:, :Ns] @ R.T + t
    igt = torch.eye(4).repeat(B, 1, 1)
    igt[:, :3, :3], igt[:, :3, 3] = R, t                                          # template -> source: the inverse of est_T
    return net, torch.cat([xyz, nrm], -1).contiguous(), torch.cat([src, nrm[:, :Ns] @ R.T], -1).contiguous(), igt


def bench_loss(result, igt):
    """FrobeniusNormLoss(est_T, igt) plus the mean of perm_matrices' row sums (a stand-in for an inlier term)"""
    from learning3d_amd.losses import FrobeniusNormLoss
    rows = torch.stack([pm.sum(2).mean() for pm in result["perm_matrices"]]).mean()
    return FrobeniusNormLoss()(result["est_T"], igt.to(result["est_T"].dtype)) + rows


def plumbing_gradients(net, template, source, igt, iterations=2):
    """{parameter name: gradient} of bench_loss through net(template, source, iterations) on whatever route the inputs select"""
    net.zero_grad(set_to_none=True)
    with torch.enable_grad():
        bench_loss(net(template, source, iterations), igt).backward()
    return {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}


# measured on the CPU at PLUMBING_SEED: max |fp32 op sequence - fp64 op sequence| / max |fp64| per parameter gradient
PLUMBING_GAPS = {
    "weights_net.prepool.0.weight": 3.5e-05, "weights_net.prepool.0.bias": 3.9e-05, "weights_net.prepool.1.weight": 4.3e-05,
    "weights_net.prepool.1.bias": 4.8e-05, "weights_net.prepool.3.weight": 3.8e-05, "weights_net.prepool.3.bias": 2.9e-05,
    "weights_net.prepool.4.weight": 3.6e-05, "weights_net.prepool.4.bias": 3.6e-05, "weights_net.prepool.6.weight": 1.8e-05,
    "weights_net.prepool.6.bias": 1.9e-05, "weights_net.prepool.7.weight": 3.3e-05, "weights_net.prepool.7.bias": 3.5e-05,
    "weights_net.prepool.9.weight": 4.2e-05, "weights_net.prepool.9.bias": 4.3e-05, "weights_net.prepool.10.weight": 5.2e-05,
    "weights_net.prepool.10.bias": 3.4e-05, "weights_net.prepool.12.weight": 3.8e-05, "weights_net.prepool.12.bias": 3.8e-05,
    "weights_net.prepool.13.weight": 2.7e-05, "weights_net.prepool.13.bias": 3.8e-05, "weights_net.postpool.0.weight": 3.1e-05,
    "weights_net.postpool.0.bias": 3.1e-05, "weights_net.postpool.1.weight": 4.4e-05, "weights_net.postpool.1.bias": 3.0e-05,
    "weights_net.postpool.3.weight": 3.9e-05, "weights_net.postpool.3.bias": 3.9e-05, "weights_net.postpool.4.weight": 2.8e-05,
    "weights_net.postpool.4.bias": 2.5e-05, "weights_net.postpool.6.weight": 3.0e-05, "weights_net.postpool.6.bias": 3.0e-05,
    "feat_extractor.prepool.0.weight": 8.4e-06, "feat_extractor.prepool.0.bias": 9.9e-06, "feat_extractor.prepool.1.weight":
    9.9e-06, "feat_extractor.prepool.1.bias": 9.2e-06, "feat_extractor.prepool.3.weight": 1.4e-05,
    "feat_extractor.prepool.3.bias": 1.2e-05, "feat_extractor.prepool.4.weight": 8.1e-06, "feat_extractor.prepool.4.bias":
    7.4e-06, "feat_extractor.prepool.6.weight": 8.2e-06, "feat_extractor.prepool.6.bias": 7.1e-06,
    "feat_extractor.prepool.7.weight": 6.1e-06, "feat_extractor.prepool.7.bias": 7.2e-06, "feat_extractor.postpool.0.weight":
    6.7e-06, "feat_extractor.postpool.0.bias": 4.9e-06, "feat_extractor.postpool.1.weight": 4.8e-06,
    "feat_extractor.postpool.1.bias": 4.1e-06, "feat_extractor.postpool.3.weight": 8.0e-06, "feat_extractor.postpool.3.bias":
    6.9e-06, "feat_extractor.postpool.4.weight": 8.3e-06, "feat_extractor.postpool.4.bias": 9.9e-06,
    "feat_extractor.postpool.6.weight": 7.4e-06, "feat_extractor.postpool.6.bias": 8.1e-06}
