"""Drop-in for learning3d/models/rpmnet.py on MI355X: RPMNet, iterative registration by soft correspondences.  Per iteration a
small PointNet predicts the annealing parameters beta and alpha from both clouds, PPFNet gives a unit feature per point, the
feature distances become a [B,J,K] affinity -beta (dist - alpha), a Sinkhorn normalisation with a slack row and column turns it
into a soft permutation, and a weighted Kabsch step gives the transform (reference: models/rpmnet.py; examples/test_rpmnet.py).
ParameterPredictionNet, to_numpy, se3_transform, match_features, sinkhorn, compute_rigid_transform and RPMNet keep the
reference's names, arguments, attributes (add_slack, num_sk_iter; after a forward beta, alpha, feat_source, feat_template,
affinity, perm_matrix), result keys and state_dict keys (weights_net.*, feat_extractor.*), so its checkpoints load with strict=True.

Deliberate differences:
  * RPMNet(feature_model=None) builds its own PPFNet.  The reference's default argument is ONE PPFNet instance made at import and
    shared by every default-constructed RPMNet; here two models never share weights by accident (as MaskNet's default does).
  * On the fused route the assertion on det(R) > 0 is dropped: it is a host read in the middle of the loop, and the kernel picks
    the rotation by the determinant's sign itself.
  * beta and alpha of every iteration are gathered on the device and become numpy once, after the last launch; the reference
    copies them to the host inside every iteration.
  * split_normals builds the zero normals of a [B,N,3] cloud in the cloud's own dtype (zeros_like): fp64 clouds without normals
    work; the reference builds fp32 zeros and fails there.

Two routes:
  * the op sequence: the reference's torch ops; CPU tensors, fp64 (`net.double()`) and autograd work.  It also serves
    add_slack=False, a Sinkhorn eps > 0, metric='angle', and any feature network without a `fused_features` the kernels take.
  * fused (FUSED, device fp32, nothing to differentiate, add_slack, a fusable PPFNet): RPMNet._forward_fused.  The template's
    features are computed once and reused by the later iterations (GroupNorm has no running state: the same bits); per iteration
    the parameter network (ParameterPredictionNet.fused_forward where its gate holds: the pre-pool stack on l3d_gn_conv and
    l3d_gn_conv_gpool, the head in torch; switch PARAM_HIP), PPFNet.fused_features of the moved source, the affinity from utils.square_distance,
    l3d_sinkhorn_slack (potentials only, the padded matrix is never written; it also gives the row sums and the weighted template
    points) and l3d_rigid_transform_weighted (3x3 SVD on the device).  No host read inside the loop.
Training (a parameter requires a gradient, neither cloud does): the op-sequence loop, whose feature network then takes its
differentiable HIP route (PPFNet.train_features); the template's features are computed once per forward and the tensor is reused
by the later iterations, autograd adding the gradients of its uses.  The matching stage -- affinity, Sinkhorn, exp, row sums and
weighted template -- is one differentiable unit on HIP (RPMNet._Match, gate RPMNet.matches_on_hip, A/B switch MATCH_HIP):
l3d_sinkhorn_slack_keep keeps the fp64 potentials of every iteration and l3d_sinkhorn_slack_backward runs the reverse sweep from
them, so no padded [B,J+1,K+1] tensor exists and the Kabsch weights are the unit's own row sums.  The feature distance, the
weighted Kabsch step (torch.svd) and the parameter network's post-pool head stay torch autograd.  ParameterPredictionNet's
pre-pool stack is differentiable on HIP too (ParameterPredictionNet._Train, gate trains_on_hip, A/B switch PARAM_HIP): its last
layer, 128 -> 1024 channels over all J + K positions into a maximum, never writes its [B,1024,J+K] output, forward
(l3d_gn_conv_gpool) or backward (l3d_gn_gpool_backward forms it again).  _fused.TRAIN_HIP = False, or a cloud that requires a
gradient, gives the plain op sequence for both clouds, for the matching and for the parameter network.
_lib.LAUNCH_LOG shows the route: l3d_ppf_group and l3d_gn_conv appear on the fused and the training route only (the public
sinkhorn takes l3d_sinkhorn_slack on device fp32 tensors without autograd on either route, unless FUSED is off)."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from .._lib import call, f32c, on_device_of
from ..utils import angle_difference, square_distance as _device_square_distance
from .ppfnet import PPFNet, _device_ops_take, _kernel_takes, _square_distance, backward_descent, gn_affine, gn_conv, gn_mean_rstd, gn_relu
from .ppfnet import op_sequence_only
from .ppfnet import _TLS as _ppfnet_tls
from . import _fused

_EPS = 1e-5  # To prevent division by zero
FUSED = True                 # False: the op sequence for every input (A/B: tools/rpmnet_bench.py)
MATCH_HIP = True             # False: the matching stage of a training step on torch autograd (A/B: tools/rpmnet_train_bench.py)
PARAM_HIP = True             # False: ParameterPredictionNet's pre-pool stack in torch on every route (A/B: both tools above)


def _block(layer, groups, width):
    return [layer, nn.GroupNorm(groups, width), nn.ReLU()]


def gn_conv_gpool(x, in_a, in_s, weight, bias):
    """l3d_gn_conv_gpool: x [B,Cin,P], in_a / in_s [B,Cin] or None, weight [Cout,Cin(,1)], bias [Cout] or None -> (ymax, ymin [B,Cout],
    pmax, pmin int32 [B,Cout], moments fp64 [B,Cout,2]) of the convolution output over all P positions; the output is never stored"""
    x = f32c(x)
    B, Cin, P = x.shape
    Cout = weight.shape[0]
    w = f32c(weight.detach()).view(Cout, Cin)
    dev = x.device
    ymax = torch.empty((B, Cout), dtype=torch.float32, device=dev)
    ymin = torch.empty_like(ymax)
    pmax = torch.empty((B, Cout), dtype=torch.int32, device=dev)
    pmin = torch.empty_like(pmax)
    moments = torch.empty((B, Cout, 2), dtype=torch.float64, device=dev)
    ws = torch.empty(_lib.lib().l3d_gn_conv_gpool_workspace_bytes(B, Cout, P) // 8, dtype=torch.float64, device=dev)
    call("l3d_gn_conv_gpool", x, in_a, in_s, w, None if bias is None else f32c(bias.detach()), B, Cin, Cout, P, ymax, ymin, pmax, pmin,
         moments, ws)
    return ymax, ymin, pmax, pmin, moments


def gn_gpool_backward(x, in_a, in_s, weight, bias, g, ext, pw, stat, gamma, groups, want_dz=True, want_gamma=True, want_beta=True):
    """The backward of a conv -> GroupNorm -> ReLU -> maximum over all positions layer at the convolution output, which is formed
    again from the forward's operands (x, in_a, in_s, weight, bias as gn_conv_gpool took them).  g [B,C] the gradient at the pooled
    value times [pooled > 0]; ext, pw [B,C] the winning extreme and its position; stat from gn_mean_rstd; gamma [C].  The channel sums
    S1 = g, S2 = g zhat(ext) in torch (fp64, [B,C]), l3d_gn_backward_reduce with count = P, l3d_gn_gpool_backward
    -> (dz [B,C,P] or None, dgamma [C] or None, dbeta [C] or None)"""
    x = f32c(x)
    B, Cin, P = x.shape
    Cc = weight.shape[0]
    dev = x.device
    gamma, g = f32c(gamma.detach()), f32c(g)
    cpg = Cc // groups
    s1 = g.double()
    zhat = (ext.double() - stat[:, :, 0].repeat_interleave(cpg, 1)) * stat[:, :, 1].repeat_interleave(cpg, 1)
    part = torch.stack([s1, s1 * zhat], -1).contiguous()
    m = torch.empty((B, groups, 2), dtype=torch.float64, device=dev)
    dgamma = torch.empty(Cc, dtype=torch.float32, device=dev) if want_gamma else None
    dbeta = torch.empty(Cc, dtype=torch.float32, device=dev) if want_beta else None
    call("l3d_gn_backward_reduce", part, gamma, B, Cc, int(groups), P, m, dgamma, dbeta)
    dz = None
    if want_dz:
        dz = torch.empty((B, Cc, P), dtype=torch.float32, device=dev)
        call("l3d_gn_gpool_backward", x, in_a, in_s, f32c(weight.detach()).view(Cc, Cin), None if bias is None else f32c(bias.detach()),
             g, pw, stat, gamma, m, B, Cin, Cc, int(groups), P, dz)
    return dz, dgamma, dbeta


class ParameterPredictionNet(nn.Module):
    """PointNet over both clouds (a fourth coordinate tells them apart) -> beta, alpha > 0 per pair.
    The pre-pool stack (five conv -> GroupNorm -> ReLU layers and the maximum over all J + K positions) has two HIP routes beside
    the op sequence, both behind PARAM_HIP; the post-pool head (three Linear layers over B rows) is torch on every route.
      * `fused_forward` (gate `fused_takes`; RPMNet._forward_fused calls it, `forward` never takes it on its own): layers 1-4 by
        l3d_gn_conv + l3d_gn_affine, layer 5 by l3d_gn_conv_gpool, whose [B,1024,J+K] output is never written.
      * `_Train` (gate `trains_on_hip`; `forward` dispatches to it): the same launch list under autograd, differentiable with respect
        to the 20 pre-pool parameter tensors; the backward forms layer 5's output again (l3d_gn_gpool_backward)."""

    def __init__(self, weights_dim):
        super().__init__()
        self.weights_dim = weights_dim
        pre, cin = [], 4
        for cout, groups in ((64, 8), (64, 8), (64, 8), (128, 8), (1024, 16)):
            pre += _block(nn.Conv1d(cin, cout, 1), groups, cout)
            cin = cout
        self.prepool = nn.Sequential(*pre)
        self.pooling = nn.AdaptiveMaxPool1d(1)
        self.postpool = nn.Sequential(*_block(nn.Linear(1024, 512), 16, 512), *_block(nn.Linear(512, 256), 16, 256),
                                      nn.Linear(256, 2 + int(np.prod(weights_dim))))

    def _layers(self):
        """the five pre-pool convolutions in order, each with the GroupNorm behind it"""
        pre = self.prepool
        return [(pre[i], pre[i + 1]) for i in range(0, len(pre), 3)]

    def _parameters_in_order(self):
        """the pre-pool parameter tensors layer by layer: weight, bias of the convolution, weight, bias of the GroupNorm"""
        return [p for pair in self._layers() for m in pair for p in (m.weight, m.bias) if p is not None]

    def _kernels_take(self):
        """layers of Conv1d(k = 1) -> affine GroupNorm -> ReLU with widths the kernels take, forward and as dgrad"""
        layers = self._layers()
        if not all(isinstance(c, nn.Conv1d) and c.kernel_size == (1,) and c.bias is not None and isinstance(n, nn.GroupNorm)
                   and n.affine for c, n in layers):
            return False
        last = layers[-1][0]
        # forward: l3d_gn_conv, the last layer l3d_gn_conv_gpool; dgrad of every layer but the first: l3d_gn_conv on the transpose
        return (all(_kernel_takes(c.in_channels, c.out_channels) for c, _ in layers[:-1])
                and all(_kernel_takes(c.out_channels, c.in_channels) for c, _ in layers[1:])
                and last.out_channels % 16 == 0 and 16 <= last.out_channels <= _lib.L3D_GN_GPOOL_MAX_COUT
                and 1 <= last.in_channels <= _lib.L3D_GN_CONV_MAX_CIN)

    @staticmethod
    def _clouds_fit(src, ref):
        return (all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.shape[2] == 3
                    for t in (src, ref)) and src.shape[0] == ref.shape[0] <= 65535)

    def fused_takes(self, src, ref):
        """the eval route's gate: PARAM_HIP, device fp32 clouds [B,J,3], [B,K,3], nothing to differentiate, widths the kernels take"""
        return PARAM_HIP and self._clouds_fit(src, ref) and self._kernels_take() and _fused.fusable(self, src, ref)

    def trains_on_hip(self, src, ref):
        """the differentiable HIP route's gate: PARAM_HIP and _fused.TRAIN_HIP, grad mode on and not inside op_sequence_only, device
        fp32 clouds that require no gradient themselves, affine GroupNorms and widths the kernels take, and a pre-pool parameter that
        requires a gradient"""
        return (PARAM_HIP and _fused.TRAIN_HIP and torch.is_grad_enabled() and not getattr(_ppfnet_tls, "op_sequence", False)
                and self._clouds_fit(src, ref) and not src.requires_grad and not ref.requires_grad and self._kernels_take()
                and any(p.requires_grad for p in self._parameters_in_order()))

    @staticmethod
    def _input(src, ref):
        """[B,J,3], [B,K,3] -> [B,4,J+K] contiguous, the fourth channel 0 on the source and 1 on the reference"""
        src = F.pad(src, (0, 1), mode='constant', value=0)
        ref = F.pad(ref, (0, 1), mode='constant', value=1)
        return torch.cat([src, ref], dim=1).permute(0, 2, 1).contiguous()

    def _prepool_hip(self, x, keep=False):
        """x [B,4,P] -> the pooled activation [B,C]; keep: also (ys, affs, stats, ext, pw) for the backward: the convolution outputs of
        layers 1-4, every layer's a, s [B,C] and (mean, rstd), the winning extreme of layer 5 and its position [B,C]"""
        P = x.shape[2]
        layers = self._layers()
        a = s = None
        ys, affs, stats = [], [], []
        for i, (conv, norm) in enumerate(layers):
            if i < len(layers) - 1:
                y, _, _, mom = gn_conv(x, a, s, conv.weight, conv.bias)
            else:
                ymax, ymin, pmax, pmin, mom = gn_conv_gpool(x, a, s, conv.weight, conv.bias)
            if keep:
                stats.append(gn_mean_rstd(mom, norm.num_groups, P, norm.eps))
            a, s = gn_affine(mom, norm, P)
            affs += [a, s]
            if i < len(layers) - 1:
                ys.append(y)
                x = y
        up = a >= 0
        ext = torch.where(up, ymax, ymin)                  # the extreme the GroupNorm's sign turns into the maximum
        pooled = self._pooled(a, s, ext)
        return (pooled, (ys, affs, stats, ext, torch.where(up, pmax, pmin))) if keep else pooled

    @staticmethod
    def _pooled(a, s, ext):
        return torch.relu(a * ext + s)

    def _head(self, pooled):
        raw = self.postpool(pooled)
        return F.softplus(raw[:, 0]), F.softplus(raw[:, 1])

    def fused_prepool(self, x):
        """x = [src [B,J,3], ref [B,K,3]] -> the pooled pre-pool activation [B,1024]; device fp32, no autograd, no host read"""
        with on_device_of(x[0]):
            return self._prepool_hip(self._input(f32c(x[0]), f32c(x[1])))

    def fused_forward(self, x):
        """forward on the eval HIP route (the caller has asked fused_takes)"""
        return self._head(self.fused_prepool(x))

    # A class of the model, as PPFNet._Train and RPMNet._Match are: tests/test_gpu_views_backward.py pins the set of module-level
    # autograd.Functions.  Its checks (view inputs, gradients that arrive as views) are held by tests/test_gpu_rpmnet_param.py.
    class _Train(torch.autograd.Function):
        """src [B,J,3], ref [B,K,3] -> the pooled activation [B,1024], differentiable with respect to the 20 pre-pool parameter
        tensors.  forward: fused_prepool's launch list plus an l3d_gn_mean_rstd per layer.  Kept for the backward: the input [B,4,P],
        the convolution outputs y1..y4, per layer a, s [B,C] and (mean, rstd), layer 5's winning extreme and its position [B,1024],
        the parameters -- no [B,1024,P] tensor.  backward: layer 5's GroupNorm by gn_gpool_backward (its output formed again), then
        ppfnet.backward_descent from layer 5's convolution, every layer dense; it stops at the lowest layer that learns."""

        @staticmethod
        def forward(ctx, net, src, ref, *params):
            x = net._input(f32c(src.detach()), f32c(ref.detach()))
            pooled, (ys, affs, stats, ext, pw) = net._prepool_hip(x, keep=True)
            ctx.net = net
            ctx.save_for_backward(x, ext, pw, *ys, *affs, *stats, *params)
            return pooled

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, dpooled):
            net = ctx.net
            layers = net._layers()
            L = len(layers)
            saved = list(ctx.saved_tensors)
            x, ext, pw = saved[:3]
            ys, affs, stats, params = saved[3:L + 2], saved[L + 2:3 * L + 2], saved[3 * L + 2:4 * L + 2], saved[4 * L + 2:]
            needs = ctx.needs_input_grad[3:]
            grads = [None] * len(params)
            slot = {id(p): j for j, p in enumerate(net._parameters_in_order())}
            conv, norm = layers[-1]
            jw, jb, jg, jt = (slot[id(p)] for p in (conv.weight, conv.bias, norm.weight, norm.bias))
            # layer 5's dz is wanted where its convolution, or anything underneath, learns
            upto = [p for pair in layers[:-1] for m in pair for p in (m.weight, m.bias)] + [conv.weight, conv.bias]
            with on_device_of(x):
                g = f32c(dpooled) * (net._pooled(affs[-2], affs[-1], ext) > 0)
                dz = [None]                                # layer 5's is the one [B,1024,P] tensor: no second reference to it
                dz[0], grads[jg], grads[jt] = gn_gpool_backward(
                    ys[-1] if L > 1 else x, affs[-4] if L > 1 else None, affs[-3] if L > 1 else None, params[jw], params[jb], g, ext, pw,
                    stats[-1], params[jg], norm.num_groups, want_dz=any(needs[slot[id(p)]] for p in upto),
                    want_gamma=needs[jg], want_beta=needs[jt])
                if dz[0] is not None:
                    backward_descent(layers, ys, affs, stats, params, needs, slot, grads, dz, L - 1,
                                     lambda i: x if i == 0 else gn_relu(ys[i - 1], affs[2 * i - 2], affs[2 * i - 1]))
            return (None, None, None, *grads)

    def forward(self, x):
        """x = [src [B,J,3], ref [B,K,3]] -> beta [B], alpha [B]: the pre-pool stack on _Train where trains_on_hip holds, the op
        sequence else (the eval HIP route is fused_forward, the caller's choice)"""
        if self.trains_on_hip(x[0], x[1]):
            with on_device_of(x[0]):
                return self._head(self._Train.apply(self, x[0], x[1], *self._parameters_in_order()))
        src = F.pad(x[0], (0, 1), mode='constant', value=0)
        ref = F.pad(x[1], (0, 1), mode='constant', value=1)
        feat = self.prepool(torch.cat([src, ref], dim=1).permute(0, 2, 1))
        raw = self.postpool(torch.flatten(self.pooling(feat), start_dim=-2))
        return F.softplus(raw[:, 0]), F.softplus(raw[:, 1])


def to_numpy(tensor):
    """a tensor's values as a numpy array (an array passes through)"""
    if isinstance(tensor, torch.Tensor):
        return tensor.detach().cpu().numpy()
    if isinstance(tensor, np.ndarray):
        return tensor
    raise NotImplementedError


def se3_transform(g, a, normals=None):
    """g [B,3|4,4], a [B,N,3] -> R a + t; with normals [B,N,3] also the rotated normals"""
    R, p = g[..., :3, :3], g[..., :3, 3]
    if g.dim() != a.dim():
        raise NotImplementedError
    b = torch.matmul(a, R.transpose(-1, -2)) + p[..., None, :]
    if normals is None:
        return b
    return b, normals @ R.transpose(-1, -2)


def _pairwise_sq(src, dst):
    if _device_ops_take(src, dst):
        return _device_square_distance(src, dst)
    return _square_distance(src, dst)


def match_features(feat_src, feat_ref, metric='l2'):
    """feat_src [B,J,C], feat_ref [B,K,C] -> [B,J,K]: squared distances ('l2') or angles ('angle')"""
    assert feat_src.shape[-1] == feat_ref.shape[-1]
    if metric == 'l2':
        return _pairwise_sq(feat_src, feat_ref)
    if metric == 'angle':
        s = feat_src / (torch.norm(feat_src, dim=-1, keepdim=True) + _EPS)
        r = feat_ref / (torch.norm(feat_ref, dim=-1, keepdim=True) + _EPS)
        return angle_difference(s, r)
    raise NotImplementedError


def sinkhorn_slack(log_alpha, n_iters, xyz_ref=None, eps=_EPS, want_log=True, want_perm=False):
    """l3d_sinkhorn_slack on device fp32 log_alpha [B,J,K] -> (log_perm, perm, rowsum [B,J], weighted [B,J,3]); the outputs that
    were not asked for are None (rowsum and weighted come with xyz_ref [B,K,3])"""
    A = f32c(log_alpha)
    B, J, K = A.shape
    dev = A.device
    log_perm = torch.empty_like(A) if want_log else None
    perm = torch.empty_like(A) if want_perm else None
    rowsum = weighted = None
    if xyz_ref is not None:
        xyz_ref = f32c(xyz_ref)
        rowsum = torch.empty((B, J), dtype=torch.float32, device=dev)
        weighted = torch.empty((B, J, 3), dtype=torch.float32, device=dev)
    ws = torch.empty(_lib.lib().l3d_sinkhorn_workspace_bytes(B, J, K) // 8, dtype=torch.float64, device=dev)
    call("l3d_sinkhorn_slack", A, B, J, K, int(n_iters), xyz_ref, float(eps), log_perm, perm, rowsum, weighted, ws)
    return log_perm, perm, rowsum, weighted


def sinkhorn_slack_keep(log_alpha, n_iters, xyz_ref, eps=_EPS):
    """l3d_sinkhorn_slack_keep on contiguous device fp32 log_alpha [B,J,K], xyz_ref [B,K,3] -> (perm, rowsum [B,J], weighted [B,J,3],
    potentials fp64 [n_iters,B,J+K]); the first three are l3d_sinkhorn_slack's bits"""
    B, J, K = log_alpha.shape
    dev = log_alpha.device
    perm = torch.empty_like(log_alpha)
    rowsum = torch.empty((B, J), dtype=torch.float32, device=dev)
    weighted = torch.empty((B, J, 3), dtype=torch.float32, device=dev)
    potentials = torch.empty((int(n_iters), B, J + K), dtype=torch.float64, device=dev)
    call("l3d_sinkhorn_slack_keep", log_alpha, B, J, K, int(n_iters), xyz_ref, float(eps), None, perm, rowsum, weighted,
         potentials if n_iters else None)
    return perm, rowsum, weighted, potentials


def sinkhorn_slack_backward(log_alpha, potentials, xyz_ref=None, eps=_EPS, d_perm=None, d_rowsum=None, d_weighted=None, d_affinity=None,
                            dist=None, beta=None, alpha=None, want_beta=False, want_alpha=False):
    """l3d_sinkhorn_slack_backward: contiguous device fp32 tensors, potentials from sinkhorn_slack_keep, whichever cotangents arrived
    -> (d_out [B,J,K], d_beta [B] or None, d_alpha [B] or None).  With dist, beta, alpha d_out is the gradient at dist, else at
    log_alpha"""
    B, J, K = log_alpha.shape
    n = potentials.shape[0]
    dev = log_alpha.device
    d_out = torch.empty_like(log_alpha)
    d_beta = torch.empty(B, dtype=torch.float32, device=dev) if want_beta else None
    d_alpha = torch.empty(B, dtype=torch.float32, device=dev) if want_alpha else None
    ws = torch.empty(_lib.lib().l3d_sinkhorn_backward_workspace_bytes(B, J, K, n) // 8, dtype=torch.float64, device=dev)
    call("l3d_sinkhorn_slack_backward", log_alpha, potentials if n else None, B, J, K, n, xyz_ref, float(eps), d_perm, d_rowsum,
         d_weighted, d_affinity, dist, beta, alpha, d_out, d_beta, d_alpha, ws)
    return d_out, d_beta, d_alpha


def sinkhorn(log_alpha, n_iters: int = 5, slack: bool = True, eps: float = -1) -> torch.Tensor:
    """n_iters rounds of row then column normalisation of exp(log_alpha) [B,J,K] in the log domain -> log of the result.  slack:
    an extra row and column of zeros take part and are never normalised themselves, so rows and columns sum to <= 1.  eps > 0:
    stop once the matrix moves by less than eps (summed absolute change, the largest over the batch).
    Device fp32 without autograd, slack and eps <= 0: l3d_sinkhorn_slack.  Anything else: torch."""
    if slack and eps <= 0 and _device_ops_take(log_alpha) and FUSED:
        with on_device_of(log_alpha):
            return sinkhorn_slack(log_alpha, n_iters)[0]
    prev = None
    if slack:
        padded = F.pad(log_alpha, (0, 1, 0, 1))
        for _ in range(n_iters):
            padded = torch.cat((padded[:, :-1, :] - torch.logsumexp(padded[:, :-1, :], dim=2, keepdim=True),
                                padded[:, -1:, :]), dim=1)                       # every row but the slack row
            padded = torch.cat((padded[:, :, :-1] - torch.logsumexp(padded[:, :, :-1], dim=1, keepdim=True),
                                padded[:, :, -1:]), dim=2)                       # every column but the slack column
            if eps > 0:
                now = torch.exp(padded[:, :-1, :-1])
                if prev is not None and torch.max(torch.sum(torch.abs(now - prev), dim=[1, 2])) < eps:
                    break
                prev = now.clone()
        return padded[:, :-1, :-1]
    for _ in range(n_iters):
        log_alpha = log_alpha - torch.logsumexp(log_alpha, dim=2, keepdim=True)
        log_alpha = log_alpha - torch.logsumexp(log_alpha, dim=1, keepdim=True)
        if eps > 0:
            now = torch.exp(log_alpha)
            if prev is not None and torch.max(torch.sum(torch.abs(now - prev), dim=[1, 2])) < eps:
                break
            prev = now.clone()
    return log_alpha


def rigid_transform_weighted(a, b, weights):
    """l3d_rigid_transform_weighted: a, b [B,M,3], weights [B,M] (device fp32) -> T [B,3,4]"""
    a, b, weights = f32c(a), f32c(b), f32c(weights)
    B, M, _ = a.shape
    T = torch.empty((B, 3, 4), dtype=torch.float32, device=a.device)
    call("l3d_rigid_transform_weighted", a, b, weights, B, M, _EPS, T)
    return T


def compute_rigid_transform(a: torch.Tensor, b: torch.Tensor, weights: torch.Tensor):
    """the op-sequence weighted Kabsch: a, b [B,M,3], weights [B,M] -> T [B,3,4] with T a = b.  Differentiable through torch.svd."""
    wn = weights[..., None] / (torch.sum(weights[..., None], dim=1, keepdim=True) + _EPS)
    ca = torch.sum(a * wn, dim=1)
    cb = torch.sum(b * wn, dim=1)
    cov = (a - ca[:, None, :]).transpose(-2, -1) @ ((b - cb[:, None, :]) * wn)
    u, _, v = torch.svd(cov, some=False, compute_uv=True)
    rot_pos = v @ u.transpose(-1, -2)
    v_neg = v.clone()
    v_neg[:, :, 2] *= -1                                                        # the smallest singular direction flipped
    rot_neg = v_neg @ u.transpose(-1, -2)
    rot = torch.where(torch.det(rot_pos)[:, None, None] > 0, rot_pos, rot_neg)
    assert torch.all(torch.det(rot) > 0)
    t = cb[:, :, None] - rot @ ca[:, :, None]
    return torch.cat((rot, t), dim=2)


class RPMNet(nn.Module):
    def __init__(self, feature_model=None):
        super().__init__()
        self.add_slack = True
        self.num_sk_iter = 5
        self.weights_net = ParameterPredictionNet(weights_dim=[0])
        self.feat_extractor = feature_model if feature_model is not None else PPFNet()

    def compute_affinity(self, beta, feat_distance, alpha=0.5):
        """log of the initial match matrix: -beta (distance - alpha); alpha a float or [B]"""
        if not isinstance(alpha, float):
            alpha = alpha[:, None, None]
        return -beta[:, None, None] * (feat_distance - alpha)

    @staticmethod
    def split_normals(data):
        """[B,N,6] -> xyz, normals; [B,N,3] -> xyz and zero normals"""
        if data.shape[2] == 6:
            return data[:, :, :3], data[:, :, 3:6]
        if data.shape[2] == 3:
            return data, torch.zeros_like(data)
        raise ValueError(f"RPMNet takes clouds [B,N,3] or [B,N,6], got {tuple(data.shape)}")

    def spam(self, xyz_template, norm_template, xyz_source, norm_source, feat_template=None):
        """one round of the op sequence: parameters, features of both clouds, affinity, Sinkhorn -> weighted template [B,J,3].
        feat_template: the template's features from an earlier round, used instead of computing them again"""
        self.beta, self.alpha = self.weights_net([xyz_source, xyz_template])
        self.feat_source = self.feat_extractor(xyz_source, norm_source)
        self.feat_template = self.feat_extractor(xyz_template, norm_template) if feat_template is None else feat_template
        dist = match_features(self.feat_source, self.feat_template)
        self.affinity, self.perm_matrix, self._match_rowsum, weighted = self.match_stage(dist, self.beta, self.alpha, xyz_template)
        return weighted

    def match_stage(self, dist, beta, alpha, xyz_ref):
        """feature distances [B,J,K], beta, alpha, xyz_ref [B,K,3] -> (affinity, perm, rowsum, weighted [B,J,3]): RPMNet._Match where
        matches_on_hip holds (rowsum [B,J] is then the unit's own output), else the op sequence (rowsum None: the caller sums perm)"""
        if self.matches_on_hip(dist, beta, alpha, xyz_ref):
            with on_device_of(dist):
                return self._Match.apply(dist, beta, alpha, xyz_ref, self.num_sk_iter)
        affinity = self.compute_affinity(beta, dist, alpha=alpha)
        perm = torch.exp(sinkhorn(affinity, n_iters=self.num_sk_iter, slack=self.add_slack))
        return affinity, perm, None, perm @ xyz_ref / (torch.sum(perm, dim=2, keepdim=True) + _EPS)

    def matches_on_hip(self, dist, beta, alpha, xyz_ref):
        """the gate of the matching stage's differentiable HIP route: MATCH_HIP and _fused.TRAIN_HIP, grad mode on and not inside
        op_sequence_only, the slack Sinkhorn, device fp32 tensors with beta and alpha [B], a template that requires no gradient and
        at least one of dist, beta, alpha that does"""
        tensors = (dist, beta, alpha, xyz_ref)
        return (MATCH_HIP and _fused.TRAIN_HIP and torch.is_grad_enabled() and not getattr(_ppfnet_tls, "op_sequence", False)
                and self.add_slack and all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in tensors)
                and dist.dim() == 3 and beta.shape == alpha.shape == dist.shape[:1] and not xyz_ref.requires_grad
                and (dist.requires_grad or beta.requires_grad or alpha.requires_grad))

    # A class of the model, as PPFNet._Train is: tests/test_gpu_views_backward.py pins the set of module-level autograd.Functions.
    class _Match(torch.autograd.Function):
        """dist [B,J,K], beta [B], alpha [B], xyz_ref [B,K,3], n_iters -> affinity, perm, rowsum [B,J], weighted [B,J,3]: the chain
        compute_affinity -> sinkhorn -> exp -> row sums -> weighted template as one unit, differentiable with respect to dist, beta
        and alpha.  forward: the affinity by compute_affinity's own torch expression (the op sequence's bits), then
        l3d_sinkhorn_slack_keep.  Kept for the backward: the inputs, the affinity and the fp64 potentials [n,B,J+K]; perm is not,
        the backward forms P again in fp64.  backward: one l3d_sinkhorn_slack_backward call on whichever cotangents arrived, with
        the fold's d_beta / d_alpha only where beta / alpha needs a gradient; None for xyz_ref."""

        @staticmethod
        def forward(ctx, dist, beta, alpha, xyz_ref, n_iters):
            dist, beta, alpha, xyz_ref = f32c(dist.detach()), f32c(beta.detach()), f32c(alpha.detach()), f32c(xyz_ref.detach())
            affinity = -beta[:, None, None] * (dist - alpha[:, None, None])      # compute_affinity's expression
            perm, rowsum, weighted, potentials = sinkhorn_slack_keep(affinity, n_iters, xyz_ref)
            ctx.save_for_backward(dist, beta, alpha, xyz_ref, affinity, potentials)
            ctx.set_materialize_grads(False)
            return affinity, perm, rowsum, weighted

        @staticmethod
        def backward(ctx, d_affinity, d_perm, d_rowsum, d_weighted):
            dist, beta, alpha, xyz_ref, affinity, potentials = ctx.saved_tensors
            given = [None if g is None else f32c(g) for g in (d_perm, d_rowsum, d_weighted, d_affinity)]
            need_dist, need_beta, need_alpha = ctx.needs_input_grad[:3]
            if all(g is None for g in given) or not (need_dist or need_beta or need_alpha):
                return None, None, None, None, None
            with on_device_of(affinity):
                d_dist, d_beta, d_alpha = sinkhorn_slack_backward(affinity, potentials, xyz_ref, _EPS, *given, dist=dist, beta=beta,
                                                                  alpha=alpha, want_beta=need_beta, want_alpha=need_alpha)
            return d_dist if need_dist else None, d_beta, d_alpha, None, None

    def fusable(self, template, source):
        """the fused route's gate: FUSED, the slack Sinkhorn, device fp32 clouds, nothing to differentiate in either network,
        and a feature network whose own gate agrees"""
        fx = self.feat_extractor
        return (FUSED and self.add_slack and hasattr(fx, "fused_features") and _fused.fusable(self, template, source)
                and fx.fusable(template, source))

    def _result(self, source, transforms, gammas, perms, weighted, beta, alpha):
        last = transforms[-1]
        # [R t; 0 0 0 1] built on the tensor's own device: convert2transformation makes its bottom row on the host and copies it
        # over, which a stream capture refuses
        est_T = torch.zeros((last.shape[0], 4, 4), dtype=last.dtype, device=last.device)
        est_T[:, :3, :] = last[:, :3, :]
        est_T[:, 3, 3] = 1
        moved = torch.bmm(est_T[:, :3, :3], source[:, :, :3].permute(0, 2, 1)).permute(0, 2, 1) + est_T[:, :3, 3].unsqueeze(1)
        return {'est_R': est_T[:, :3, :3], 'est_t': est_T[:, :3, 3], 'est_T': est_T, 'transformed_source': moved,
                'perm_matrices_init': gammas, 'perm_matrices': perms, 'weighted_template': weighted, 'beta': beta,
                'alpha': alpha, 'transforms': transforms}

    def _forward_fused(self, template, source, max_iterations):
        """the fused route: the result dict with 'beta' and 'alpha' as device tensors [iterations,B]; nothing is read back"""
        fx = self.feat_extractor
        xyz_t, xyz_s = f32c(template[:, :, :3]), f32c(source[:, :, :3])
        norm_t = f32c(template[:, :, 3:6]) if template.shape[2] == 6 else None
        norm_s = f32c(source[:, :, 3:6]) if source.shape[2] == 6 else None
        if template.shape[2] not in (3, 6) or source.shape[2] not in (3, 6):
            raise ValueError(f"RPMNet takes clouds [B,N,3] or [B,N,6], got {tuple(template.shape)} and {tuple(source.shape)}")
        self.feat_template = fx.fused_features(xyz_t, norm_t)                    # once: later iterations reuse it
        cur, cur_n = xyz_s, norm_s
        transforms, gammas, perms, weighted, betas, alphas = [], [], [], [], [], []
        for _ in range(max_iterations):
            wn = self.weights_net
            hip_params = hasattr(wn, "fused_takes") and wn.fused_takes(cur, xyz_t)
            self.beta, self.alpha = wn.fused_forward([cur, xyz_t]) if hip_params else wn([cur, xyz_t])
            self.feat_source = fx.fused_features(cur, cur_n)
            dist = _device_square_distance(self.feat_source, self.feat_template)
            self.affinity = self.compute_affinity(self.beta, dist, alpha=self.alpha)
            _, self.perm_matrix, rowsum, wt = sinkhorn_slack(self.affinity, self.num_sk_iter, xyz_ref=xyz_t, want_log=False,
                                                             want_perm=True)
            T = rigid_transform_weighted(xyz_s, wt, rowsum)
            if norm_s is None:
                cur = se3_transform(T, xyz_s)
            else:
                cur, cur_n = se3_transform(T, xyz_s, norm_s)
            transforms.append(T)
            gammas.append(torch.exp(self.affinity))
            perms.append(self.perm_matrix)
            weighted.append(wt)
            betas.append(self.beta)
            alphas.append(self.alpha)
        return self._result(source, transforms, gammas, perms, weighted, torch.stack(betas), torch.stack(alphas))

    def forward(self, template, source, max_iterations: int = 1):
        """template [B,K,3|6], source [B,J,3|6] (xyz, or xyz and normals) -> the reference's dict: est_R, est_t, est_T (source ->
        template), transformed_source, and per iteration perm_matrices_init, perm_matrices, weighted_template, transforms, with
        beta and alpha as numpy [iterations,B]"""
        if self.fusable(template, source):
            with on_device_of(template, source):
                result = self._forward_fused(template, source, max_iterations)
            result['beta'], result['alpha'] = to_numpy(result['beta']), to_numpy(result['alpha'])
            return result

        # the feature network's differentiable HIP route (PPFNet.train_features) serves a pair only as a whole: with one cloud that
        # requires a gradient both take the op sequence.  On that route the template's features are computed once and the tensor is
        # reused by the later iterations (GroupNorm has no running state: the same values; autograd adds the gradients of its uses)
        fx = self.feat_extractor
        hip_train = hasattr(fx, "trains_on_hip") and fx.trains_on_hip(template, source)
        if hip_train:
            return self._forward_op_sequence(template, source, max_iterations, True)
        with op_sequence_only():
            return self._forward_op_sequence(template, source, max_iterations, False)

    def _forward_op_sequence(self, template, source, max_iterations, reuse_template):
        xyz_t, norm_t = self.split_normals(template)
        xyz_s, norm_s = self.split_normals(source)
        cur, cur_n = xyz_s, norm_s
        transforms, gammas, perms, weighted, betas, alphas = [], [], [], [], [], []
        for it in range(max_iterations):
            wt = self.spam(xyz_t, norm_t, cur, cur_n, feat_template=self.feat_template if reuse_template and it else None)
            # the matching unit's own row sums where it ran: a torch.sum of its perm would send a dense d_perm back to it
            rowsum = getattr(self, "_match_rowsum", None)
            T = compute_rigid_transform(xyz_s, wt, weights=torch.sum(self.perm_matrix, dim=2) if rowsum is None else rowsum)
            cur, cur_n = se3_transform(T.detach(), xyz_s, norm_s)                # always the ORIGINAL source, moved
            transforms.append(T)
            gammas.append(torch.exp(self.affinity))
            perms.append(self.perm_matrix)
            weighted.append(wt)
            betas.append(self.beta.detach())
            alphas.append(self.alpha.detach())
        self._match_rowsum = None
        return self._result(source, transforms, gammas, perms, weighted, to_numpy(torch.stack(betas)), to_numpy(torch.stack(alphas)))
