"""Drop-in for learning3d/models/ppfnet.py on MI355X: PPFNet, RPMNet's feature network.  Each point's neighbours inside a ball are
described by ten numbers (the centre's xyz, the offset d, the four point-pair features), a PointNet over the neighbours
(Conv2d -> GroupNorm -> ReLU three times, maximum over the neighbours) and three Conv1d layers give one unit feature per point.
get_prepool, get_postpool and PPFNet keep the reference's names, constructor arguments and state_dict keys
(prepool.{0,1,3,4,6,7}.*, postpool.{0,1,3,4,6}.*), so its checkpoints load with strict=True.

Three routes:
  * differentiable (`train_features`, gate `trains_on_hip`): device fp32 clouds that need no gradient themselves, grad mode on, a
    parameter that requires a gradient, _fused.TRAIN_HIP, the features and widths `fusable` accepts.  GroupNorm has no batch
    statistics, so the forward is the fused launch list below; what is kept is the three pre-pool convolution outputs in fp32,
    each layer's (a, s) and (mean, rstd), the ball-query idx and a one-byte pooling winner -- no ReLU output, no normalised
    value.  The backward runs on rpmnet_train.hip (include/ext/l3d_rpmnet_train.h), l3d_gn_conv as dgrad, l3d_wgrad and
    l3d_channel_stats (`PPFNet._Train`).
  * the op sequence: the reference's torch ops, on any device and dtype and under autograd.  utils.sample_and_group_multi is
    device-only, so for CPU tensors (and fp64, and inputs that need a gradient) this module carries private torch forms of the
    ball query with itself_indices, the gather and the squared distance; device fp32 tensors go through the HIP ops of utils.
  * fused (`fused_features`): device fp32, nothing to differentiate, the default three features, widths the kernel takes
    (`fusable`).  The ball query, l3d_ppf_group ([B,10,K,N] channel-first, geometry in fp64), then six l3d_gn_conv launches, an
    l3d_gn_affine behind each of the first five (the last convolution is bare): every convolution applies the previous GroupNorm + ReLU to its operand as it loads it and sums
    the next GroupNorm's moments in its epilogue, and the third one keeps only the maximum and minimum over the neighbours -- the
    [B,192,K,N] activation is never written.  The pooled activation is max(0, a (a >= 0 ? ymax : ymin) + s): both extremes,
    because a GroupNorm weight can be negative.  Weights are read from the parameters at every call; nothing is cached.
The final division by the norm has no epsilon, as in the reference."""
import threading

import torch
import torch.nn as nn

from .. import _lib
from .._lib import call, f32c, on_device_of
from ..utils import ppfnet_util
from . import _fused

_raw_features_sizes = {'xyz': 3, 'dxyz': 3, 'ppf': 4}
_raw_features_order = {'xyz': 0, 'dxyz': 1, 'ppf': 2}


def _gn_relu_stack(conv, widths, last_bare=False):
    """conv(w0 -> w1), GroupNorm(8, w1), ReLU, conv(w1 -> w2), ...; last_bare: the final convolution stands alone"""
    layers = []
    for i, (cin, cout) in enumerate(zip(widths[:-1], widths[1:])):
        layers.append(conv(cin, cout, 1))
        if not (last_bare and i == len(widths) - 2):
            layers += [nn.GroupNorm(8, cout), nn.ReLU()]
    return nn.Sequential(*layers)


def get_prepool(in_dim, out_dim):
    """the per-neighbour stack in front of the pooling: in_dim -> out_dim/2 -> out_dim/2 -> out_dim (modules 0,1,3,4,6,7 carry state)"""
    return _gn_relu_stack(nn.Conv2d, [in_dim, out_dim // 2, out_dim // 2, out_dim])


def get_postpool(in_dim, out_dim):
    """the per-point stack behind the pooling: in_dim -> in_dim -> out_dim -> out_dim, the last convolution bare (0,1,3,4,6)"""
    return _gn_relu_stack(nn.Conv1d, [in_dim, in_dim, out_dim, out_dim], last_bare=True)


# ---------------------------------------------------------------------------------------------------------------------------
# the op sequence's grouping for tensors the HIP ops do not take (CPU, fp64, autograd): utils/ppfnet_util.py:96-131, :197-244
def _square_distance(src, dst):
    dist = -2 * torch.matmul(src, dst.permute(0, 2, 1))
    dist = dist + torch.sum(src ** 2, -1)[:, :, None]
    return dist + torch.sum(dst ** 2, -1)[:, None, :]


def _index_points(points, idx):
    B = points.shape[0]
    batch = torch.arange(B, dtype=torch.long, device=points.device).view([B] + [1] * (idx.dim() - 1)).expand_as(idx)
    return points[batch, idx, :]


def _query_ball_point(radius, nsample, xyz, new_xyz, itself_indices):
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    group_idx = torch.arange(N, dtype=torch.long, device=xyz.device).view(1, 1, N).repeat([B, S, 1])
    sqrdists = _square_distance(new_xyz, xyz)
    group_idx.scatter_(2, itself_indices[:, :, None], N)               # the centre is kept out of its own neighbourhood
    group_idx[sqrdists > radius ** 2] = N
    group_idx = group_idx.sort(dim=-1)[0][:, :, :nsample]
    if group_idx.shape[2] < nsample:                                   # fewer points than slots: the reference fails here
        raise RuntimeError(f"query_ball_point: nsample {nsample} exceeds the cloud's {N} points")
    group_first = itself_indices[:, :, None].repeat([1, 1, nsample])
    mask = group_idx == N
    group_idx[mask] = group_first[mask]
    return group_idx


def _sample_and_group_multi(radius, nsample, xyz, normals):
    """sample_and_group_multi(-1, ...) in torch ops: every point is a centre"""
    B, N, C = xyz.shape
    itself = torch.arange(N, device=xyz.device)[None].repeat(B, 1)
    with torch.no_grad():
        idx = _query_ball_point(radius, nsample, xyz, xyz, itself)
    nr = normals[:, :, None, :]
    d = _index_points(xyz, idx) - xyz.view(B, N, 1, C)
    ni = _index_points(normals, idx)
    angle = ppfnet_util.angle
    ppf = torch.stack([angle(nr, d), angle(ni, d), angle(nr, ni), torch.norm(d, dim=-1)], dim=-1)
    return {'xyz': xyz, 'dxyz': d, 'ppf': ppf}


def _device_ops_take(*tensors):
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors) and not (
        torch.is_grad_enabled() and any(t.requires_grad for t in tensors))


# ---------------------------------------------------------------------------------------------------------------------------
def gn_conv(x, in_a, in_s, weight, bias, pool=0, want_y=True):
    """l3d_gn_conv: x [B,Cin,P], in_a / in_s [B,Cin] or None, weight [Cout,Cin(,1(,1))], bias [Cout] or None ->
    (y [B,Cout,P] or None, ymax, ymin [B,Cout,P/pool] or None, moments fp64 [B,Cout,2])"""
    x = f32c(x)
    B, Cin, P = x.shape
    Cout = weight.shape[0]
    w = f32c(weight.detach()).view(Cout, Cin)
    dev = x.device
    y = torch.empty((B, Cout, P), dtype=torch.float32, device=dev) if (want_y or pool == 0) else None
    ymax = torch.empty((B, Cout, P // pool), dtype=torch.float32, device=dev) if pool else None
    ymin = torch.empty_like(ymax) if pool else None
    moments = torch.empty((B, Cout, 2), dtype=torch.float64, device=dev)
    ws = torch.empty(_lib.lib().l3d_gn_conv_workspace_bytes(B, Cout, P) // 8, dtype=torch.float64, device=dev)
    call("l3d_gn_conv", x, in_a, in_s, w, None if bias is None else f32c(bias.detach()), B, Cin, Cout, P, pool, y, ymax, ymin,
         moments, ws)
    return y, ymax, ymin, moments


def gn_affine(moments, norm, count):
    """l3d_gn_affine: the GroupNorm `norm` over `count` positions per channel as a per-(cloud, channel) scale and shift [B,C]"""
    B, Cc, _ = moments.shape
    a = torch.empty((B, Cc), dtype=torch.float32, device=moments.device)
    s = torch.empty_like(a)
    call("l3d_gn_affine", moments, f32c(norm.weight.detach()), f32c(norm.bias.detach()), B, Cc, norm.num_groups, count,
         float(norm.eps), a, s)
    return a, s


def ppf_group(xyz, normals, idx):
    """l3d_ppf_group: xyz, normals [B,N,3] (normals None: zeros), idx int64 [B,N,K] -> [B,10,K,N]"""
    xyz = f32c(xyz)
    B, N, _ = xyz.shape
    K = idx.shape[2]
    feat = torch.empty((B, 10, K, N), dtype=torch.float32, device=xyz.device)
    call("l3d_ppf_group", xyz, None if normals is None else f32c(normals), idx.contiguous(), B, N, K, feat)
    return feat


def _kernel_takes(cin, cout):
    return cout % 16 == 0 and 16 <= cout <= _lib.L3D_GN_CONV_MAX_COUT and 1 <= cin <= _lib.L3D_GN_CONV_MAX_CIN


# ---------------------------------------------------------------------------------------------------------------------------
# the backward of a conv -> GroupNorm -> ReLU (-> maximum over the neighbours) layer (include/ext/l3d_rpmnet_train.h)
def gn_mean_rstd(moments, groups, count, eps):
    """l3d_gn_mean_rstd: l3d_gn_conv's moments [B,C,2] -> (mean, rstd) per (cloud, group), fp64 [B,groups,2]"""
    B, Cc, _ = moments.shape
    stat = torch.empty((B, groups, 2), dtype=torch.float64, device=moments.device)
    call("l3d_gn_mean_rstd", moments, B, Cc, int(groups), int(count), float(eps), stat)
    return stat


def gn_pool_winner(y, a, K):
    """l3d_gn_pool_winner: y [B,C,K N'] (p = k N' + n), a [B,C] -> uint8 [B,C,N']: the lowest k of the extreme a's sign selects"""
    B, Cc, P = y.shape
    widx = torch.empty((B, Cc, P // K), dtype=torch.uint8, device=y.device)
    call("l3d_gn_pool_winner", y, a, B, Cc, int(K), P // K, widx)
    return widx


def gn_relu(y, a, s):
    """l3d_gn_relu: max(0, fmaf(a, y, s)) [B,C,P], the layer's output as the forward's next convolution loaded it"""
    B, Cc, P = y.shape
    u = torch.empty((B, Cc, P), dtype=torch.float32, device=y.device)
    call("l3d_gn_relu", y, a, s, B, Cc, P, u)
    return u


def gn_backward(du, y, a, s, stat, gamma, groups, widx=None, K=0, want_gamma=True, want_beta=True):
    """The GroupNorm + ReLU backward of one layer: l3d_gn_backward_stats, _reduce, _apply.  du [B,C,P], or with widx / K the gradient
    at the pooled value [B,C,P/K]; y [B,C,P]; a, s [B,C]; stat from gn_mean_rstd; gamma [C]
    -> (dz [B,C,P], dgamma [C] or None, dbeta [C] or None)"""
    B, Cc, P = y.shape
    dev = y.device
    du, gamma = f32c(du), f32c(gamma.detach())
    K = int(K) if widx is not None else 0
    part = torch.empty((B, Cc, 2), dtype=torch.float64, device=dev)
    ws = torch.empty(_lib.lib().l3d_gn_backward_workspace_bytes(B, Cc, P) // 8, dtype=torch.float64, device=dev)
    call("l3d_gn_backward_stats", du, widx, K, y, a, s, stat, B, Cc, int(groups), P, part, ws)
    m = torch.empty((B, groups, 2), dtype=torch.float64, device=dev)
    dgamma = torch.empty(Cc, dtype=torch.float32, device=dev) if want_gamma else None
    dbeta = torch.empty(Cc, dtype=torch.float32, device=dev) if want_beta else None
    call("l3d_gn_backward_reduce", part, gamma, B, Cc, int(groups), P, m, dgamma, dbeta)
    dz = torch.empty((B, Cc, P), dtype=torch.float32, device=dev)
    call("l3d_gn_backward_apply", du, widx, K, y, a, s, stat, gamma, m, B, Cc, int(groups), P, dz)
    return dz, dgamma, dbeta


def backward_descent(layers, ys, affs, stats, params, needs, slot, grads, dz, start, operand, pooled=None):
    """The backward of a stack of conv -> GroupNorm -> ReLU layers from layer `start` down, shared by PPFNet._Train and
    ParameterPredictionNet._Train.  layers: (conv, norm) pairs; ys[i], affs[2 i], affs[2 i + 1], stats[i]: layer i's convolution
    output, a, s and (mean, rstd) as the forward kept them; params, needs, slot: the parameter tensors, which of them need a gradient,
    and id(parameter) -> its place in both; grads: filled in place.  dz: a one-element list holding the gradient at layer `start`'s
    convolution output, emptied here -- the caller keeps no other reference, so that the releases below hand the blocks back.
    operand(i): the wgrad operand of layer i, the input its convolution loaded.  pooled = (index, widx, K): that layer's output went
    through the maximum over K neighbours, widx its winner index.
    Per layer: dW by l3d_wgrad on the operand (released behind the wgrad, so that the allocator hands the block to the layer below),
    db as the first column of l3d_channel_stats summed over the clouds; it stops at the first layer, or where nothing underneath
    learns; else du = W^T dz by l3d_gn_conv on the transposed weight, then gn_backward of the layer below."""
    from ._train import channel_stats, sum_clouds, wgrad
    dz = dz.pop()
    for i in range(start, -1, -1):
        conv, _ = layers[i]
        jw, jb = slot[id(conv.weight)], slot.get(id(conv.bias))
        if needs[jw]:
            u = operand(i)
            grads[jw] = wgrad(dz, u).view_as(conv.weight)
            del u                                  # back to the allocator before du and dz of the layer below are made
        if jb is not None and needs[jb]:
            grads[jb] = sum_clouds(channel_stats(dz))[:, 0].float()
        below = [p for pair in layers[:i] for m in pair for p in (m.weight, m.bias) if p is not None]
        if not any(needs[slot[id(p)]] for p in below):
            break                                  # the first layer, or nothing underneath learns
        w = f32c(params[jw]).view(conv.out_channels, conv.in_channels)
        du = gn_conv(dz, None, None, w.t().contiguous(), None)[0]
        del dz                                     # (the widest one in either network: gone before the next is made)
        norm = layers[i - 1][1]
        jg, jt = slot[id(norm.weight)], slot[id(norm.bias)]
        widx, K = pooled[1:] if pooled is not None and pooled[0] == i - 1 else (None, 0)
        dz, grads[jg], grads[jt] = gn_backward(du, ys[i - 1], affs[2 * i - 2], affs[2 * i - 1], stats[i - 1], params[jg],
                                               norm.num_groups, widx, K, want_gamma=needs[jg], want_beta=needs[jt])
        del du


_TLS = threading.local()


class op_sequence_only:
    """`with op_sequence_only():` -- PPFNet.forward inside takes the op sequence whatever trains_on_hip says.  RPMNet enters it
    when one cloud of a pair requires a gradient: the other one's features must not change route beside it."""

    def __enter__(self):
        self.prev = getattr(_TLS, "op_sequence", False)
        _TLS.op_sequence = True

    def __exit__(self, *exc):
        _TLS.op_sequence = self.prev
        return False


_POOLED = 2          # the layer of PPFNet's six whose output goes through the maximum over the neighbours


class PPFNet(nn.Module):
    """per-point features from the ball neighbourhoods of a cloud with normals"""

    def __init__(self, features=['ppf', 'dxyz', 'xyz'], emb_dims=96, radius=0.3, num_neighbors=64):
        super().__init__()
        self.radius = radius
        self.n_sample = num_neighbors
        self.features = sorted(features, key=_raw_features_order.get)           # the order of the input channels
        raw_dim = sum(_raw_features_sizes[f] for f in self.features)
        self.prepool = get_prepool(raw_dim, emb_dims * 2)
        self.postpool = get_postpool(emb_dims * 2, emb_dims)

    def fusable(self, *tensors):
        """the fused route's gate: device fp32 tensors, nothing to differentiate, all three features, a neighbour count and layer
        widths the kernels take (anything else is the op sequence's)"""
        return self._kernels_take() and _fused.fusable(self, *tensors)

    def _layers(self):
        """the six convolutions in order, each with the GroupNorm behind it (the last one bare)"""
        pre, post = self.prepool, self.postpool
        return [(pre[0], pre[1]), (pre[3], pre[4]), (pre[6], pre[7]), (post[0], post[1]), (post[3], post[4]), (post[6], None)]

    def _parameters_in_order(self):
        """the parameter tensors of _layers, layer by layer: weight, bias of the convolution, weight, bias of the GroupNorm"""
        mods = [m for pair in self._layers() for m in pair if m is not None]
        return [p for m in mods for p in (m.weight, m.bias) if p is not None]

    def _kernels_take(self):
        """all three features, a neighbour count and layer widths the kernels take"""
        return (self.features == ['xyz', 'dxyz', 'ppf'] and 1 <= self.n_sample <= _lib.L3D_PPF_MAX_K
                and all(_kernel_takes(c.in_channels, c.out_channels) for c, _ in self._layers()))

    def trains_on_hip(self, *tensors):
        """the differentiable HIP route's gate: _fused.TRAIN_HIP, grad mode on and a parameter of the network that requires a
        gradient, device fp32 clouds that do not require one themselves, and the features and widths `fusable` accepts.  A
        GroupNorm without affine parameters takes the op sequence."""
        return (_fused.TRAIN_HIP and torch.is_grad_enabled() and not getattr(_TLS, "op_sequence", False) and self._kernels_take()
                and all(t.is_cuda and t.dtype == torch.float32 and not t.requires_grad for t in tensors)
                and all(norm is None or norm.affine for _, norm in self._layers())
                and any(p.requires_grad for p in self.parameters()))

    def train_features(self, xyz, normals):
        """fused_features under autograd: xyz, normals [B,N,3] -> unit features [B,N,C], differentiable with respect to the
        network's parameters (PPFNet._Train); the division by the norm and the permute are torch ops"""
        with on_device_of(xyz):
            y = self._Train.apply(self, xyz, normals, *self._parameters_in_order())
            cluster_feat = y.permute(0, 2, 1)
            return cluster_feat / torch.norm(cluster_feat, dim=-1, keepdim=True)

    def fused_features(self, xyz, normals):
        """xyz [B,N,3], normals [B,N,3] or None (a cloud without normals) -> [B,N,C]; device fp32, no autograd"""
        B, N, _ = xyz.shape
        K = self.n_sample
        xyz = f32c(xyz)
        itself = torch.arange(N, device=xyz.device)[None].repeat(B, 1)
        idx = ppfnet_util.query_ball_point(self.radius, K, xyz, xyz, itself_indices=itself)
        x = ppf_group(xyz, normals, idx).view(B, 10, K * N)
        pre, post = self.prepool, self.postpool
        y, _, _, mom = gn_conv(x, None, None, pre[0].weight, pre[0].bias)
        a, s = gn_affine(mom, pre[1], K * N)
        y, _, _, mom = gn_conv(y, a, s, pre[3].weight, pre[3].bias)
        a, s = gn_affine(mom, pre[4], K * N)
        _, ymax, ymin, mom = gn_conv(y, a, s, pre[6].weight, pre[6].bias, pool=K, want_y=False)
        a, s = gn_affine(mom, pre[7], K * N)
        x = torch.where((a >= 0)[:, :, None], ymax, ymin)              # the extreme the GroupNorm's sign turns into the maximum
        y, _, _, mom = gn_conv(x, a, s, post[0].weight, post[0].bias)
        a, s = gn_affine(mom, post[1], N)
        y, _, _, mom = gn_conv(y, a, s, post[3].weight, post[3].bias)
        a, s = gn_affine(mom, post[4], N)
        y, _, _, _ = gn_conv(y, a, s, post[6].weight, post[6].bias)
        cluster_feat = y.permute(0, 2, 1)
        return cluster_feat / torch.norm(cluster_feat, dim=-1, keepdim=True)

    # A class of the model, not of the module: tests/test_gpu_views_backward.py pins the set of module-level autograd.Functions and
    # a feature change may not edit it.  Its checks -- the backward on gradients that arrive as views, the forward on view inputs,
    # bit for bit against contiguous clones -- are held for this Function by tests/test_gpu_rpmnet_train.py
    # (test_train_function_on_view_gradients, test_train_function_on_view_inputs).  Once that registry may gain a name, this
    # belongs at module level with its name in it.
    class _Train(torch.autograd.Function):
        """PPFNet's feature stack [B,C,N] (in front of the division by the norm) on the HIP kernels, differentiable with respect to the
        22 parameter tensors.  forward: fused_features' launch list with want_y on the pooled layer, plus per GroupNorm layer an
        l3d_gn_mean_rstd and, behind the pooled one, an l3d_gn_pool_winner.  Kept for the backward: the clouds and the ball-query
        idx, the convolution outputs y1..y5 (the three pre-pool ones are the only [B,C,K N] tensors), the pooled extreme [B,C,N],
        per layer a, s [B,C] and (mean, rstd) fp64 [B,8,2], and the winner index, one byte per [B,C,N].  No ReLU output, no
        normalised value and no fp64 tensor of activation size: the backward recomputes them from y, a, s.
        backward: backward_descent from the last layer; a layer's wgrad operand is max(0, fmaf(a, y, s)) of the layer below written by
        l3d_gn_relu (the first layer's is l3d_ppf_group again)."""

        @staticmethod
        def forward(ctx, net, xyz, normals, *params):
            B, N, _ = xyz.shape
            K = net.n_sample
            xyz = f32c(xyz)
            normals = None if normals is None else f32c(normals)
            itself = torch.arange(N, device=xyz.device)[None].repeat(B, 1)
            idx = ppfnet_util.query_ball_point(net.radius, K, xyz, xyz, itself_indices=itself)
            layers = net._layers()
            x, a, s = ppf_group(xyz, normals, idx).view(B, 10, K * N), None, None
            ys, affs, stats, widx, xp = [], [], [], None, None
            for i, (conv, norm) in enumerate(layers):
                count = K * N if i <= _POOLED else N
                y, ymax, ymin, mom = gn_conv(x, a, s, conv.weight, conv.bias, pool=K if i == _POOLED else 0)
                if norm is None:
                    break
                a, s = gn_affine(mom, norm, count)
                ys.append(y)
                affs += [a, s]
                stats.append(gn_mean_rstd(mom, norm.num_groups, count, norm.eps))
                x = y
                if i == _POOLED:
                    widx = gn_pool_winner(y, a, K)
                    x = xp = torch.where((a >= 0)[:, :, None], ymax, ymin)
            ctx.net, ctx.has_normals = net, normals is not None
            ctx.save_for_backward(xyz, idx, widx, xp, *([normals] if normals is not None else []), *ys, *affs, *stats, *params)
            return y

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, dout):
            net = ctx.net
            saved = list(ctx.saved_tensors)
            xyz, idx, widx, xp = saved[:4]
            saved = saved[4:]
            normals = saved.pop(0) if ctx.has_normals else None
            ys, affs, stats, params = saved[:5], saved[5:15], saved[15:20], saved[20:]
            layers = net._layers()
            B, N, _ = xyz.shape
            K = net.n_sample
            grads = [None] * len(params)
            slot = {id(p): j for j, p in enumerate(net._parameters_in_order())}

            def operand(i):
                if i == 0:
                    return ppf_group(xyz, normals, idx).view(B, 10, K * N)
                return gn_relu(xp if i == _POOLED + 1 else ys[i - 1], affs[2 * i - 2], affs[2 * i - 1])

            with on_device_of(xyz):
                backward_descent(layers, ys, affs, stats, params, ctx.needs_input_grad[3:], slot, grads, [f32c(dout)],
                                 len(layers) - 1, operand, pooled=(_POOLED, widx, K))
            return (None, None, None, *grads)

    def forward(self, xyz, normals):
        """xyz, normals [B,N,3] -> unit features [B,N,C]: train_features where its gate holds, the op sequence else"""
        if self.trains_on_hip(xyz, normals):
            return self.train_features(xyz, normals)
        group = ppfnet_util.sample_and_group_multi if _device_ops_take(xyz, normals) else \
            (lambda _, r, k, x, n: _sample_and_group_multi(r, k, x, n))
        raw = group(-1, self.radius, self.n_sample, xyz, normals)
        raw['xyz'] = raw['xyz'][:, :, None, :].expand(-1, -1, self.n_sample, -1)  # the centre, once per neighbour slot
        x = torch.cat([raw[f] for f in self.features], dim=-1)                     # [B,N,K,raw_dim]
        x = self.prepool(x.permute(0, 3, 2, 1))                                    # [B,C,K,N]
        x = self.postpool(x.max(dim=2)[0])                                         # maximum over the neighbours: [B,C,N]
        x = x.permute(0, 2, 1)
        return x / torch.norm(x, dim=-1, keepdim=True)                             # no epsilon, as in the reference
