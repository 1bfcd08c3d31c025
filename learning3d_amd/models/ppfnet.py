"""Drop-in for learning3d/models/ppfnet.py on MI355X: PPFNet, RPMNet's feature network.  Each point's neighbours inside a ball are
described by ten numbers (the centre's xyz, the offset d, the four point-pair features), a PointNet over the neighbours
(Conv2d -> GroupNorm -> ReLU three times, maximum over the neighbours) and three Conv1d layers give one unit feature per point.
get_prepool, get_postpool and PPFNet keep the reference's names, constructor arguments and state_dict keys
(prepool.{0,1,3,4,6,7}.*, postpool.{0,1,3,4,6}.*), so its checkpoints load with strict=True.

Two routes:
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
import torch
import torch.nn as nn

from .. import _lib
from .._lib import call, f32c
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
        convs = [self.prepool[0], self.prepool[3], self.prepool[6], self.postpool[0], self.postpool[3], self.postpool[6]]
        return (self.features == ['xyz', 'dxyz', 'ppf'] and 1 <= self.n_sample <= _lib.L3D_PPF_MAX_K
                and all(_kernel_takes(c.in_channels, c.out_channels) for c in convs)
                and _fused.fusable(self, *tensors))

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

    def forward(self, xyz, normals):
        """the op sequence: xyz, normals [B,N,3] -> unit features [B,N,C]"""
        group = ppfnet_util.sample_and_group_multi if _device_ops_take(xyz, normals) else \
            (lambda _, r, k, x, n: _sample_and_group_multi(r, k, x, n))
        raw = group(-1, self.radius, self.n_sample, xyz, normals)
        raw['xyz'] = raw['xyz'][:, :, None, :].expand(-1, -1, self.n_sample, -1)  # the centre, once per neighbour slot
        x = torch.cat([raw[f] for f in self.features], dim=-1)                     # [B,N,K,raw_dim]
        x = self.prepool(x.permute(0, 3, 2, 1))                                    # [B,C,K,N]
        x = self.postpool(x.max(dim=2)[0])                                         # maximum over the neighbours: [B,C,N]
        x = x.permute(0, 2, 1)
        return x / torch.norm(x, dim=-1, keepdim=True)                             # no epsilon, as in the reference
