"""Drop-in for learning3d/utils/pointconv_util.py on MI355X (BASELINE.json north_star names this file).

The point-set helpers call the HIP kernels: `square_distance`, `index_points`, `query_ball_point` are the same
functions as utils/model_common_utils.py's (identical bodies in the reference, pointconv_util.py:18-58, :85-105);
`farthest_point_sample` always starts at index 0 (:60-83) and `knn_point` ranks the EXPANDED distance and returns
indices only (:107-118).  The small PointConv modules around them (DensityNet, WeightNet, the two set-abstraction
layers, :205-371) keep the reference's attribute names, so checkpoints load unchanged.
`compute_density` (:194-203) is fused: no [B,N,N] tensor.

The two set-abstraction layers have two routes:
  * the op sequence: the reference's torch ops around the point-set helpers.  The public helpers above are device-only; for
    tensors they do not take (CPU, any dtype but fp32) the layers group through private torch forms of the same functions
    (`_t_*`), so the op sequence also runs on the CPU and in fp64.
  * fused (`FUSED`, the default): device fp32 tensors, eval-mode BatchNorm, nothing to differentiate, the reference's WeightNet
    (3-8-8-16) and DensityNet (1-16-8-1) widths and a last mlp width the kernel takes (a multiple of 16 up to 1024).  The grouped
    input is gathered in [B,K,S,C] order, so the mlp_convs stack runs on the pointwise-conv kernels (Conv + BatchNorm folded, ReLU)
    and leaves [B,C,K,S]; l3d_pointconv_aggregate (WeightNet, DensityNet, their product and the contraction over the neighbours in
    one launch) writes [B,16 C,S] channel-first, which `linear` + `bn_linear` + ReLU read in place as the right operand of a
    split-K l3d_bmm_f32 (`linear_bn_relu`; S = 1: the same memory as rows) -- no permute, no [B,C,K,S] product, no B S small
    matmuls, no host read.  Folded parameters are cached per parameter / running-statistic version (models/_fused.py `cached`).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from .._lib import call, f32c, require_gpu
from . import model_common_utils as _m

FUSED = True                 # False: the op sequence for every input (A/B: tools/pointconv_bench.py)

square_distance = _m.square_distance
index_points = _m.index_points
query_ball_point = _m.query_ball_point


def farthest_point_sample(xyz, npoint):
    """reference: utils/pointconv_util.py:60-83 (first centroid is index 0)."""
    return _m.farthest_point_sample(xyz, npoint, start_with_first_point=True)


def knn_point(nsample, xyz, new_xyz):
    """reference: utils/pointconv_util.py:107-118.  xyz [B,N,3] searched, new_xyz [B,S,3] queries ->
    group_idx int64 [B,S,nsample]: the nsample smallest entries of square_distance(new_xyz, xyz).  The reference's
    topk(sorted=False) leaves the order within a row unspecified; here nearest first."""
    require_gpu(xyz, new_xyz)
    B, N, Cc = xyz.shape
    S = new_xyz.shape[1]
    if Cc != 3:
        raise NotImplementedError("knn_point: C=3 only")
    if nsample > N:
        raise RuntimeError("selected index k out of range")      # what torch.topk raises
    x, q = f32c(xyz), f32c(new_xyz)
    idx = torch.empty((B, S, nsample), dtype=torch.int64, device=xyz.device)
    call("l3d_knn_point_expanded", nsample, x, q, B, N, S, idx)
    return idx


# ---------------------------------------------------------------------------------------------------------------------------
# the same helpers in torch ops, for tensors the HIP ops do not take (CPU, fp64): reference :18-118, :194-203
def _device_ops_take(*tensors):
    return all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in tensors)


def _t_square_distance(src, dst):
    dist = -2 * torch.matmul(src, dst.permute(0, 2, 1))
    dist = dist + torch.sum(src ** 2, -1)[:, :, None]
    return dist + torch.sum(dst ** 2, -1)[:, None, :]


def _t_index_points(points, idx):
    B = points.shape[0]
    batch = torch.arange(B, dtype=torch.long, device=points.device).view([B] + [1] * (idx.dim() - 1)).expand_as(idx)
    return points[batch, idx, :]


def _t_farthest_point_sample(xyz, npoint):
    B, N, _ = xyz.shape
    centroids = torch.zeros(B, npoint, dtype=torch.long, device=xyz.device)
    distance = torch.full((B, N), 1e10, dtype=xyz.dtype, device=xyz.device)
    farthest = torch.zeros(B, dtype=torch.long, device=xyz.device)
    batch = torch.arange(B, dtype=torch.long, device=xyz.device)
    for i in range(npoint):
        centroids[:, i] = farthest
        centroid = xyz[batch, farthest, :].view(B, 1, 3)
        distance = torch.minimum(distance, torch.sum((xyz - centroid) ** 2, -1))
        farthest = torch.max(distance, -1)[1]
    return centroids


def _t_compute_density(xyz, bandwidth):
    sqrdists = _t_square_distance(xyz, xyz)
    return (torch.exp(-sqrdists / (2.0 * bandwidth * bandwidth)) / (2.5 * bandwidth)).mean(dim=-1)


def _fps(xyz, npoint):
    with torch.no_grad():
        return farthest_point_sample(xyz, npoint) if _device_ops_take(xyz) else _t_farthest_point_sample(xyz, npoint)


def _knn(nsample, xyz, new_xyz):
    if _device_ops_take(xyz, new_xyz):
        return knn_point(nsample, xyz, new_xyz)
    with torch.no_grad():
        return torch.topk(_t_square_distance(new_xyz, xyz), nsample, dim=-1, largest=False, sorted=True)[1]


def _index(points, idx):
    return index_points(points, idx) if _device_ops_take(points) else _t_index_points(points, idx)


def _density(xyz, bandwidth):
    return compute_density(xyz, bandwidth) if _device_ops_take(xyz) else _t_compute_density(xyz, bandwidth)


def sample_and_group(npoint, nsample, xyz, points, density_scale=None):
    """reference: :120-149.  xyz [B,N,3], points [B,N,D] -> new_xyz [B,S,3], new_points [B,S,K,3+D],
    grouped_xyz_norm [B,S,K,3], idx [B,S,K] (+ grouped_density)."""
    B, N, C = xyz.shape
    S = npoint
    fps_idx = _fps(xyz, npoint)
    new_xyz = _index(xyz, fps_idx)
    idx = _knn(nsample, xyz, new_xyz)
    grouped_xyz_norm = _index(xyz, idx) - new_xyz.view(B, S, 1, C)
    if points is not None:
        new_points = torch.cat([grouped_xyz_norm, _index(points, idx)], dim=-1)
    else:
        new_points = grouped_xyz_norm
    if density_scale is None:
        return new_xyz, new_points, grouped_xyz_norm, idx
    return new_xyz, new_points, grouped_xyz_norm, idx, _index(density_scale, idx)


def sample_and_group_all(xyz, points, density_scale=None):
    """reference: :151-172 (one group: the whole cloud, centred on its mean)."""
    B, N, C = xyz.shape
    new_xyz = xyz.mean(dim=1, keepdim=True)
    grouped_xyz = xyz.view(B, 1, N, C) - new_xyz.view(B, 1, 1, C)
    new_points = torch.cat([grouped_xyz, points.view(B, 1, N, -1)], dim=-1) if points is not None else grouped_xyz
    if density_scale is None:
        return new_xyz, new_points, grouped_xyz
    return new_xyz, new_points, grouped_xyz, density_scale.view(B, 1, N, 1)


def group(nsample, xyz, points):
    """reference: :174-192 (every point is a centre)."""
    B, N, C = xyz.shape
    idx = _knn(nsample, xyz, xyz)
    grouped_xyz_norm = _index(xyz, idx) - xyz.view(B, N, 1, C)
    if points is not None:
        return torch.cat([grouped_xyz_norm, _index(points, idx)], dim=-1), grouped_xyz_norm
    return grouped_xyz_norm, grouped_xyz_norm


def compute_density(xyz, bandwidth):
    """reference: :194-203.  xyz [B,N,3] -> mean_j exp(-d2_ij / (2 bw^2)) / (2.5 bw), [B,N]; one fused pass
    (l3d_gaussian_density) instead of square_distance + exp + mean over a [B,N,N] tensor."""
    require_gpu(xyz)
    B, N, Cc = xyz.shape
    if Cc != 3:
        raise NotImplementedError("compute_density: C=3 only")
    x = f32c(xyz)
    out = torch.empty((B, N), dtype=torch.float32, device=xyz.device)
    call("l3d_gaussian_density", x, B, N, float(bandwidth), out)
    return out


class DensityNet(nn.Module):
    """reference: :205-229 (the sigmoid branch `i == len(...)` is unreachable there too: every layer is ReLU)."""

    def __init__(self, hidden_unit=[16, 8]):
        super(DensityNet, self).__init__()
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        chans = [1] + list(hidden_unit) + [1]
        for cin, cout in zip(chans[:-1], chans[1:]):
            self.mlp_convs.append(nn.Conv2d(cin, cout, 1))
            self.mlp_bns.append(nn.BatchNorm2d(cout))

    def forward(self, density_scale):
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            density_scale = F.relu(bn(conv(density_scale)))
        return density_scale


class WeightNet(nn.Module):
    """reference: :231-259."""

    def __init__(self, in_channel, out_channel, hidden_unit=[8, 8]):
        super(WeightNet, self).__init__()
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        chans = [in_channel] + (list(hidden_unit) if hidden_unit else []) + [out_channel]
        for cin, cout in zip(chans[:-1], chans[1:]):
            self.mlp_convs.append(nn.Conv2d(cin, cout, 1))
            self.mlp_bns.append(nn.BatchNorm2d(cout))

    def forward(self, localized_xyz):
        weights = localized_xyz
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            weights = F.relu(bn(conv(weights)))
        return weights


# ---------------------------------------------------------------------------------------------------------------------------
# the fused route's host glue
def _widths(net):
    return [(c.in_channels, c.out_channels) for c in net.mlp_convs]


def _packed_net(net):
    """WeightNet / DensityNet as the kernel's parameter block: per layer (scale w) [cout][cin] then (shift) [cout], Conv +
    eval-mode BatchNorm folded; cached on the module per parameter / running-statistic version"""
    from ..models import _fused
    sources = [t for c, b in zip(net.mlp_convs, net.mlp_bns) for t in [c.weight, c.bias] + _fused.bn_state(b)]

    def build():
        parts = []
        for conv, bn in zip(net.mlp_convs, net.mlp_bns):
            w, scale, shift = _fused.fold_conv_bn(conv, bn)
            parts += [(scale[:, None] * w).reshape(-1), shift.reshape(-1)]
        return torch.cat(parts).float().contiguous()
    return _fused.cached(net.__dict__, "_l3d_pointconv", sources, build)


def pointconv_aggregate(feat, gxyz, ginv, wn, dn):
    """l3d_pointconv_aggregate: feat [B,C,K,S], gxyz [B,S,K,3], ginv [B,S,K] or None, packed WeightNet / DensityNet blocks
    (`_packed_net`) -> [B,16 C,S], row 16 c + j = sum_k feat[c,k] DensityNet(ginv / max ginv)[k] WeightNet(gxyz)[k,j]"""
    B, Cc, K, S = feat.shape
    out = torch.empty((B, 16 * Cc, S), dtype=torch.float32, device=feat.device)
    call("l3d_pointconv_aggregate", f32c(feat), f32c(gxyz), None if ginv is None else f32c(ginv), wn, dn, B, Cc, K, S, out)
    return out


def linear_bn_relu(x, lin, bn, channel_first=False):
    """max(0, BatchNorm(lin(x))) with eval-mode statistics (bn None: lin alone, no ReLU), the product on l3d_bmm_f32 with its K range
    split into parts that are summed afterwards.  x [R,Cin] rows -> [R,Cout], or channel_first x [B,Cin,S] -> [B,Cout,S] (the
    weight is the left operand, broadcast over B: no transpose of either).
    Split, because these Linear layers are 2048 to 16384 inputs wide: one fp32 accumulation chain of that length (what the
    pointwise-conv kernel and l3d_linear_rows run) carries 2 to 4 times the error of a blocked sum, the reference's sgemm, and
    that alone took the layers' outputs past 4 x the reference's own fp32-to-fp64 gap (LABLOG R20.1)."""
    from ..models import _fused, _rows
    w, scale, shift = _fused.fold_conv_bn(lin, bn)
    Cout, Cin = w.shape
    if channel_first:
        # (the kernel's grid holds batch x parts <= 65535)
        y = _rows.bmm(w.unsqueeze(0), x, parts=max(1, min(_rows._split_parts(Cout, x.shape[2], Cin), 65535 // x.shape[0])))
        if bn is None:
            return y if shift is None else y.add_(shift[:, None])
        return y.mul_(scale[:, None]).add_(shift[:, None]).relu_()
    y = _rows.bmm(x, w.t(), parts=_rows._split_parts(x.shape[0], Cout, Cin))
    if bn is None:
        return y if shift is None else y.add_(shift)
    return y.mul_(scale).add_(shift).relu_()


class _PointConvBase(nn.Module):
    def __init__(self, npoint, nsample, in_channel, mlp, group_all):
        super().__init__()
        self.npoint = npoint
        self.nsample = nsample
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last_channel = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv2d(last_channel, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm2d(out_channel))
            last_channel = out_channel
        self.weightnet = WeightNet(3, 16)
        self.linear = nn.Linear(16 * mlp[-1], mlp[-1])
        self.bn_linear = nn.BatchNorm1d(mlp[-1])
        self.group_all = group_all

    def _tail(self, B, new_points, grouped_xyz_norm, new_xyz):
        grouped_xyz = grouped_xyz_norm.permute(0, 3, 2, 1)
        weights = self.weightnet(grouped_xyz)
        new_points = torch.matmul(input=new_points.permute(0, 3, 1, 2),
                                  other=weights.permute(0, 3, 2, 1)).view(B, self.npoint, -1)
        new_points = self.linear(new_points)
        new_points = F.relu(self.bn_linear(new_points.permute(0, 2, 1)))
        return new_xyz.permute(0, 2, 1), new_points

    def fusable(self, xyz, points):
        """the fused route's gate: FUSED, device fp32 tensors, eval-mode BatchNorm, nothing to differentiate, the reference's
        WeightNet / DensityNet widths and a channel count the kernel takes (anything else is the op sequence's)"""
        from ..models import _fused
        Cc = self.mlp_convs[-1].out_channels
        density = getattr(self, "densitynet", None)
        return (FUSED and xyz.dim() == 3 and xyz.shape[1] == 3 and xyz.shape[0] <= 65535
                and Cc % 16 == 0 and 16 <= Cc <= _lib.L3D_POINTCONV_MAX_C
                and _widths(self.weightnet) == [(3, 8), (8, 8), (8, 16)]
                and (density is None or _widths(density) == [(1, 16), (16, 8), (8, 1)])
                and _fused.fusable(self, *[t for t in (xyz, points) if t is not None]))

    def _forward_fused(self, xyz, points):
        """xyz [B,3,N], points [B,D,N] or None -> new_xyz [B,3,S], new_points [B,C',S]; device fp32, no autograd"""
        from ..models import _fused
        B, _, N = xyz.shape
        x = f32c(xyz.permute(0, 2, 1))                                             # [B,N,3]
        pts = f32c(points.permute(0, 2, 1)) if points is not None else None        # [B,N,D]
        density = getattr(self, "densitynet", None)
        inv = 1.0 / compute_density(x, self.bandwidth) if density is not None else None
        if self.group_all:
            S, K = 1, N
            new_xyz = x.mean(dim=1, keepdim=True)
            gxyz = x.view(B, 1, N, 3) - new_xyz.view(B, 1, 1, 3)                   # [B,S,K,3]; with S = 1 also [B,K,S,3]
            grouped = gxyz.view(B, N, 3) if pts is None else torch.cat([gxyz.view(B, N, 3), pts], dim=-1)
            ginv = inv
        else:
            S, K = self.npoint, self.nsample
            new_xyz = index_points(x, farthest_point_sample(x, S))
            idx = knn_point(K, x, new_xyz)                                         # [B,S,K]
            gxyz = index_points(x, idx) - new_xyz.view(B, S, 1, 3)
            # the grouped input gathered neighbour-major, [B,K,S,3+D]: the conv stack then leaves [B,C,K,S] with no permute
            idx_t = idx.transpose(1, 2).contiguous()
            grouped = index_points(x, idx_t) - new_xyz.view(B, 1, S, 3)
            if pts is not None:
                grouped = torch.cat([grouped, index_points(pts, idx_t)], dim=-1)
            grouped = grouped.view(B, K * S, -1)
            ginv = index_points(inv.view(B, N, 1), idx).view(B, S, K) if inv is not None else None
        y = grouped
        for i, (conv, bn) in enumerate(zip(self.mlp_convs, self.mlp_bns)):
            w, scale, shift = _fused.fold_conv_bn(conv, bn)
            y = _fused.pointwise_conv(y, w, scale, shift, relu=True, channel_last=(i == 0))
        Cc = y.shape[1]
        agg = pointconv_aggregate(y.view(B, Cc, K, S), gxyz, ginv, _packed_net(self.weightnet),
                                  _packed_net(density) if density is not None else None)
        z = linear_bn_relu(agg.view(B, 16 * Cc) if S == 1 else agg, self.linear, self.bn_linear, channel_first=S > 1)
        return new_xyz.permute(0, 2, 1), z.view(B, -1, S)


class PointConvSetAbstraction(_PointConvBase):
    """reference: :261-312.  xyz [B,3,N], points [B,D,N] -> new_xyz [B,3,S], new_points [B,D',S]."""

    def forward(self, xyz, points):
        if self.fusable(xyz, points):
            return self._forward_fused(xyz, points)
        B = xyz.shape[0]
        xyz = xyz.permute(0, 2, 1)
        if points is not None:
            points = points.permute(0, 2, 1)
        if self.group_all:
            new_xyz, new_points, grouped_xyz_norm = sample_and_group_all(xyz, points)
        else:
            new_xyz, new_points, grouped_xyz_norm, _ = sample_and_group(self.npoint, self.nsample, xyz, points)
        new_points = new_points.permute(0, 3, 2, 1)
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            new_points = F.relu(bn(conv(new_points)))
        return self._tail(B, new_points, grouped_xyz_norm, new_xyz)


class PointConvDensitySetAbstraction(_PointConvBase):
    """reference: :314-371 (adds the inverse-density scale through DensityNet)."""

    def __init__(self, npoint, nsample, in_channel, mlp, bandwidth, group_all):
        super().__init__(npoint, nsample, in_channel, mlp, group_all)
        self.densitynet = DensityNet()
        self.bandwidth = bandwidth

    def forward(self, xyz, points):
        if self.fusable(xyz, points):
            return self._forward_fused(xyz, points)
        B = xyz.shape[0]
        N = xyz.shape[2]
        xyz = xyz.permute(0, 2, 1)
        if points is not None:
            points = points.permute(0, 2, 1)
        xyz_density = _density(xyz, self.bandwidth)
        inverse_density = 1.0 / xyz_density
        if self.group_all:
            new_xyz, new_points, grouped_xyz_norm, grouped_density = sample_and_group_all(
                xyz, points, inverse_density.view(B, N, 1))
        else:
            new_xyz, new_points, grouped_xyz_norm, _, grouped_density = sample_and_group(
                self.npoint, self.nsample, xyz, points, inverse_density.view(B, N, 1))
        new_points = new_points.permute(0, 3, 2, 1)
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            new_points = F.relu(bn(conv(new_points)))
        inverse_max_density = grouped_density.max(dim=2, keepdim=True)[0]
        density_scale = grouped_density / inverse_max_density
        density_scale = self.densitynet(density_scale.permute(0, 3, 2, 1))
        new_points = new_points * density_scale
        return self._tail(B, new_points, grouped_xyz_norm, new_xyz)

