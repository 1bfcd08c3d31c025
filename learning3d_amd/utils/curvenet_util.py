"""Drop-in for learning3d/utils/curvenet_util.py on MI355X: LPFA, the curve modules (Walk, CurveGrouping, CurveAggregation), CIC,
MaskedMaxPool and the feature-propagation layers, with the reference's constructor arguments, attribute names and state_dict keys.

Two routes compute the same forward, as in models/pointnetlk.py:
  * the FUSED route (device fp32 tensors, BatchNorm on running statistics, nothing to differentiate, a shape curvenet.hip takes):
    CurveGrouping.forward is l3d_curve_prepare (1-channel conv + sigmoid + scale + transpose), torch.topk for the start points and
    ONE l3d_curve_walk for every step of every curve; CIC's convs run on the folded 1x1-conv kernels, LPFA on l3d_lpfa_group,
    MaskedMaxPool on the HIP farthest-point sampling / ball query / index_points.  No host read anywhere: a forward can be
    captured in a graph;
  * the OP-SEQUENCE route (CPU tensors, autograd, train-mode BatchNorm, unsupported shapes): the reference's operations in torch
    (utils/curvenet_util.py:78-195 for the walk, ~30 small ops per step); LPFA's convs still reach the HIP training layers.
FUSED_WALK = False sends everything through the op-sequence route (tests compare the two).

`knn` is utils/model_common_utils.knn on the xyz coordinates with add_one_to_k (:264, :411) -- the fused HIP kNN -- and LPFA's
gathers / concatenation run as one kernel (l3d_lpfa_group).

Kept from the reference because it decides which curves are walked: the momentum softmax [bs,2,n] is viewed as [bs,1,n,2] without a
transpose (:147), so the curve at position q of the start list blends with the values at flat positions 2 q, 2 q + 1 of its cloud's
[2][n] array; the order torch.topk(sorted=False) returns the start points in is therefore an input of the walk, on both routes.

Deviations from the reference, on purpose: Walk never reads xyz (the reference's `xyz.transpose(1,2).contiguous` at :120 lacks its
call and the value is unused); index offsets are built on the input's device, not on `cuda` whenever one is available (:126,
:233); the torch.cuda.empty_cache() calls of sample_and_group (:39-45) are dropped.  Walk keeps the points it picked in
`last_path` (int [B,curve_num,curve_length]) and its start points in `last_start` ([B,curve_num]) on both routes."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import struct

from .._lib import call, f32a, f32c
from .model_common_utils import farthest_point_sample, index_points, knn, query_ball_point, square_distance  # noqa: F401

FUSED_WALK = True
WALK_MAX_C, WALK_MAX_K = 128, 64        # curvenet.hip: CW_MAXC, one lane per candidate


_ACT_LRELU = struct.unpack("<i", struct.pack("<f", 0.2))[0]      # activation code of the conv kernels: the LeakyReLU slope's fp32 bits


def lpfa_group(xyz, x, idx):
    """xyz [B,3,N], x [B,C,N] or None, idx int64 [B,N,k] -> (geo [B,9,N,k], diff [B,C,N,k] or None)"""
    B, _, N = xyz.shape
    k = idx.shape[2]
    p = f32c(xyz.transpose(2, 1))
    geo = torch.empty((B, 9, N, k), dtype=torch.float32, device=xyz.device)
    diff, xc, C = None, None, 0
    if x is not None:
        xc = f32c(x)
        C = xc.shape[1]
        diff = torch.empty((B, C, N, k), dtype=torch.float32, device=xyz.device)
    call("l3d_lpfa_group", p, xc, idx.contiguous(), B, N, C, k, geo, diff)
    return geo, diff


class LPFA(nn.Module):
    """reference: utils/curvenet_util.py:229-291 (same constructor, attribute names and state_dict keys)."""

    def __init__(self, in_channel, out_channel, k, mlp_num=2, initial=False):
        super(LPFA, self).__init__()
        self.k = k
        self.initial = initial
        if not initial:
            self.xyz2feature = nn.Sequential(nn.Conv2d(9, in_channel, kernel_size=1, bias=False), nn.BatchNorm2d(in_channel))
        mlp = []
        for _ in range(mlp_num):
            mlp.append(nn.Sequential(nn.Conv2d(in_channel, out_channel, 1, bias=False), nn.BatchNorm2d(out_channel), nn.LeakyReLU(0.2)))
            in_channel = out_channel
        self.mlp = nn.Sequential(*mlp)

    def _conv_bn(self, seq, h, act):
        """Conv2d + BatchNorm2d (+ LeakyReLU 0.2) of one nn.Sequential: with autograd live on the GPU the HIP conv / dgrad /
        wgrad + BatchNorm layer (models/_train.py), else the torch modules."""
        from ..models._train import conv_bn_act, hip_layers_ok
        if torch.is_grad_enabled() and hip_layers_ok(h) and (h.requires_grad or seq[0].weight.requires_grad):
            return conv_bn_act(h.contiguous(), seq[0], seq[1], relu=(_ACT_LRELU if act else 0))
        return seq(h)

    def forward(self, x, xyz, idx=None):
        x = self.group_feature(x, xyz, idx)
        for seq in self.mlp:
            x = self._conv_bn(seq, x, True)
        return x.max(dim=-1, keepdim=False)[0] if self.initial else x.mean(dim=-1, keepdim=False)

    def group_feature(self, x, xyz, idx):
        if idx is None:
            idx = knn_self(xyz, self.k)[:, :, :self.k]                            # (batch_size, num_points, k)
        grad = torch.is_grad_enabled() and ((x is not None and x.requires_grad) or xyz.requires_grad)
        if grad or not xyz.is_cuda:                                               # autograd / CPU: the reference's op sequence on the HIP kNN
            B, C, N = x.shape
            pts = xyz.transpose(2, 1).contiguous()
            nb = index_points(pts, idx) if pts.is_cuda and not pts.requires_grad else torch.gather(
                pts.unsqueeze(1).expand(B, N, N, 3), 2, idx.unsqueeze(-1).expand(B, N, self.k, 3))
            ctr = pts.view(B, N, 1, 3).expand(-1, -1, self.k, -1)
            geo = torch.cat((ctr, nb, nb - ctr), dim=3).permute(0, 3, 1, 2).contiguous()
            if self.initial:
                return geo
            xt = x.transpose(2, 1)
            feat = torch.gather(xt.unsqueeze(1).expand(B, N, N, C), 2, idx.unsqueeze(-1).expand(B, N, self.k, C)) - xt.unsqueeze(2)
            return F.leaky_relu(feat.permute(0, 3, 1, 2) + self._conv_bn(self.xyz2feature, geo, False), 0.2)
        geo, diff = lpfa_group(xyz, None if self.initial else x, idx)
        if self.initial:
            return geo
        return F.leaky_relu(diff + self.xyz2feature(geo), 0.2)


def _fused():
    from ..models import _fused as m          # imported late: models/ imports this package's utils
    return m


def _fusable(module, *tensors):
    """May `module` launch the fused kernels on these tensors: device fp32, BatchNorm on running statistics, nothing to
    differentiate (models/_fused.fusable)."""
    return FUSED_WALK and _fused().fusable(module, *tensors)


# ---------------------------------------------------------------------------------------------------------------
# the geometry ops: the HIP kernels for device tensors, the reference's torch formulas (utils/model_common_utils.py) for CPU ones
# ---------------------------------------------------------------------------------------------------------------
def knn_self(xyz, k):
    """xyz [B,3,N] -> the k + 1 nearest points of every point, itself included: int64 [B,N,k+1]"""
    if xyz.is_cuda:
        return knn(xyz, k, add_one_to_k=True)
    sq = torch.sum(xyz ** 2, dim=1, keepdim=True)
    inner = -2 * torch.matmul(xyz.transpose(2, 1).contiguous(), xyz)
    return (-sq - inner - sq.transpose(2, 1).contiguous()).topk(k=k + 1, dim=-1)[1]


def _gather_points(points, idx):
    """points [B,N,C], idx [B,S] or [B,S,K] -> [B,S,C] / [B,S,K,C]"""
    if points.is_cuda:
        return index_points(points, idx)
    rows = torch.arange(points.shape[0], dtype=torch.long).view([-1] + [1] * (idx.dim() - 1)).expand_as(idx)
    return points[rows, idx, :]


def _square_distance(a, b):
    if a.is_cuda:
        return square_distance(a, b)
    d = -2 * torch.matmul(a, b.permute(0, 2, 1))
    d = d + torch.sum(a ** 2, -1).unsqueeze(2)
    return d + torch.sum(b ** 2, -1).unsqueeze(1)


def _fps_first(xyz, npoint):
    """farthest point sampling from point 0: xyz [B,N,3] -> int64 [B,npoint]"""
    if xyz.is_cuda:
        return farthest_point_sample(xyz, npoint, start_with_first_point=True)
    B, N, _ = xyz.shape
    picked = torch.zeros(B, npoint, dtype=torch.long)
    nearest = torch.full((B, N), 1e10, dtype=xyz.dtype)
    far = torch.zeros(B, dtype=torch.long)
    rows = torch.arange(B)
    for i in range(npoint):
        picked[:, i] = far
        d = torch.sum((xyz - xyz[rows, far, :].view(B, 1, 3)) ** 2, -1)
        nearest = torch.where(d < nearest, d, nearest)
        far = torch.max(nearest, -1)[1]
    return picked


def _ball_query(radius, nsample, xyz, new_xyz):
    """the first nsample points (in index order) within `radius` of every query, padded with the first: int64 [B,S,nsample]"""
    if xyz.is_cuda:
        return query_ball_point(radius, nsample, xyz, new_xyz, get_cnt=False)
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    idx = torch.arange(N, dtype=torch.long).view(1, 1, N).repeat(B, S, 1)
    idx[_square_distance(new_xyz, xyz) > radius ** 2] = N
    idx = idx.sort(dim=-1)[0][:, :, :nsample]
    first = idx[:, :, :1].expand(-1, -1, nsample)
    return torch.where(idx == N, first, idx)


def sample_and_group(npoint, radius, nsample, xyz, points, returnfps=False):
    """reference: utils/curvenet_util.py:26-50.  xyz [B,N,3], points [B,N,D] -> new_xyz [B,npoint,3], new_points
    [B,npoint,nsample,D] (+ idx).  Without the reference's torch.cuda.empty_cache() calls (:39-45): they only stall the queue."""
    new_xyz = _gather_points(xyz, _fps_first(xyz, npoint))
    idx = _ball_query(radius, nsample, xyz, new_xyz)
    new_points = _gather_points(points, idx)
    return (new_xyz, new_points, idx) if returnfps else (new_xyz, new_points)


def batched_index_select(input, dim, index):
    """reference: utils/curvenet_util.py:52-59.  input [B,...], index [B,M] -> input gathered along `dim` per batch row"""
    shape = [input.shape[0]] + [-1 if i == dim else 1 for i in range(1, input.dim())]
    size = list(input.shape)
    size[0] = -1
    size[dim] = -1
    return torch.gather(input, dim, index.view(shape).expand(size))


def gumbel_softmax(logits, dim, temperature=1):
    """reference: utils/curvenet_util.py:61-76: straight-through one-hot of the softmax, without Gumbel noise"""
    y = F.softmax(logits / temperature, dim=dim)
    ind = y.max(dim=-1)[1]
    hard = torch.zeros_like(y).view(-1, y.shape[-1])
    hard.scatter_(1, ind.view(-1, 1), 1)
    return (hard.view(y.shape) - y).detach() + y


# ---------------------------------------------------------------------------------------------------------------
# the curve modules
# ---------------------------------------------------------------------------------------------------------------
def curve_prepare(x, w_att):
    """x [B,C,N], w_att [C] -> (x sigmoid(w_att . x) as [B,N,C] channel-last, the attention [B,N]): l3d_curve_prepare"""
    x = f32c(x)
    B, C, N = x.shape
    xa = torch.empty((B, N, C), dtype=torch.float32, device=x.device)
    att = torch.empty((B, N), dtype=torch.float32, device=x.device)
    call("l3d_curve_prepare", x, f32c(w_att.reshape(-1)), B, C, N, xa, att)
    return xa, att


def curve_walk(xa, adj, start, params, curve_length):
    """xa [B,N,C] channel-last (already scaled by the attention), adj int64 [B,N,k], start int64 [B,curve_num], params =
    (w_a [2C], a_scale [1], a_shift [1], w_m [2,2C], m_scale [2], m_shift [2]) -> (curves [B,C,curve_num,curve_length], path int32
    [B,curve_num,curve_length]): l3d_curve_walk, one launch"""
    # (f32a: the walk reads the candidates' rows 16 bytes at a time and refuses a misaligned xa -- a contiguous slice is copied)
    xa, adj, start = f32a(xa), adj.to(torch.int64).contiguous(), start.to(torch.int64).contiguous()
    B, N, C = xa.shape
    k, curve_num = adj.shape[2], start.shape[1]
    curves = torch.empty((B, C, curve_num, curve_length), dtype=torch.float32, device=xa.device)
    path = torch.empty((B, curve_num, curve_length), dtype=torch.int32, device=xa.device)
    call("l3d_curve_walk", xa, adj, start, B, N, C, k, curve_num, curve_length, *params, curves, path)
    return curves, path


def select_start(att, curve_num):
    """att [B,N] -> the curve_num points of largest attention, int64 [B,curve_num], in torch.topk(sorted=False)'s order (:510-513).
    That order is an input of the walk (module docstring) and differs between devices; tests replace this function to hand a walk a
    stored list."""
    return torch.topk(att, curve_num, dim=1, sorted=False)[1]


def walk_shape_ok(C, k, curve_num, N, B=1):
    """what curvenet.hip takes: l3d_curve_walk's channel / candidate / LDS limits and l3d_curve_prepare's grid limit on B"""
    if B > 65535:
        return False
    return C % 16 == 0 and C <= WALK_MAX_C and 0 < k <= WALK_MAX_K and 0 < curve_num <= N and curve_num * (2 * C + 3) <= 16384


class Walk(nn.Module):
    """reference: utils/curvenet_util.py:78-195"""

    def __init__(self, in_channel, k, curve_num, curve_length):
        super(Walk, self).__init__()
        self.curve_num = curve_num
        self.curve_length = curve_length
        self.k = k
        self.agent_mlp = nn.Sequential(nn.Conv2d(in_channel * 2, 1, kernel_size=1, bias=False), nn.BatchNorm2d(1))
        self.momentum_mlp = nn.Sequential(nn.Conv1d(in_channel * 2, 2, kernel_size=1, bias=False), nn.BatchNorm1d(2))
        self.last_path = self.last_start = None

    def crossover_suppression(self, cur, neighbor, bn, n, k):
        """cur [bs*n, c], neighbor [bs*n, c, k] -> clamp(1 + cos(cur, neighbor), 0, 1) [bs*n, k], no gradient (:99-114)"""
        neighbor = neighbor.detach()
        cur = cur.unsqueeze(-1).detach()
        dot = torch.bmm(cur.transpose(1, 2), neighbor)
        divider = torch.clamp(torch.norm(cur, dim=1, keepdim=True) * torch.norm(neighbor, dim=1, keepdim=True), min=1e-8)
        return torch.clamp(1. + torch.div(dot, divider).squeeze(1), 0., 1.0).detach()

    def folded(self, device):
        """(w_a, a_scale, a_shift, w_m, m_scale, m_shift) of l3d_curve_walk: the two convs' weights and their BatchNorms folded
        to scale and shift, cached on the module and rebuilt on every parameter / buffer version change (_fused.cached)."""
        fz = _fused()
        conv_a, bn_a = self.agent_mlp[0], self.agent_mlp[1]
        conv_m, bn_m = self.momentum_mlp[0], self.momentum_mlp[1]

        def build():
            sa, ha = fz.bn_affine(bn_a)
            sm, hm = fz.bn_affine(bn_m)
            return tuple(t.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
                         for t in (conv_a.weight, sa, ha, conv_m.weight, sm, hm))
        return fz.cached(self.__dict__, "_l3d_walk", [conv_a.weight] + fz.bn_state(bn_a) + [conv_m.weight] + fz.bn_state(bn_m), build,
                         extra=(str(device),))

    def fusable(self, x, N, k):
        """x: the feature tensor (either layout), N points, k candidates per point"""
        C = self.agent_mlp[0].weight.shape[1] // 2
        return walk_shape_ok(C, k, self.curve_num, N, x.shape[0]) and _fusable(self, x)

    def walk_device(self, xa, adj, start):
        """the fused route on channel-last features: xa [B,N,C], adj [B,N,k], start [B,curve_num] -> curves [B,C,curve_num,length]"""
        curves, self.last_path = curve_walk(xa, adj, start, self.folded(xa.device), self.curve_length)
        self.last_start = start
        return curves

    def forward(self, xyz, x, adj, cur):
        """xyz is not used (the reference's :120 never calls .contiguous and drops the value).  x [B,C,N], adj [B,N,k],
        cur [B,curve_num,1] start points -> curves [B,C,curve_num,curve_length]"""
        bn, c, tot_points = x.size()
        if self.fusable(x, tot_points, adj.shape[2]) and adj.is_cuda and cur.is_cuda:
            return self.walk_device(x.transpose(1, 2).contiguous(), adj, cur.reshape(bn, self.curve_num))
        n, k = self.curve_num, adj.shape[2]
        flat_x = x.transpose(1, 2).contiguous().view(bn * tot_points, -1)
        offset = torch.arange(0, bn, device=x.device) * tot_points               # on the input's device (the reference: :126)
        flat_adj = (adj + offset.view(-1, 1, 1)).view(bn * tot_points, -1)
        flat_cur = (cur + offset.view(-1, 1, 1)).view(-1)
        curves, path = [], []
        cur_feature = cur_cos = None
        for step in range(self.curve_length):
            if step == 0:
                pre_feature = flat_x[flat_cur, :].contiguous().view(bn, n, -1, 1).transpose(1, 2)          # bs, c, n, 1
            else:
                cat = torch.cat((cur_feature.squeeze(-1), pre_feature.squeeze(-1)), dim=1)
                att = F.softmax(self.momentum_mlp(cat), dim=1).view(bn, 1, n, 2)
                pre_feature = torch.sum(torch.cat((cur_feature, pre_feature), dim=-1) * att, dim=-1, keepdim=True)
                pre_cos = pre_feature.transpose(1, 2).contiguous().view(bn * n, -1)
            pick_idx = flat_adj[flat_cur]                                        # bs*n, k
            rows = flat_x[pick_idx.view(-1), :].view(bn * n, k, c)
            pick_values = rows.view(bn, n, k, c).permute(0, 3, 1, 2)             # bs, c, n, k
            rows_cos = rows.transpose(1, 2).contiguous()                         # bs*n, c, k
            logits = self.agent_mlp(torch.cat((pick_values, pre_feature.expand_as(pick_values)), dim=1))    # bs, 1, n, k
            if step != 0:
                d = self.crossover_suppression(cur_cos - pre_cos, rows_cos - cur_cos.unsqueeze(-1), bn, n, k)
                logits = torch.mul(logits, d.view(bn, n, k).unsqueeze(1))
            onehot = gumbel_softmax(logits, -1)
            cur_feature = torch.sum(pick_values * onehot, dim=-1, keepdim=True)  # bs, c, n, 1
            cur_cos = cur_feature.transpose(1, 2).contiguous().view(bn * n, c)
            flat_cur = batched_index_select(pick_idx, 1, torch.argmax(onehot, dim=-1).view(-1, 1)).view(-1)
            curves.append(cur_feature)
            path.append(flat_cur.view(bn, n) - offset.view(-1, 1))
        self.last_path, self.last_start = torch.stack(path, dim=-1).detach(), cur.detach().view(bn, n)
        return torch.cat(curves, dim=-1)


class Attention_block(nn.Module):
    """reference: utils/curvenet_util.py:198-226 (the attention U-Net's gate)"""

    def __init__(self, F_g, F_l, F_int):
        super(Attention_block, self).__init__()
        self.W_g = nn.Sequential(nn.Conv1d(F_g, F_int, kernel_size=1, stride=1, padding=0, bias=True), nn.BatchNorm1d(F_int))
        self.W_x = nn.Sequential(nn.Conv1d(F_l, F_int, kernel_size=1, stride=1, padding=0, bias=True), nn.BatchNorm1d(F_int))
        self.psi = nn.Sequential(nn.Conv1d(F_int, 1, kernel_size=1, stride=1, padding=0, bias=True), nn.BatchNorm1d(1), nn.Sigmoid())

    def forward(self, g, x):
        psi = self.psi(F.leaky_relu(self.W_g(g) + self.W_x(x), negative_slope=0.2))
        return psi, 1. - psi


class PointNetFeaturePropagation(nn.Module):
    """reference: utils/curvenet_util.py:293-354"""

    def __init__(self, in_channel, mlp, att=None):
        super(PointNetFeaturePropagation, self).__init__()
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        self.att = Attention_block(F_g=att[0], F_l=att[1], F_int=att[2]) if att is not None else None
        last_channel = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv1d(last_channel, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm1d(out_channel))
            last_channel = out_channel

    def forward(self, xyz1, xyz2, points1, points2):
        """xyz1 [B,3,N], xyz2 [B,3,S], points1 [B,D,N] or None, points2 [B,D,S] -> [B,D',N]"""
        xyz1, xyz2, points2 = xyz1.permute(0, 2, 1), xyz2.permute(0, 2, 1), points2.permute(0, 2, 1)
        B, N, _ = xyz1.shape
        S = xyz2.shape[1]
        if S == 1:
            interpolated = points2.repeat(1, N, 1)
        else:
            dists, idx = _square_distance(xyz1, xyz2).sort(dim=-1)
            dists, idx = dists[:, :, :3], idx[:, :, :3]
            recip = 1.0 / (dists + 1e-8)
            weight = recip / torch.sum(recip, dim=2, keepdim=True)
            interpolated = torch.sum(_gather_points(points2.contiguous(), idx.contiguous()) * weight.view(B, N, 3, 1), dim=2)
        if self.att is not None:
            psix, _ = self.att(interpolated.permute(0, 2, 1), points1)
            points1 = points1 * psix
        new_points = torch.cat([points1.permute(0, 2, 1), interpolated], dim=-1) if points1 is not None else interpolated
        new_points = new_points.permute(0, 2, 1)
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            new_points = F.leaky_relu(bn(conv(new_points)), 0.2)
        return new_points


def _conv_bn_1d(seq, x, act, fused):
    """Conv1d + BatchNorm1d (+ LeakyReLU 0.2) of one nn.Sequential: the folded 1x1-conv kernel on the fused route, else the modules"""
    if not fused:
        return seq(x)
    fz = _fused()
    w, scale, shift = fz.fold_conv_bn(seq[0], seq[1])
    return fz.pointwise_conv(x, w, scale, shift, relu=_ACT_LRELU if act else 0)


class CIC(nn.Module):
    """reference: utils/curvenet_util.py:357-428"""

    def __init__(self, npoint, radius, k, in_channels, output_channels, bottleneck_ratio=2, mlp_num=2, curve_config=None):
        super(CIC, self).__init__()
        self.in_channels = in_channels
        self.output_channels = output_channels
        self.bottleneck_ratio = bottleneck_ratio
        self.radius = radius
        self.k = k
        self.npoint = npoint
        planes = in_channels // bottleneck_ratio
        self.use_curve = curve_config is not None
        if self.use_curve:
            self.curveaggregation = CurveAggregation(planes)
            self.curvegrouping = CurveGrouping(planes, k, curve_config[0], curve_config[1])
        self.conv1 = nn.Sequential(nn.Conv1d(in_channels, planes, kernel_size=1, bias=False),
                                   nn.BatchNorm1d(in_channels // bottleneck_ratio), nn.LeakyReLU(negative_slope=0.2, inplace=True))
        self.conv2 = nn.Sequential(nn.Conv1d(planes, output_channels, kernel_size=1, bias=False), nn.BatchNorm1d(output_channels))
        if in_channels != output_channels:
            self.shortcut = nn.Sequential(nn.Conv1d(in_channels, output_channels, kernel_size=1, bias=False),
                                          nn.BatchNorm1d(output_channels))
        self.relu = nn.LeakyReLU(negative_slope=0.2, inplace=True)
        self.maxpool = MaskedMaxPool(npoint, radius, k)
        self.lpfa = LPFA(planes, planes, k, mlp_num=mlp_num, initial=False)

    def forward(self, xyz, x):
        """xyz [B,3,N], x [B,C,N] -> (xyz [B,3,npoint], x [B,C',npoint])"""
        if xyz.size(-1) != self.npoint:
            xyz, x = self.maxpool(xyz.transpose(1, 2).contiguous(), x)
            xyz = xyz.transpose(1, 2)
        fused = _fusable(self, xyz, x)
        shortcut = x
        x = _conv_bn_1d(self.conv1, x, True, fused)              # bs, c', n
        idx = knn_self(xyz, self.k)
        if self.use_curve:
            curves = self.curvegrouping(x, xyz, idx[:, :, 1:])  # the first neighbour is the point itself: no self-loop
            x = self.curveaggregation(x, curves)
        x = self.lpfa(x, xyz, idx=idx[:, :, :self.k])
        x = _conv_bn_1d(self.conv2, x, False, fused)
        if self.in_channels != self.output_channels:
            shortcut = _conv_bn_1d(self.shortcut, shortcut, False, fused)
        return xyz, self.relu(x + shortcut)


class CurveAggregation(nn.Module):
    """reference: utils/curvenet_util.py:431-490"""

    def __init__(self, in_channel):
        super(CurveAggregation, self).__init__()
        self.in_channel = in_channel
        mid_feature = in_channel // 2
        self.conva = nn.Conv1d(in_channel, mid_feature, kernel_size=1, bias=False)
        self.convb = nn.Conv1d(in_channel, mid_feature, kernel_size=1, bias=False)
        self.convc = nn.Conv1d(in_channel, mid_feature, kernel_size=1, bias=False)
        self.convn = nn.Conv1d(mid_feature, mid_feature, kernel_size=1, bias=False)
        self.convl = nn.Conv1d(mid_feature, mid_feature, kernel_size=1, bias=False)
        self.convd = nn.Sequential(nn.Conv1d(mid_feature * 2, in_channel, kernel_size=1, bias=False), nn.BatchNorm1d(in_channel))
        self.line_conv_att = nn.Conv2d(in_channel, 1, kernel_size=1, bias=False)

    def forward(self, x, curves):
        """x [B,C,N], curves [B,C,curve_num,curve_length] -> [B,C,N]"""
        curves_att = self.line_conv_att(curves)                                          # bs, 1, c_n, c_l
        inter = torch.sum(curves * F.softmax(curves_att, dim=-1), dim=-1)                # bs, c, c_n
        intra = torch.sum(curves * F.softmax(curves_att, dim=-2), dim=-2)                # bs, c, c_l
        inter, intra = self.conva(inter), self.convb(intra)
        x_logits = self.convc(x).transpose(1, 2).contiguous()
        x_inter = F.softmax(torch.bmm(x_logits, inter), dim=-1)                          # bs, n, c_n
        x_intra = F.softmax(torch.bmm(x_logits, intra), dim=-1)                          # bs, n, c_l
        inter = self.convn(inter).transpose(1, 2).contiguous()
        intra = self.convl(intra).transpose(1, 2).contiguous()
        curve_features = torch.cat((torch.bmm(x_inter, inter), torch.bmm(x_intra, intra)), dim=-1).transpose(1, 2).contiguous()
        return F.leaky_relu(x + self.convd(curve_features), negative_slope=0.2)


class CurveGrouping(nn.Module):
    """reference: utils/curvenet_util.py:493-518"""

    def __init__(self, in_channel, k, curve_num, curve_length):
        super(CurveGrouping, self).__init__()
        self.curve_num = curve_num
        self.curve_length = curve_length
        self.in_channel = in_channel
        self.k = k
        self.att = nn.Conv1d(in_channel, 1, kernel_size=1, bias=False)
        self.walk = Walk(in_channel, k, curve_num, curve_length)

    def forward(self, x, xyz, idx):
        """x [B,C,N], xyz [B,3,N], idx int64 [B,N,k] (no self column) -> curves [B,C,curve_num,curve_length]"""
        if idx.is_cuda and self.walk.fusable(x, x.shape[2], idx.shape[2]) and _fusable(self, x):
            xa, att = curve_prepare(x, self.att.weight.detach())
            return self.walk.walk_device(xa, idx, select_start(att, self.curve_num))
        x_att = torch.sigmoid(self.att(x))
        x = x * x_att
        return self.walk(xyz, x, idx, select_start(x_att.squeeze(1), self.curve_num).unsqueeze(2))


class MaskedMaxPool(nn.Module):
    """reference: utils/curvenet_util.py:521-536"""

    def __init__(self, npoint, radius, k):
        super(MaskedMaxPool, self).__init__()
        self.npoint = npoint
        self.radius = radius
        self.k = k

    def forward(self, xyz, features):
        """xyz [B,N,3], features [B,C,N] -> (sub_xyz [B,npoint,3], the maximum over each ball's k points [B,C,npoint])"""
        sub_xyz, nb = sample_and_group(self.npoint, self.radius, self.k, xyz, features.transpose(1, 2))
        nb = nb.permute(0, 3, 1, 2).contiguous()
        return sub_xyz, torch.squeeze(F.max_pool2d(nb, kernel_size=[1, nb.shape[3]]), -1)
