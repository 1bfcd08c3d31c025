"""Drop-in for learning3d/models/prnet.py on MI355X: PRNet (partial-to-partial registration: embedding, pointer network, keypoint
selection, a learned per-cloud softmax temperature, soft correspondences and Kabsch in both directions, iterated).  Same constructor
arguments, attribute names and state_dict keys as the reference (emb_nn.*, attention.model.*, temp_net.nn.{0,1,3,4,6,7,9}.*,
head.reflect, head.temperature): a state dict of the reference's PRNet() loads with strict=True.  forward(src, tgt),
forward(src, tgt, igt4x4) and forward(src, tgt, R, t) return the reference's dict (est_R, est_t, est_T, transformed_source, and
loss with ground truth).

The point embedding with DYNAMIC graphs (reference: models/prnet.py:62-97, class DGCNN).
Unlike models/dgcnn.py (one xyz graph, four convs on its edges), every layer here rebuilds the k-NN graph
in the FEATURE space of the previous layer's output (get_graph_feature on x, x1, x2, x3: C = 3, 64, 64,
128), which is what SURVEY.md 8(f) rank 2 asks for.  Same constructor, attribute / parameter names
(state_dict compatible) and output layout as the reference class.

Inference (eval + no grad), per layer:
  1. idx = knn(h, 20)            C = 3: l3d_knn_graph;  C = 64/128: l3d_knn_feature (bf16x3 GEMM + top-k)
  2. PQ  = [s*W[:, :C] ; s*W[:, C:]] h + [0 ; t]       one l3d_pointwise_conv with 2*Cout rows (BN folded):
           the conv over (neighbour ; centre) is linear, so it is applied to the N points, not the N*k edges
  3. h'  = lrelu(max_j P[idx_j] + Q)                    l3d_edge_gather_max, written into the cat buffer
and conv5 + bn5 + leaky_relu as one GEMM.  No [B,2C,N,k] tensor, no [B,N,N] tensor, k x fewer conv flops.
Training / autograd: the reference's op sequence through torch (HIP kNN + gather underneath).

Routes of PRNet.forward.  FUSED route (`FUSED`, PRNet._forward_fused): device fp32 clouds, eval-mode BatchNorm, nothing to
differentiate (_fused.can_fuse), head 'svd' with cat_sampler 'softmax', emb_nn DGCNN or PointNet, attention Transformer or Identity,
emb_dims % 16 == 0 (and <= 512, clouds of <= 16384 points: the kernels' limits).  Per iteration, with no host read in the loop:
  1. both clouds through emb_nn as one batch of 2B when their sizes match (DGCNN: its fused route above; PointNet: five folded
     Conv + BatchNorm + ReLU layers on _fused.pointwise_conv)
  2. self.attention (the pointer network picks its own route)
  3. l3d_prnet_keypoints: emb + emb_p, the squared norms, the top K in ascending index order, xyz and embedding gathered
     channel-first, and the channel means of the gathered embedding (K = N when num_keypoints == num_subsampled_points)
  4. the temperature head: |mean_src - mean_tgt| (kept as temp_net.feature_disparity), three folded Linear + BatchNorm + ReLU layers
     and the last Linear + ReLU through _fused.rows_affine, the clamp -> [B].  l3d_linear_rows takes Cin % 256 == 0 only: that is
     the first layer at emb_dims 256 / 512 and nothing else; the three 128-input layers (and the first at other widths) run on
     l3d_pointwise_conv with the rows as the points of one cloud
  5. l3d_soft_correspondence_pair: both directions' src_corr; the [K,K] scores never leave the chip
  6. l3d_kabsch for both directions, one batch of 2B when both clouds keep the same number of keypoints
  7. pose composition and the transform of src in torch on [B,3,3] / [B,3,N] tensors
With ground truth the loss terms are torch ops on these device tensors.  The whole forward captures into a graph on one stream.
EVERYTHING ELSE takes the reference's op sequence in torch (CPU tensors, fp64, autograd, train-mode BatchNorm, gumbel_softmax,
head 'mlp', other widths), on the CPU and on the device; with autograd live on device fp32 tensors the head uses the differentiable
HIP pieces (_rows.matmul / _rows.softmax_rows, _KabschFunction) as utils/svd.py does.  In train() mode head.my_iter is incremented
as in the reference.

Deliberate differences from the reference:
  * SVDHead moves R to a module-level `device` there; here R stays on the input's device.
  * the reference cannot run in fp64 (SVDHead builds `diag` as float32 and forward builds float32 poses: "expected m1 and m2 to have
    the same dtype").  Here every constant takes the input's dtype, so `.double()` works.
  * the reference's diag(1, 1, det(V U^T)) and l3d_kabsch's reflection fix (the sign of the determinant) differ only by the
    rounding of det away from +-1.
  * MLPHead calls an undefined `quat2mat` there.  Here it is the (x, y, z, w) conversion of the original PRNet code (`quat2mat`
    below); the head runs on the op-sequence route only.
  * keypoints are returned in ASCENDING index order on every route (topk(sorted=False) leaves the order unspecified; the softmax
    correspondences, the means and Kabsch are invariant to it up to summation order).  On the fused route ties at the K-th value
    go to the lowest index (l3d_mask_select's rule); torch.topk's choice among equal norms is its own.
  * clouds of different sizes are accepted (the reference's gumbel_softmax reshapes assume equal sizes)."""
import math
import struct

import torch
import torch.nn as nn
import torch.nn.functional as F

from .._lib import L3D_PRNET_MAX_N, L3D_SOFTCORR_PAIR_MAX_C, call, f32c, lib, on_device_of
from ..utils.model_common_utils import get_graph_feature, knn
from . import _fused

EDGE_GATHER_MAX_N = 32768       # l3d_edge_gather_max stages a channel row of N floats in LDS (<= 128 KiB); longer clouds take the
                                # per-layer route below (graph feature + conv / BN / max on the HIP layers)
NEG_SLOPE = 0.2                                                           # prnet.py:79-95
ACT_LRELU = struct.unpack("<i", struct.pack("<f", NEG_SLOPE))[0]          # activation code: the slope's fp32 bits


class DGCNN(torch.nn.Module):
    def __init__(self, emb_dims=512):
        super(DGCNN, self).__init__()
        self.conv1 = torch.nn.Conv2d(6, 64, kernel_size=1, bias=False)
        self.conv2 = torch.nn.Conv2d(64 * 2, 64, kernel_size=1, bias=False)
        self.conv3 = torch.nn.Conv2d(64 * 2, 128, kernel_size=1, bias=False)
        self.conv4 = torch.nn.Conv2d(128 * 2, 256, kernel_size=1, bias=False)
        self.conv5 = torch.nn.Conv2d(512, emb_dims, kernel_size=1, bias=False)
        self.bn1 = torch.nn.BatchNorm2d(64)
        self.bn2 = torch.nn.BatchNorm2d(64)
        self.bn3 = torch.nn.BatchNorm2d(128)
        self.bn4 = torch.nn.BatchNorm2d(256)
        self.bn5 = torch.nn.BatchNorm2d(emb_dims)
        self._folded = {}

    def _layer_params(self, name, conv, bn, stacked):
        """BN-folded weights, cached per parameter version.  stacked: [s*W_nbr ; s*W_ctr] [2*Cout, C] and the
        shift [0 ; t];  else the plain folded conv (conv5)."""
        def build():
            w, s, t = _fused.fold_conv_bn(conv, bn)
            w = (w.float() * s.float()[:, None])
            if stacked:
                c = w.shape[1] // 2
                w = torch.cat([w[:, :c], w[:, c:]], dim=0).contiguous()
                t = torch.cat([torch.zeros_like(t), t]).float().contiguous()
                return w, t, None
            w = w.contiguous()
            w_split = _fused.split_rows(w) if (_fused.SPLIT_BF16 and w.is_cuda) else None
            return w, t.float().contiguous(), w_split
        return _fused.cached(self._folded, name, [conv.weight, conv.bias] + _fused.bn_state(bn), build,
                             extra=(stacked, _fused.SPLIT_BF16))

    def forward(self, x):
        return _fused.checkpointed(self, self._forward, x)

    def _forward(self, x):
        batch_size, num_dims, num_points = x.size()
        if _fused.can_fuse(self, x) and x.is_cuda and num_points <= EDGE_GATHER_MAX_N:
            B, N = batch_size, num_points
            cat = torch.empty((B, 512, N), dtype=torch.float32, device=x.device)
            h, lo = x.float().contiguous(), 0
            for name, conv, bn in (("1", self.conv1, self.bn1), ("2", self.conv2, self.bn2),
                                   ("3", self.conv3, self.bn3), ("4", self.conv4, self.bn4)):
                cout = conv.weight.shape[0]
                with _fused.stage("knn"):
                    idx = knn(h, k=20)                                    # get_graph_feature's graph, prnet.py:78-90
                w, t, _ = self._layer_params(name, conv, bn, stacked=True)
                with _fused.stage("edge_pq"):
                    pq = _fused.pointwise_conv(h, w, None, t, relu=0)     # [B, 2*cout, N]
                out = cat[:, lo:lo + cout]
                with _fused.stage("edge_gather_max"):
                    call("l3d_edge_gather_max", pq, idx, B, cout, N, 20, ACT_LRELU, out, 512 * N)
                h = out.contiguous() if name != "4" else None
                lo += cout
            w5, t5, w5_split = self._layer_params("5", self.conv5, self.bn5, stacked=False)
            with _fused.stage("conv5"):
                return _fused.pointwise_conv(cat, w5, None, t5, relu=ACT_LRELU, w_split=w5_split)

        # reference op sequence (prnet.py:76-97); with autograd live on the GPU each Conv2d + BatchNorm + LeakyReLU is the HIP
        # conv / dgrad / wgrad + BatchNorm layer of _train.py
        from ._train import conv_bn_act, conv_bn_act_max, hip_layers_ok
        if hip_layers_ok(x):
            xs = []
            for conv, bn in ((self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3), (self.conv4, self.bn4)):
                x = conv_bn_act_max(get_graph_feature(x).contiguous(), conv, bn, relu=ACT_LRELU)[1]     # only the pooled output is used
                xs.append(x)
            x = conv_bn_act(torch.cat(xs, dim=1), self.conv5, self.bn5, relu=ACT_LRELU)
            return x.view(batch_size, -1, num_points)
        x = get_graph_feature(x)
        x = F.leaky_relu(self.bn1(self.conv1(x)), negative_slope=NEG_SLOPE)
        x1 = x.max(dim=-1, keepdim=True)[0]
        x = get_graph_feature(x1)
        x = F.leaky_relu(self.bn2(self.conv2(x)), negative_slope=NEG_SLOPE)
        x2 = x.max(dim=-1, keepdim=True)[0]
        x = get_graph_feature(x2)
        x = F.leaky_relu(self.bn3(self.conv3(x)), negative_slope=NEG_SLOPE)
        x3 = x.max(dim=-1, keepdim=True)[0]
        x = get_graph_feature(x3)
        x = F.leaky_relu(self.bn4(self.conv4(x)), negative_slope=NEG_SLOPE)
        x4 = x.max(dim=-1, keepdim=True)[0]
        x = torch.cat((x1, x2, x3, x4), dim=1)
        x = F.leaky_relu(self.bn5(self.conv5(x)), negative_slope=NEG_SLOPE).view(batch_size, -1, num_points)
        return x


# ------------------------------------------------------------------------------------------------------------------------------
# The rest of PRNet (reference: models/prnet.py:26-59 and :100-387)
FUSED = True                     # False: the op-sequence route on every input (A/B runs, tests)


def pairwise_distance(src, tgt):
    """prnet.py:26-31"""
    inner = -2 * torch.matmul(src.transpose(2, 1).contiguous(), tgt)
    xx = torch.sum(src ** 2, dim=1, keepdim=True)
    yy = torch.sum(tgt ** 2, dim=1, keepdim=True)
    distances = xx.transpose(2, 1).contiguous() + inner + yy
    return torch.sqrt(distances)


def cycle_consistency(rotation_ab, translation_ab, rotation_ba, translation_ba):
    """prnet.py:33-36"""
    batch_size = rotation_ab.size(0)
    identity = torch.eye(3, device=rotation_ab.device, dtype=rotation_ab.dtype).unsqueeze(0).repeat(batch_size, 1, 1)
    return F.mse_loss(torch.matmul(rotation_ab, rotation_ba), identity) + F.mse_loss(translation_ab, -translation_ba)


def quat2mat(quat):
    """unit quaternions (x, y, z, w) [B,4] -> rotation matrices [B,3,3]: the convention of the original PRNet code"""
    x, y, z, w = quat[:, 0], quat[:, 1], quat[:, 2], quat[:, 3]
    w2, x2, y2, z2 = w * w, x * x, y * y, z * z
    wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
    return torch.stack([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz,
                        2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
                        2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2], dim=1).reshape(quat.size(0), 3, 3)


def _graph_feature_torch(x, k=20):
    """get_graph_feature (utils/model_common_utils.py:3-9, :132-156) in torch ops, for the tensors the HIP one does not take (CPU,
    fp64): x [B,C,N] -> [B,2C,N,k], channels 0..C-1 the neighbour's, C..2C-1 the centre's"""
    x = x.view(*x.size()[:3])
    B, C, N = x.shape
    inner = -2 * torch.matmul(x.transpose(2, 1).contiguous(), x)
    xx = torch.sum(x ** 2, dim=1, keepdim=True)
    idx = (-xx - inner - xx.transpose(2, 1).contiguous()).topk(k=k, dim=-1)[1]
    idx = (idx + torch.arange(0, B, device=x.device).view(-1, 1, 1) * N).view(-1)
    xt = x.transpose(2, 1).contiguous()
    feature = xt.view(B * N, -1)[idx, :].view(B, N, k, C)
    xt = xt.view(B, N, 1, C).repeat(1, 1, k, 1)
    return torch.cat((feature, xt), dim=3).permute(0, 3, 1, 2)


def _dgcnn_op_sequence(net, x):
    """DGCNN.forward's op sequence (prnet.py:76-97) on tensors DGCNN itself does not take (its graph features are HIP only)"""
    batch_size, _, num_points = x.size()
    xs = []
    for conv, bn in ((net.conv1, net.bn1), (net.conv2, net.bn2), (net.conv3, net.bn3), (net.conv4, net.bn4)):
        x = F.leaky_relu(bn(conv(_graph_feature_torch(x))), negative_slope=NEG_SLOPE).max(dim=-1, keepdim=True)[0]
        xs.append(x)
    x = torch.cat(xs, dim=1)
    return F.leaky_relu(net.bn5(net.conv5(x)), negative_slope=NEG_SLOPE).view(batch_size, -1, num_points)


class PointNet(nn.Module):
    """prnet.py:39-59: five bias-free Conv1d + BatchNorm1d + ReLU layers, [B,3,N] -> [B,emb_dims,N]"""

    def __init__(self, emb_dims=512):
        super(PointNet, self).__init__()
        self.conv1 = nn.Conv1d(3, 64, kernel_size=1, bias=False)
        self.conv2 = nn.Conv1d(64, 64, kernel_size=1, bias=False)
        self.conv3 = nn.Conv1d(64, 64, kernel_size=1, bias=False)
        self.conv4 = nn.Conv1d(64, 128, kernel_size=1, bias=False)
        self.conv5 = nn.Conv1d(128, emb_dims, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(64)
        self.bn3 = nn.BatchNorm1d(64)
        self.bn4 = nn.BatchNorm1d(128)
        self.bn5 = nn.BatchNorm1d(emb_dims)

    def forward(self, x):
        layers = ((self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3), (self.conv4, self.bn4), (self.conv5, self.bn5))
        if FUSED and _fused.fusable(self, x):
            for conv, bn in layers:                          # Conv + eval-mode BatchNorm + ReLU as one launch each
                w, s, t = _fused.fold_conv_bn(conv, bn)
                x = _fused.pointwise_conv(x, w, s, t, relu=True)
            return x
        for conv, bn in layers:
            x = F.relu(bn(conv(x)))
        return x


class MLPHead(nn.Module):
    """prnet.py:100-125 (op-sequence route only)"""

    def __init__(self, emb_dims):
        super(MLPHead, self).__init__()
        n_emb_dims = emb_dims
        self.n_emb_dims = n_emb_dims
        self.nn = nn.Sequential(nn.Linear(n_emb_dims * 2, n_emb_dims // 2),
                                nn.BatchNorm1d(n_emb_dims // 2),
                                nn.ReLU(),
                                nn.Linear(n_emb_dims // 2, n_emb_dims // 4),
                                nn.BatchNorm1d(n_emb_dims // 4),
                                nn.ReLU(),
                                nn.Linear(n_emb_dims // 4, n_emb_dims // 8),
                                nn.BatchNorm1d(n_emb_dims // 8),
                                nn.ReLU())
        self.proj_rot = nn.Linear(n_emb_dims // 8, 4)
        self.proj_trans = nn.Linear(n_emb_dims // 8, 3)

    def forward(self, *input):
        src_embedding = input[0]
        tgt_embedding = input[1]
        embedding = torch.cat((src_embedding.max(dim=-1)[0], tgt_embedding.max(dim=-1)[0]), dim=1)    # (the max of the concatenation)
        embedding = self.nn(embedding)
        rotation = self.proj_rot(embedding)
        rotation = rotation / torch.norm(rotation, p=2, dim=1, keepdim=True)
        translation = self.proj_trans(embedding)
        return quat2mat(rotation), translation


class TemperatureNet(nn.Module):
    """prnet.py:128-155"""

    def __init__(self, emb_dims, temp_factor):
        super(TemperatureNet, self).__init__()
        self.n_emb_dims = emb_dims
        self.temp_factor = temp_factor
        self.nn = nn.Sequential(nn.Linear(self.n_emb_dims, 128),
                                nn.BatchNorm1d(128),
                                nn.ReLU(),
                                nn.Linear(128, 128),
                                nn.BatchNorm1d(128),
                                nn.ReLU(),
                                nn.Linear(128, 128),
                                nn.BatchNorm1d(128),
                                nn.ReLU(),
                                nn.Linear(128, 1),
                                nn.ReLU())
        self.feature_disparity = None
        self._folded = {}

    def forward(self, *input):
        src_embedding = input[0]
        tgt_embedding = input[1]
        src_embedding = src_embedding.mean(dim=2)
        tgt_embedding = tgt_embedding.mean(dim=2)
        residual = torch.abs(src_embedding - tgt_embedding)

        self.feature_disparity = residual

        return torch.clamp(self.nn(residual), 1.0 / self.temp_factor, 1.0 * self.temp_factor), residual

    def _layer(self, i, bn_at):
        """Linear nn[i] (+ eval-mode BatchNorm nn[bn_at]) as (w, b) with y = w x + b, cached per parameter / statistic version"""
        lin, bn = self.nn[i], (self.nn[bn_at] if bn_at is not None else None)

        def build():
            w, s, t = _fused.fold_conv_bn(lin, bn)
            return ((w * s[:, None]).contiguous(), t) if s is not None else (w, t)
        return _fused.cached(self._folded, str(i), [lin.weight, lin.bias] + _fused.bn_state(bn), build)

    def rows(self, residual):
        """the head on a device fp32 residual [B,emb_dims] in eval mode -> temperature [B]"""
        h = residual
        for i, bn_at in ((0, 1), (3, 4), (6, 7), (9, None)):
            w, b = self._layer(i, bn_at)
            h = _fused.rows_affine(h, w, b, relu=True)
        return torch.clamp(h.reshape(-1), 1.0 / self.temp_factor, 1.0 * self.temp_factor).contiguous()


class SVDHead(nn.Module):
    """prnet.py:158-215: softmax(temperature <src_emb, tgt_emb> / sqrt(C)) correspondences and Kabsch"""

    def __init__(self, emb_dims, cat_sampler):
        super(SVDHead, self).__init__()
        self.n_emb_dims = emb_dims
        self.cat_sampler = cat_sampler
        self.reflect = nn.Parameter(torch.eye(3), requires_grad=False)
        self.reflect[2, 2] = -1
        self.temperature = nn.Parameter(torch.ones(1) * 0.5, requires_grad=True)
        self.my_iter = torch.ones(1)

    def forward(self, *input):
        from ..utils.svd import _KabschFunction, kabsch
        from . import _rows
        src_embedding = input[0]
        tgt_embedding = input[1]
        src = input[2]
        tgt = input[3]
        batch_size, num_dims, num_points = src.size()
        num_targets = tgt_embedding.size(2)
        temperature = input[4].view(batch_size, 1, 1)
        d_k = src_embedding.size(1)
        live = torch.is_grad_enabled() and any(t.requires_grad for t in (src_embedding, tgt_embedding, src, tgt, temperature))
        hip = _rows.rows_ok(src_embedding, tgt_embedding, src, tgt, temperature) and batch_size <= 65535

        if self.cat_sampler == 'softmax':
            if hip and live and num_targets <= 8192:
                # autograd live on the device: the same op sequence on l3d_bmm_f32 / l3d_softmax_rows, forward and backward
                scores = _rows.matmul(src_embedding.transpose(2, 1), tgt_embedding, 1.0 / math.sqrt(d_k))
                scores = _rows.softmax_rows(temperature * scores)
                src_corr = _rows.matmul(tgt, scores.transpose(2, 1))
            else:
                scores = torch.matmul(src_embedding.transpose(2, 1).contiguous(), tgt_embedding) / math.sqrt(d_k)
                scores = torch.softmax(temperature * scores, dim=2)
                src_corr = torch.matmul(tgt, scores.transpose(2, 1).contiguous())
        elif self.cat_sampler == 'gumbel_softmax':
            scores = torch.matmul(src_embedding.transpose(2, 1).contiguous(), tgt_embedding) / math.sqrt(d_k)
            scores = scores.view(batch_size * num_points, num_targets)
            temperature = temperature.repeat(1, num_points, 1).view(-1, 1)
            scores = F.gumbel_softmax(scores, tau=temperature, hard=True)
            scores = scores.view(batch_size, num_points, num_targets)
            src_corr = torch.matmul(tgt, scores.transpose(2, 1).contiguous())
        else:
            raise Exception('not implemented')

        if hip:
            if torch.is_grad_enabled() and (src_corr.requires_grad or src.requires_grad):
                R, t = _KabschFunction.apply(src, src_corr)
            else:
                R, t = kabsch(src, src_corr)
        else:
            src_centered = src - src.mean(dim=2, keepdim=True)
            src_corr_centered = src_corr - src_corr.mean(dim=2, keepdim=True)
            H = torch.matmul(src_centered, src_corr_centered.transpose(2, 1).contiguous()).cpu()
            u, s, v = torch.svd(H)
            r = torch.matmul(v, u.transpose(2, 1))
            diag = torch.diag_embed(torch.stack([torch.ones_like(s[:, 0]), torch.ones_like(s[:, 0]), torch.det(r).detach()], dim=1))
            R = torch.matmul(torch.matmul(v, diag), u.transpose(2, 1)).contiguous().to(src.device)
            t = torch.matmul(-R, src.mean(dim=2, keepdim=True)) + src_corr.mean(dim=2, keepdim=True)
        if self.training:
            self.my_iter += 1
        return R, t.view(batch_size, 3)


class KeyPointNet(nn.Module):
    """prnet.py:218-243; the keypoints in ascending index order"""

    def __init__(self, num_keypoints):
        super(KeyPointNet, self).__init__()
        self.num_keypoints = num_keypoints

    def forward(self, *input):
        src = input[0]
        tgt = input[1]
        src_embedding = input[2]
        tgt_embedding = input[3]
        num_dims = src_embedding.size(1)
        src_norm = torch.norm(src_embedding, dim=1, keepdim=True)
        tgt_norm = torch.norm(tgt_embedding, dim=1, keepdim=True)
        src_topk_idx = torch.topk(src_norm, k=self.num_keypoints, dim=2, sorted=False)[1].sort(dim=2)[0]
        tgt_topk_idx = torch.topk(tgt_norm, k=self.num_keypoints, dim=2, sorted=False)[1].sort(dim=2)[0]
        src_keypoints_idx = src_topk_idx.repeat(1, 3, 1)
        tgt_keypoints_idx = tgt_topk_idx.repeat(1, 3, 1)
        src_embedding_idx = src_topk_idx.repeat(1, num_dims, 1)
        tgt_embedding_idx = tgt_topk_idx.repeat(1, num_dims, 1)

        src_keypoints = torch.gather(src, dim=2, index=src_keypoints_idx)
        tgt_keypoints = torch.gather(tgt, dim=2, index=tgt_keypoints_idx)

        src_embedding = torch.gather(src_embedding, dim=2, index=src_embedding_idx)
        tgt_embedding = torch.gather(tgt_embedding, dim=2, index=tgt_embedding_idx)
        self.idx = (src_topk_idx[:, 0], tgt_topk_idx[:, 0])        # [B,K] each, ascending: the latest call's keypoints
        return src_keypoints, tgt_keypoints, src_embedding, tgt_embedding


def keypoints(emb, emb_p, xyz, K, want_idx=False, xyz_k=None, mean=None):
    """l3d_prnet_keypoints on device fp32 tensors: emb, emb_p [B,C,N] (emb_p None: zeros), xyz [B,3,N] ->
    (idx int64 [B,K] or None, xyz_k [B,3,K], emb_k [B,C,K], mean [B,C]); xyz_k / mean: tensors to write into"""
    emb, xyz = f32c(emb), f32c(xyz)
    emb_p = f32c(emb_p) if emb_p is not None else None
    B, C, N = emb.shape
    idx = torch.empty((B, K), dtype=torch.int64, device=emb.device) if want_idx else None
    xyz_k = torch.empty((B, 3, K), dtype=torch.float32, device=emb.device) if xyz_k is None else xyz_k
    emb_k = torch.empty((B, C, K), dtype=torch.float32, device=emb.device)
    mean = torch.empty((B, C), dtype=torch.float32, device=emb.device) if mean is None else mean
    call("l3d_prnet_keypoints", emb, emb_p, xyz, B, C, N, K, idx, xyz_k, emb_k, mean)
    return idx, xyz_k, emb_k, mean


def soft_correspondence_pair(src_emb, tgt_emb, src, tgt, temperature, corr_ab=None, corr_ba=None):
    """l3d_soft_correspondence_pair: src_emb [B,C,N], tgt_emb [B,C,M], src [B,3,N], tgt [B,3,M], temperature [B] (device) ->
    (corr_ab [B,3,N], corr_ba [B,3,M]); corr_ab / corr_ba: tensors to write into"""
    src_emb, tgt_emb, src, tgt, temperature = (f32c(t) for t in (src_emb, tgt_emb, src, tgt, temperature))
    B, C, N = src_emb.shape
    M = tgt_emb.shape[2]
    corr_ab = torch.empty((B, 3, N), dtype=torch.float32, device=src.device) if corr_ab is None else corr_ab
    corr_ba = torch.empty((B, 3, M), dtype=torch.float32, device=src.device) if corr_ba is None else corr_ba
    nbytes = lib().l3d_soft_correspondence_pair_workspace_bytes(B, N, M)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=src.device) if nbytes else None
    call("l3d_soft_correspondence_pair", src_emb, tgt_emb, src, tgt, temperature, B, C, N, M, ws, corr_ab, corr_ba)
    return corr_ab, corr_ba


class PRNet(nn.Module):
    def __init__(self, emb_nn='dgcnn', attention='transformer', head='svd', emb_dims=512, num_keypoints=512, num_subsampled_points=768,
                 num_iters=3, cycle_consistency_loss=0.1, feature_alignment_loss=0.1, discount_factor=0.9, input_shape='bnc'):
        super(PRNet, self).__init__()
        from ..utils.transformer import Identity, Transformer
        self.emb_dims = emb_dims
        self.num_keypoints = num_keypoints
        self.num_subsampled_points = num_subsampled_points
        self.num_iters = num_iters
        self.discount_factor = discount_factor
        self.feature_alignment_loss = feature_alignment_loss
        self.cycle_consistency_loss = cycle_consistency_loss
        self.input_shape = input_shape

        if emb_nn == 'pointnet':
            self.emb_nn = PointNet(emb_dims=self.emb_dims)
        elif emb_nn == 'dgcnn':
            self.emb_nn = DGCNN(emb_dims=self.emb_dims)
        else:
            raise Exception('Not implemented')

        if attention == 'identity':
            self.attention = Identity()
        elif attention == 'transformer':
            self.attention = Transformer(emb_dims=self.emb_dims, n_blocks=1, dropout=0.0, ff_dims=1024, n_heads=4)
        else:
            raise Exception("Not implemented")

        self.temp_net = TemperatureNet(emb_dims=self.emb_dims, temp_factor=100)

        if head == 'mlp':
            self.head = MLPHead(emb_dims=self.emb_dims)
        elif head == 'svd':
            self.head = SVDHead(emb_dims=self.emb_dims, cat_sampler='softmax')
        else:
            raise Exception('Not implemented')

        if self.num_keypoints != self.num_subsampled_points:
            self.keypointnet = KeyPointNet(num_keypoints=self.num_keypoints)
        else:
            self.keypointnet = Identity()
        self.keypoint_log = None     # set to a list: every iteration appends its (src, tgt) keypoint indices [B,K], on either route

    def _embed(self, x):
        """emb_nn(x); DGCNN's graph features are HIP only, so CPU and fp64 clouds take its op sequence in torch"""
        if type(self.emb_nn) is DGCNN and not (x.is_cuda and x.dtype == torch.float32):
            return _dgcnn_op_sequence(self.emb_nn, x)
        return self.emb_nn(x)

    def predict_embedding(self, *input):
        src = input[0]
        tgt = input[1]
        src_embedding = self._embed(src)
        tgt_embedding = self._embed(tgt)

        src_embedding_p, tgt_embedding_p = self.attention(src_embedding, tgt_embedding)

        src_embedding = src_embedding + src_embedding_p
        tgt_embedding = tgt_embedding + tgt_embedding_p

        src, tgt, src_embedding, tgt_embedding = self.keypointnet(src, tgt, src_embedding, tgt_embedding)
        if self.keypoint_log is not None and isinstance(self.keypointnet, KeyPointNet):
            self.keypoint_log.append(self.keypointnet.idx)

        temperature, feature_disparity = self.temp_net(src_embedding, tgt_embedding)

        return src, tgt, src_embedding, tgt_embedding, temperature, feature_disparity

    # Single Pass Alignment Module for PRNet
    def spam(self, *input):
        src, tgt, src_embedding, tgt_embedding, temperature, feature_disparity = self.predict_embedding(*input)
        rotation_ab, translation_ab = self.head(src_embedding, tgt_embedding, src, tgt, temperature)
        rotation_ba, translation_ba = self.head(tgt_embedding, src_embedding, tgt, src, temperature)
        return rotation_ab, translation_ab, rotation_ba, translation_ba, feature_disparity

    def predict_keypoint_correspondence(self, *input):
        src, tgt, src_embedding, tgt_embedding, temperature, _ = self.predict_embedding(*input)
        batch_size, num_dims, num_points = src.size()
        num_targets = tgt.size(2)
        d_k = src_embedding.size(1)
        scores = torch.matmul(src_embedding.transpose(2, 1).contiguous(), tgt_embedding) / math.sqrt(d_k)
        scores = scores.view(batch_size * num_points, num_targets)
        temperature = temperature.view(batch_size, 1, 1).repeat(1, num_points, 1).view(-1, 1)
        scores = F.gumbel_softmax(scores, tau=temperature, hard=True)
        scores = scores.view(batch_size, num_points, num_targets)
        return src, tgt, scores

    # ------------------------------------------------------------------------------------------------------------------
    def _fusable(self, src, tgt):
        """the fused route's gate (module docstring); src, tgt channel-first"""
        from ..utils.transformer import Identity, Transformer
        if not (FUSED and src.is_cuda and tgt.is_cuda and src.dtype == torch.float32 and tgt.dtype == torch.float32):
            return False
        if not (isinstance(self.head, SVDHead) and self.head.cat_sampler == 'softmax' and type(self.emb_nn) in (DGCNN, PointNet)
                and type(self.attention) in (Transformer, Identity) and type(self.keypointnet) in (KeyPointNet, Identity)):
            return False
        C, N, M = self.emb_dims, src.size(2), tgt.size(2)
        if C % 16 or not 16 <= C <= L3D_SOFTCORR_PAIR_MAX_C or src.size(0) != tgt.size(0) or src.size(0) > 32767 or src.size(1) != 3:
            return False
        if isinstance(self.keypointnet, KeyPointNet) and not (self.num_keypoints <= min(N, M) and max(N, M) <= L3D_PRNET_MAX_N):
            return False
        return _fused.can_fuse(self, src, tgt)

    def _spam_fused(self, src, tgt):
        """one iteration on the fused route: src [B,3,N], tgt [B,3,M] contiguous device fp32 -> spam's outputs"""
        from ..utils.svd import kabsch
        B, _, N = src.shape
        M, C, dev = tgt.shape[2], self.emb_dims, src.device
        with _fused.stage("prnet_embed"):
            if N == M:
                emb = self.emb_nn(torch.cat([src, tgt], dim=0))
                src_embedding, tgt_embedding = emb[:B], emb[B:]
            else:
                src_embedding, tgt_embedding = self.emb_nn(src), self.emb_nn(tgt)
        with _fused.stage("prnet_attention"):
            src_embedding_p, tgt_embedding_p = self.attention(src_embedding, tgt_embedding)
        ranked = isinstance(self.keypointnet, KeyPointNet)
        Ks, Kt = (self.num_keypoints, self.num_keypoints) if ranked else (N, M)
        same = Ks == Kt
        # both directions' points and correspondences side by side: Kabsch then runs once on 2B clouds
        pts = torch.empty((2 * B, 3, Ks), dtype=torch.float32, device=dev) if same else None
        corr = torch.empty((2 * B, 3, Ks), dtype=torch.float32, device=dev) if same else None
        mean = torch.empty((2, B, C), dtype=torch.float32, device=dev)
        log = self.keypoint_log is not None and ranked
        with _fused.stage("prnet_keypoints"):
            si, src_k, src_emb_k, _ = keypoints(src_embedding, src_embedding_p, src, Ks, log, pts[:B] if same else None, mean[0])
            ti, tgt_k, tgt_emb_k, _ = keypoints(tgt_embedding, tgt_embedding_p, tgt, Kt, log, pts[B:] if same else None, mean[1])
        if log:
            self.keypoint_log.append((si, ti))
        with _fused.stage("prnet_temperature"):
            feature_disparity = torch.abs(mean[0] - mean[1])
            self.temp_net.feature_disparity = feature_disparity
            temperature = self.temp_net.rows(feature_disparity)
        with _fused.stage("prnet_softcorr_pair"):
            corr_ab, corr_ba = soft_correspondence_pair(src_emb_k, tgt_emb_k, src_k, tgt_k, temperature,
                                                        corr_ab=corr[:B] if same else None, corr_ba=corr[B:] if same else None)
        with _fused.stage("prnet_kabsch"):
            if same:
                R, t = kabsch(pts, corr)
                return R[:B], t[:B], R[B:], t[B:], feature_disparity
            rotation_ab, translation_ab = kabsch(src_k, corr_ab)
            rotation_ba, translation_ba = kabsch(tgt_k, corr_ba)
        return rotation_ab, translation_ab, rotation_ba, translation_ba, feature_disparity

    def _forward_fused(self, src, tgt, rotation_ab=None, translation_ab=None):
        """the iteration loop on the fused route (src, tgt channel-first); no host read anywhere in it"""
        return self._loop(self._spam_fused, f32c(src), f32c(tgt), rotation_ab, translation_ab)

    def _loop(self, spam, src, tgt, rotation_ab, translation_ab):
        """prnet.py:335-387 on channel-first clouds, constants in the clouds' dtype"""
        calculate_loss = rotation_ab is not None
        batch_size = src.size(0)
        kw = dict(device=src.device, dtype=src.dtype)
        identity = torch.eye(3, **kw).unsqueeze(0).repeat(batch_size, 1, 1)

        rotation_ab_pred = torch.eye(3, **kw).view(1, 3, 3).repeat(batch_size, 1, 1)
        translation_ab_pred = torch.zeros(3, **kw).view(1, 3).repeat(batch_size, 1)

        rotation_ba_pred = torch.eye(3, **kw).view(1, 3, 3).repeat(batch_size, 1, 1)
        translation_ba_pred = torch.zeros(3, **kw).view(1, 3).repeat(batch_size, 1)

        total_loss = 0
        total_feature_alignment_loss = 0
        total_cycle_consistency_loss = 0

        for i in range(self.num_iters):
            rotation_ab_pred_i, translation_ab_pred_i, rotation_ba_pred_i, translation_ba_pred_i, feature_disparity = spam(src, tgt)

            rotation_ab_pred = torch.matmul(rotation_ab_pred_i, rotation_ab_pred)
            translation_ab_pred = torch.matmul(rotation_ab_pred_i, translation_ab_pred.unsqueeze(2)).squeeze(2) + translation_ab_pred_i

            rotation_ba_pred = torch.matmul(rotation_ba_pred_i, rotation_ba_pred)
            translation_ba_pred = torch.matmul(rotation_ba_pred_i, translation_ba_pred.unsqueeze(2)).squeeze(2) + translation_ba_pred_i

            if calculate_loss:
                loss = (F.mse_loss(torch.matmul(rotation_ab_pred.transpose(2, 1), rotation_ab), identity)
                        + F.mse_loss(translation_ab_pred, translation_ab)) * self.discount_factor ** i

                feature_alignment_loss = feature_disparity.mean() * self.feature_alignment_loss * self.discount_factor ** i
                cycle_consistency_loss = cycle_consistency(rotation_ab_pred_i, translation_ab_pred_i,
                                                           rotation_ba_pred_i, translation_ba_pred_i) \
                    * self.cycle_consistency_loss * self.discount_factor ** i

                total_feature_alignment_loss += feature_alignment_loss
                total_cycle_consistency_loss += cycle_consistency_loss
                total_loss = total_loss + loss + feature_alignment_loss + cycle_consistency_loss

            # transform_point_cloud (ops/transform_functions.py:24-29) on the channel-first cloud
            src = torch.matmul(rotation_ab_pred_i, src) + translation_ab_pred_i.unsqueeze(2)

        # convert2transformation (ops/transform_functions.py:31-35), built on the device: nothing is copied from the host
        est_T = torch.zeros((batch_size, 4, 4), **kw)
        est_T[:, :3, :3], est_T[:, :3, 3], est_T[:, 3, 3] = rotation_ab_pred, translation_ab_pred, 1.0
        result = {'est_R': rotation_ab_pred,
                  'est_t': translation_ab_pred,
                  'est_T': est_T,
                  'transformed_source': src.permute(0, 2, 1) if self.input_shape == 'bnc' else src}

        if calculate_loss:
            result['loss'] = total_loss
        return result

    def forward(self, *input):
        rotation_ab = translation_ab = None
        if len(input) == 2:
            src, tgt = input[0], input[1]
        elif len(input) == 3:
            src, tgt, rotation_ab, translation_ab = input[0], input[1], input[2][:, :3, :3], input[2][:, :3, 3].view(-1, 3)
        elif len(input) == 4:
            src, tgt, rotation_ab, translation_ab = input[0], input[1], input[2], input[3]
        else:
            raise TypeError("PRNet.forward takes (src, tgt), (src, tgt, igt) or (src, tgt, rotation_ab, translation_ab)")

        if self.input_shape == 'bnc':
            src, tgt = src.permute(0, 2, 1), tgt.permute(0, 2, 1)

        if self._fusable(src, tgt):
            # one range verdict for the whole forward (_fused.run_guarded): the nested models run straight through
            with on_device_of(src):
                return _fused.run_guarded(src.device, lambda: self._forward_fused(src, tgt, rotation_ab, translation_ab))
        return self._loop(self.spam, src, tgt, rotation_ab, translation_ab)
