"""PRNet's point embedding with DYNAMIC graphs on MI355X (reference: models/prnet.py:62-97, class DGCNN).

Unlike models/dgcnn.py (one xyz graph, four convs on its edges), every layer here rebuilds the k-NN graph
in the FEATURE space of the previous layer's output (get_graph_feature on x, x1, x2, x3: C = 3, 64, 64,
128), which is what SURVEY.md 8(f) rank 2 asks for.  Same constructor, attribute / parameter names
(state_dict compatible) and output layout as the reference class.  The rest of PRNet (keypoint sampling,
Gumbel-softmax correspondences, the actor-critic loop, prnet.py:100-396) is outside this round's scope.

Inference (eval + no grad), per layer:
  1. idx = knn(h, 20)            C = 3: l3d_knn_graph;  C = 64/128: l3d_knn_feature (bf16x3 GEMM + top-k)
  2. PQ  = [s*W[:, :C] ; s*W[:, C:]] h + [0 ; t]       one l3d_pointwise_conv with 2*Cout rows (BN folded):
           the conv over (neighbour ; centre) is linear, so it is applied to the N points, not the N*k edges
  3. h'  = lrelu(max_j P[idx_j] + Q)                    l3d_edge_gather_max, written into the cat buffer
and conv5 + bn5 + leaky_relu as one GEMM.  No [B,2C,N,k] tensor, no [B,N,N] tensor, k x fewer conv flops.
Training / autograd: the reference's op sequence through torch (HIP kNN + gather underneath)."""
import struct

import torch
import torch.nn.functional as F

from .._lib import call
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
