"""Drop-in for learning3d/models/segmentation.py on MI355X: the per-point classification head over PointNet(global_feat=False)
(reference: models/segmentation.py:6-27).  Same constructor arguments, attribute names and state_dict keys (conv1..4, bn1..3).

The feature model's output there is cat([global.repeat(N), point_feature]) [B,emb+64,N], and conv1 runs over all of it.  The
repeated half is one vector per cloud, so with device fp32 input, BatchNorm on running statistics and nothing to differentiate
    bn1(conv1(cat)) = scale (W1[:, emb:] point_feature) + [scale (W1[:, :emb] global) + shift]
runs as a 64 -> 512 conv with a per-cloud shift (l3d_linear_rows for the bracket): 16/17 of conv1's products and the
[B,emb+64,N] tensor are gone (PointNet.forward_parts hands over the two halves), and conv2..4 run on the folded conv kernels.
Other feature models, train mode, autograd and CPU tensors take the reference's op sequence in torch."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .._lib import on_device_of
from . import _fused


FUSED = True                 # False: the op sequence for every input (A/B in the tests)


class Segmentation(nn.Module):
    def __init__(self, feature_model, num_classes=40):
        super(Segmentation, self).__init__()
        self.feature_model = feature_model
        self.num_classes = num_classes

        self.conv1 = torch.nn.Conv1d(self.feature_model.emb_dims + 64, 512, 1)
        self.conv2 = torch.nn.Conv1d(512, 256, 1)
        self.conv3 = torch.nn.Conv1d(256, 128, 1)
        self.conv4 = torch.nn.Conv1d(128, self.num_classes, 1)
        self.bn1 = nn.BatchNorm1d(512)
        self.bn2 = nn.BatchNorm1d(256)
        self.bn3 = nn.BatchNorm1d(128)

    def forward(self, input_data):
        fm = self.feature_model
        if FUSED and hasattr(fm, "forward_parts") and _fused.fusable(self, input_data):
            with on_device_of(input_data):
                out = _fused.run_guarded(input_data.device, lambda: self._forward_fused(input_data))
            if out is not None:
                return out
        output = self.feature_model(input_data)
        output = F.relu(self.bn1(self.conv1(output)))
        output = F.relu(self.bn2(self.conv2(output)))
        output = F.relu(self.bn3(self.conv3(output)))
        output = self.conv4(output)
        output = output.permute(0, 2, 1)                # B x N x num_classes
        return output

    def _forward_fused(self, input_data):
        parts = self.feature_model.forward_parts(input_data)
        if parts is None:
            return None
        pooled, point_feature = parts                   # [B,emb], [B,64,N]
        emb = pooled.shape[1]
        wg, wp, scale, shift = _fused.conv_column_blocks(self.conv1, self.bn1, emb)
        # the global half comes first in this concatenation: a per-cloud shift [B,512]
        cloud_shift = scale * _fused.rows_affine(pooled, wg) + shift
        x = _fused.pointwise_conv(point_feature, wp, scale, cloud_shift, relu=True)
        for conv, bn in ((self.conv2, self.bn2), (self.conv3, self.bn3)):
            w, sc, sh = _fused.fold_conv_bn(conv, bn)
            x = _fused.pointwise_conv(x, w, sc, sh, relu=True)
        w, _, b = _fused.fold_conv_bn(self.conv4)
        return _fused.pointwise_conv(x, w, None, b, relu=False).permute(0, 2, 1)
