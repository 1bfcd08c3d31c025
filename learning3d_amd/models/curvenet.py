"""Drop-in for learning3d/models/curvenet.py on MI355X: the CurveNet classifier (ModelNet40 0.938 in BASELINE.md).  Same
constructor arguments, attribute names and state_dict keys as the reference, so its checkpoints load with strict=True.

Every block picks its route by itself (utils/curvenet_util.py): with device fp32 input, BatchNorm on running statistics and
nothing to differentiate, the four curve blocks of the 'default' setting run one l3d_curve_walk each, the 1x1 convs run on the
folded conv kernels and the geometry on the HIP kNN / grouping kernels, with no host read in the forward; anything else
(CPU tensors, autograd, train mode) takes the reference's op sequence in torch.

The reference hard-codes npoint = 1024 for stages 1-2 (models/curvenet.py:65-69): clouds of another size are first resampled to
1024 points by MaskedMaxPool, exactly as there."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..utils.curvenet_util import CIC, LPFA, _fusable

curve_config = {
    'default': [[100, 5], [100, 5], None, None],
    'long': [[10, 30], None, None, None],
}


class CurveNet(nn.Module):
    def __init__(self, num_classes=40, k=20, setting='default', input_shape="bnc"):
        super(CurveNet, self).__init__()
        if input_shape not in ["bcn", "bnc"]:
            raise ValueError("Allowed shapes are 'bcn' (batch * channels * num_in_points), 'bnc' ")
        self.input_shape = input_shape
        assert setting in curve_config
        cfg = curve_config[setting]
        additional_channel = 32
        self.lpfa = LPFA(9, additional_channel, k=k, mlp_num=1, initial=True)

        def cic(npoint, radius, cin, cout, ratio, stage):
            return CIC(npoint=npoint, radius=radius, k=k, in_channels=cin, output_channels=cout, bottleneck_ratio=ratio, mlp_num=1,
                       curve_config=cfg[stage])
        self.cic11 = cic(1024, 0.05, additional_channel, 64, 2, 0)
        self.cic12 = cic(1024, 0.05, 64, 64, 4, 0)
        self.cic21 = cic(1024, 0.05, 64, 128, 2, 1)
        self.cic22 = cic(1024, 0.1, 128, 128, 4, 1)
        self.cic31 = cic(256, 0.1, 128, 256, 2, 2)
        self.cic32 = cic(256, 0.2, 256, 256, 4, 2)
        self.cic41 = cic(64, 0.2, 256, 512, 2, 3)
        self.cic42 = cic(64, 0.4, 512, 512, 4, 3)

        self.conv0 = nn.Sequential(nn.Conv1d(512, 1024, kernel_size=1, bias=False), nn.BatchNorm1d(1024), nn.ReLU(inplace=True))
        self.conv1 = nn.Linear(1024 * 2, 512, bias=False)
        self.conv2 = nn.Linear(512, num_classes)
        self.bn1 = nn.BatchNorm1d(512)
        self.dp1 = nn.Dropout(p=0.5)

    def forward(self, xyz):
        if self.input_shape == 'bnc':
            xyz = xyz.permute(0, 2, 1)
        points = self.lpfa(xyz, xyz)
        for block in (self.cic11, self.cic12, self.cic21, self.cic22, self.cic31, self.cic32, self.cic41, self.cic42):
            xyz, points = block(xyz, points)
        if _fusable(self, points):
            from . import _fused
            w, scale, shift = _fused.fold_conv_bn(self.conv0[0], self.conv0[1])
            x = _fused.pointwise_conv(points, w, scale, shift, relu=True)
        else:
            x = self.conv0(points)
        x = torch.cat((F.adaptive_max_pool1d(x, 1), F.adaptive_avg_pool1d(x, 1)), dim=1).squeeze(-1)
        x = F.relu(self.bn1(self.conv1(x).unsqueeze(-1)), inplace=True).squeeze(-1)
        return self.conv2(self.dp1(x))
