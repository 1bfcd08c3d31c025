"""Drop-in for learning3d/models/pointconv.py on MI355X: the PointConv classifier / embedding network.  Three
PointConvDensitySetAbstraction layers (utils/pointconv_util.py: 1024 -> 512 centres of 32 neighbours -> 128 centres of 64 ->
one group of all 128) give one emb_dims vector per cloud; the optional head is Linear + BatchNorm1d + ReLU (+ Dropout) twice, a
Linear and log_softmax.  PointConvDensityClsSsg and create_pointconv keep the reference's constructor arguments, attribute names
and state_dict keys (sa{1,2,3}.*, fc{1,2,3}.*, bn{1,2}.*), so its checkpoints load with strict=True.

Routes.  Each set-abstraction layer picks its own (pointconv_util.FUSED, `fusable`): on device fp32 tensors in eval mode with
nothing to differentiate, the fused one (conv kernels, l3d_pointconv_aggregate, a split-K l3d_bmm_f32 for the Linear); else the
reference's op sequence, which also runs on the CPU and in fp64.  The head follows the same gate: eval mode, device fp32, no
gradient -> the rows product of models/_rows.py (l3d_bmm_f32, K split) with the BatchNorm folded into a scale and shift behind
it (pointconv_util.linear_bn_relu); else torch modules.

Deliberate differences from the reference:
  * create_pointconv(classifier=True, pretrained=<path>) returns a class there whose __init__ calls `super(PointConv, self)`
    with `PointConv` undefined: it cannot be instantiated.  Here that class works: it wraps a PointConvDensityClsSsg as
    `self.pointconv` (the reference's attribute name) and `use_pretrained` loads checkpoint['model_state_dict'] into it.
  * PointConvDensityClsSsg ignores its `pretrained` argument there.  Here a path given with classifier=True is loaded the same
    way (`use_pretrained`); without a classifier it is ignored as in the reference (the stock checkpoint carries the head's keys).
  * the neighbours of a centre are gathered nearest first (the reference's topk(sorted=False) leaves the order open): the sum
    over the neighbours is the same up to rounding."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..utils.pointconv_util import PointConvDensitySetAbstraction, linear_bn_relu
from . import _fused


class PointConvDensityClsSsg(torch.nn.Module):
    def __init__(self, emb_dims=1024, input_shape="bnc", input_channel_dim=3, classifier=False, num_classes=40, pretrained=None):
        super(PointConvDensityClsSsg, self).__init__()
        if input_shape not in ["bnc", "bcn"]:
            raise ValueError("Allowed shapes are 'bcn' (batch * channels * num_in_points), 'bnc' ")
        self.input_shape = input_shape
        self.emb_dims = emb_dims
        self.classifier = classifier
        self.input_channel_dim = input_channel_dim
        self.create_structure()
        if self.classifier:
            self.create_classifier(num_classes)
            if pretrained is not None:
                self.use_pretrained(pretrained)

    def create_structure(self):
        # npoint: centres sampled; nsample: neighbours per centre; in_channel: input channels (xyz included); mlp: widths of the
        # shared MLP; bandwidth: of the Gaussian density estimate; group_all: one group holding the whole cloud
        self.sa1 = PointConvDensitySetAbstraction(npoint=512, nsample=32, in_channel=self.input_channel_dim,
                                                  mlp=[64, 64, 128], bandwidth=0.1, group_all=False)
        self.sa2 = PointConvDensitySetAbstraction(npoint=128, nsample=64, in_channel=128 + 3,
                                                  mlp=[128, 128, 256], bandwidth=0.2, group_all=False)
        self.sa3 = PointConvDensitySetAbstraction(npoint=1, nsample=None, in_channel=256 + 3,
                                                  mlp=[256, 512, self.emb_dims], bandwidth=0.4, group_all=True)

    def create_classifier(self, num_classes):
        self.fc1 = nn.Linear(self.emb_dims, 512)
        self.bn1 = nn.BatchNorm1d(512)
        self.drop1 = nn.Dropout(0.7)
        self.fc2 = nn.Linear(512, 256)
        self.bn2 = nn.BatchNorm1d(256)
        self.drop2 = nn.Dropout(0.7)
        self.fc3 = nn.Linear(256, num_classes)

    def use_pretrained(self, pretrained):
        checkpoint = torch.load(pretrained, map_location='cpu')
        self.load_state_dict(checkpoint['model_state_dict'])

    def _head_rows(self, features):
        """the head on the rows kernels: y = max(0, scale (x W^T) + shift) twice (Linear bias and BatchNorm folded), then fc3"""
        features = linear_bn_relu(features, self.fc1, self.bn1)
        features = linear_bn_relu(features, self.fc2, self.bn2)
        return linear_bn_relu(features, self.fc3, None)

    def forward(self, input_data):
        if self.input_shape == "bnc":
            input_data = input_data.permute(0, 2, 1)
        batch_size = input_data.shape[0]
        points = input_data[:, 3:, :] if input_data.shape[1] > 3 else None      # (the reference passes an empty [B,0,N] slice on)
        l1_points, l1_features = self.sa1(input_data[:, :3, :], points)
        l2_points, l2_features = self.sa2(l1_points, l1_features)
        l3_points, l3_features = self.sa3(l2_points, l2_features)
        features = l3_features.view(batch_size, self.emb_dims)
        if not self.classifier:
            return features
        if _fused.fusable(self, features):
            features = self._head_rows(features)
        else:
            features = self.drop1(F.relu(self.bn1(self.fc1(features))))
            features = self.drop2(F.relu(self.bn2(self.fc2(features))))
            features = self.fc3(features)
        return F.log_softmax(features, -1)


def create_pointconv(classifier=False, pretrained=None):
    if classifier and pretrained is not None:
        class Network(torch.nn.Module):
            def __init__(self, emb_dims=1024, input_shape="bnc", input_channel_dim=3, classifier=False, num_classes=40, pretrained=None):
                super().__init__()
                self.pointconv = PointConvDensityClsSsg(emb_dims, input_shape, input_channel_dim, classifier, num_classes)
                if classifier and pretrained is not None:
                    self.use_pretrained(pretrained)

            def use_pretrained(self, pretrained):
                checkpoint = torch.load(pretrained, map_location='cpu')
                self.pointconv.load_state_dict(checkpoint['model_state_dict'])

            def forward(self, input_data):
                return self.pointconv(input_data)
        return Network

    class Network(PointConvDensityClsSsg):
        def __init__(self, emb_dims=1024, input_shape="bnc", input_channel_dim=3, classifier=False, num_classes=40, pretrained=None):
            super().__init__(emb_dims=emb_dims, input_shape=input_shape, input_channel_dim=input_channel_dim, classifier=classifier,
                             num_classes=num_classes, pretrained=pretrained)
    return Network
