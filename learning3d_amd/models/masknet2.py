"""Drop-in for learning3d/models/masknet2.py on MI355X: MaskNet2, MaskNet's successor, which masks BOTH clouds of a pair (reference:
models/masknet2.py; examples/test_masknet2.py).  Mish, BasicConv1D, Self_Attn, PointNet, self_attention_fc, PointNetMask and MaskNet2
have the reference's constructor arguments, attribute names and state_dict keys (maskNet.feature_model.conv{1..5}.*,
maskNet.global_feat_{1,2,3}.*, maskNet.h3.{0..3}.*: 76 keys), so its checkpoints load with strict=True.

Deliberate differences:
  * A fresh feature model per default-constructed instance.  The reference's default arguments (`feature_model=PointNet()`) are
    evaluated once, so all its default-constructed instances share ONE module; the keys are the same either way.
  * MaskNet2.forward works on the GPU (the reference leaves `device` unset there and raises NameError) and raises ValueError for
    B != 1, which the reference's boolean indexing cannot express.  The selected indices, ascending, are kept in
    `template_idx` / `source_idx` ([1, count] int64).
  * Clouds of different sizes are accepted on both routes: each global feature is repeated to the OTHER cloud's point count.  The
    reference repeats the source's global feature `num_points` of the source onto the template's features (:198-201) and raises
    unless both clouds have the same number of points; for equal sizes the two rules are the same.

With device fp32 clouds, BatchNorm on running statistics and nothing to differentiate (_fused.can_fuse), the forward is
  * both clouds as one batch of 2B through the feature model when they have the same number of points,
  * per Self_Attn: the folded Conv+BN on the conv kernels, l3d_mish in place, l3d_self_attention_shared -- the [B,N,N] scores, their
    softmax and the second bmm of the reference (:59-68) never exist,
  * per self_attention_fc: ONE l3d_linear_rows over the 2B stacked vectors (BN folded into the weight rows), l3d_mish,
    l3d_outer_softmax_mix -- no [B,C,C] tensor,
  * h3[0] over the point features alone: the other cloud's global feature is the same for every point, so
    bn(W [t ; g]) = scale (W[:, :Ct] t) + (scale (W[:, Ct:] g) + shift), a per-cloud shift from l3d_linear_rows -- half of the
    largest GEMM and both [B,1024,N] concatenations are gone,
  * h3[1], h3[2] on the conv kernels with l3d_mish behind each; h3[3] and the sigmoid stay torch ops ([B,128,N] is tiny),
  * the selection and the gather as one l3d_mask_select launch per cloud (models/masknet.py).
Anything else (CPU tensors, autograd, train-mode BatchNorm) takes the reference's op sequence in torch, with one more difference:
  * when a Self_Attn output is differentiated, its scores q^T q and their softmax are computed in fp64 (SCORES_FP64_FOR_GRAD) and the
    weights cast back.  The logits are unscaled and reach several hundred, where one fp32 ulp (6e-5 at 583) is already a relative
    error of that size in the softmax's weights; in fp32 the clouds' gradients miss fp64 by 1.1e-5 .. 1.5e-5 of their scale, with
    fp64 scores by 4e-6.  It costs the score tensor twice its size during training; forwards without a gradient are unchanged."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .._lib import call, f32c, on_device_of
from . import _fused
from .masknet import MaskNet, mask_select
from .pooling import Pooling

FUSED = True                 # False: the op sequence for every input (A/B: tools/masknet2_bench.py)
SCORES_FP64_FOR_GRAD = True  # Self_Attn, when its output is differentiated: q^T q and its softmax in fp64 (the [B,N,N] tensor twice as large)


def _fusable(module, *tensors):
    """device fp32 tensors, BatchNorm on running statistics, nothing to differentiate"""
    return FUSED and _fused.fusable(module, *tensors)


def mish_(x):
    """l3d_mish in place on a contiguous fp32 device tensor"""
    call("l3d_mish", x, x.numel(), x)
    return x


class Mish(nn.Module):
    def __init__(self):
        super(Mish, self).__init__()

    def forward(self, x):
        return x * torch.tanh(F.softplus(x))


class BasicConv1D(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, active=True):
        super(BasicConv1D, self).__init__()
        self.active = active
        self.bn = nn.BatchNorm1d(out_channels)
        if self.active == True:      # noqa: E712  (the reference's test: only the value True activates)
            self.activation = Mish()
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size, stride, bias=False)

    def forward(self, x):
        x = self.conv(x)
        x = self.bn(x)
        if self.active == True:      # noqa: E712
            x = self.activation(x)
        return x

    def fused(self, x, channel_last=False, shift=None):
        """the folded conv, then l3d_mish in place: x [B,Cin,N] (or [B,N,Cin]) -> [B,Cout,N].  shift: a per-cloud [B,Cout] shift that
        replaces the folded one (PointNetMask's h3[0])"""
        w, scale, sh = _fused.fold_conv_bn(self.conv, self.bn)
        y = _fused.pointwise_conv(x, w, scale, sh if shift is None else shift, relu=False, channel_last=channel_last)
        return mish_(y) if self.active == True else y      # noqa: E712

    def folded_rows(self):
        """(w', b') with bn(conv(v)) = w' v + b' for a vector v: the BN scale folded into the weight rows (cached per state)"""
        def build():
            w, scale, shift = _fused.fold_conv_bn(self.conv, self.bn)
            return (scale[:, None] * w).contiguous(), shift
        return _fused.cached(self.__dict__, "_l3d_rows", [self.conv.weight] + _fused.bn_state(self.bn), build)


class Self_Attn(nn.Module):
    """q = query_conv(x) is query, key and value at once: out = q + beta * softmax(q^T q) applied to q, logits unscaled"""

    def __init__(self, in_dim, out_dim):
        super(Self_Attn, self).__init__()
        self.in_dim = in_dim
        self.out_dim = out_dim
        self.query_conv = BasicConv1D(in_dim, out_dim)
        self.beta = nn.Parameter(torch.zeros(1))
        self.softmax = nn.Softmax(dim=-1)

    def forward(self, x):
        """x [B,in_dim,N] -> [B,out_dim,N]: q + beta * (softmax(q^T q) applied to q), q = query_conv(x)"""
        proj_query = self.query_conv(x).permute(0, 2, 1)      # [B,N,C]
        proj_key = proj_query.permute(0, 2, 1)                # [B,C,N]
        if SCORES_FP64_FOR_GRAD and proj_key.dtype == torch.float32 and torch.is_grad_enabled() and proj_key.requires_grad:
            # the differentiable route keeps the scores in fp64: an unscaled logit of several hundred has an fp32 ulp near 6e-5, which
            # the softmax turns into a relative error of that size in every weight and the backward into 1e-5 of the clouds' gradients
            q64 = proj_key.double()
            attention = self.softmax(torch.bmm(q64.permute(0, 2, 1), q64)).to(proj_key.dtype)
        else:
            energy = torch.bmm(proj_query, proj_key)          # [B,N,N]
            attention = self.softmax(energy)
        out_x = torch.bmm(proj_key, attention.permute(0, 2, 1))
        return self.beta * out_x + proj_key

    def fused(self, x, channel_last=False):
        q = self.query_conv.fused(x, channel_last)
        B, D, N = q.shape
        out = torch.empty_like(q)
        call("l3d_self_attention_shared", q, self.beta.detach(), B, D, N, out)       # beta: the parameter's own memory, no host read
        return out


class PointNet(torch.nn.Module):
    def __init__(self, emb_dims=224, input_shape="bnc", use_bn=False, global_feat=True):
        # emb_dims: width of the last attention layer; input_shape: "bnc" [B,N,3] or "bcn" [B,3,N]
        super(PointNet, self).__init__()
        if input_shape not in ["bcn", "bnc"]:
            raise ValueError("Allowed shapes are 'bcn' (batch * channels * num_in_points), 'bnc' ")
        self.input_shape = input_shape
        self.emb_dims = emb_dims
        self.use_bn = use_bn
        self.global_feat = global_feat
        if not self.global_feat:
            self.pooling = Pooling('max')

        self.conv1 = Self_Attn(3, 32)
        self.conv2 = Self_Attn(32, 64)
        self.conv3 = Self_Attn(64, 64)
        self.conv4 = Self_Attn(64, 128)
        self.conv5 = Self_Attn(128, self.emb_dims)

    def forward(self, input_data):
        # input_data in input_shape -> per-point features [B, 288 + emb_dims, N] (global_feat=False: the pooled vector repeated in front)
        channel_last = self.input_shape == "bnc"
        num_points = input_data.shape[1 if channel_last else 2]
        if input_data.shape[2 if channel_last else 1] != 3:
            raise RuntimeError("shape of x must be of [Batch x 3 x NumInPoints]")

        if _fusable(self, input_data):
            with on_device_of(input_data):
                x1 = self.conv1.fused(f32c(input_data), channel_last)
                x2 = self.conv2.fused(x1)
                x3 = self.conv3.fused(x2)
                x4 = self.conv4.fused(x3 + x2)
                x5 = self.conv5.fused(x4)
        else:
            x = input_data.permute(0, 2, 1) if channel_last else input_data
            x1 = self.conv1(x)
            x2 = self.conv2(x1)
            x3 = self.conv3(x2)
            x4 = self.conv4(x3 + x2)
            x5 = self.conv5(x4)

        output = torch.cat([x1, x2, x3, x4, x5], dim=1)
        if self.global_feat:
            return output
        point_feature = output
        output = self.pooling(output)
        output = output.view(-1, self.emb_dims, 1).repeat(1, 1, num_points)
        return torch.cat([output, point_feature], 1)


class self_attention_fc(nn.Module):
    """two feature vectors per cloud through ONE query_conv, then each plus beta times its mix under the softmax of their outer product"""

    def __init__(self, in_dim, out_dim):
        super(self_attention_fc, self).__init__()
        self.in_dim = in_dim
        self.out_dim = out_dim
        self.query_conv = BasicConv1D(in_dim, out_dim)
        self.beta = nn.Parameter(torch.zeros(1))
        self.softmax = nn.Softmax(dim=-1)

    def forward(self, x, y):
        """x, y [B,in_dim,1] -> two [B,out_dim,1]: each projected vector plus beta times its mix under the softmax of the outer product"""
        proj_query_x = self.query_conv(x)                       # [B,C,1]
        proj_key_y = self.query_conv(y).permute(0, 2, 1)        # [B,1,C]
        energy_xy = torch.bmm(proj_query_x, proj_key_y)         # [B,C,C]
        attention_xy = self.softmax(energy_xy)
        attention_yx = self.softmax(energy_xy.permute(0, 2, 1))
        proj_value_x = proj_query_x
        proj_value_y = proj_key_y.permute(0, 2, 1)
        out_x = torch.bmm(attention_xy, proj_value_x)
        out_x = self.beta * out_x + proj_value_x
        out_y = torch.bmm(attention_yx, proj_value_y)
        out_y = self.beta * out_y + proj_value_y
        return out_x, out_y

    def fused(self, rows, swap=False):
        """rows [2B,in_dim]: the x vectors, then the y vectors -> [2B,out_dim]: out_x then out_y (swap: out_y then out_x)"""
        if self.query_conv.active != True:      # noqa: E712
            raise RuntimeError("self_attention_fc's fused route takes a query_conv with its Mish")
        B = rows.shape[0] // 2
        w, b = self.query_conv.folded_rows()
        p = mish_(_fused.rows_affine(rows, w, b).contiguous())
        C = p.shape[1]
        out = torch.empty_like(p)
        ox, oy = (out[B:], out[:B]) if swap else (out[:B], out[B:])
        call("l3d_outer_softmax_mix", p[:B], p[B:], self.beta.detach(), B, C, ox, oy)
        return out


class PointNetMask(nn.Module):
    def __init__(self, template_feature_size=1024, source_feature_size=1024, feature_model=None):
        super().__init__()
        self.feature_model = feature_model if feature_model is not None else PointNet()
        self.pooling_max = Pooling(pool_type='max')
        self.pooling_avg = Pooling(pool_type='avg')

        self.global_feat_1 = self_attention_fc(1024, 512)
        self.global_feat_2 = self_attention_fc(512, 256)
        self.global_feat_3 = self_attention_fc(256, 512)

        self.h3 = nn.Sequential(BasicConv1D(1024, 512),
                                BasicConv1D(512, 256),
                                BasicConv1D(256, 128),
                                nn.Conv1d(128, 1, 1), nn.Sigmoid())

    def find_mask(self, source_features, template_features):
        global_source_features = torch.cat([self.pooling_max(source_features), self.pooling_avg(source_features)], dim=1)
        global_template_features = torch.cat([self.pooling_max(template_features), self.pooling_avg(template_features)], dim=1)

        shared_feat_1, shared_feat_2 = self.global_feat_1(global_source_features.unsqueeze(2), global_template_features.unsqueeze(2))
        shared_feat_1, shared_feat_2 = self.global_feat_2(shared_feat_1, shared_feat_2)
        shared_feat_1, shared_feat_2 = self.global_feat_3(shared_feat_1, shared_feat_2)

        batch_size = template_features.shape[0]
        x = torch.cat([template_features, shared_feat_1.repeat(1, 1, template_features.shape[2])], dim=1)
        x = self.h3(x)
        y = torch.cat([source_features, shared_feat_2.repeat(1, 1, source_features.shape[2])], dim=1)
        y = self.h3(y)
        return x.view(batch_size, -1), y.view(batch_size, -1)

    def fusable(self, *tensors):
        return _fusable(self, *tensors)

    def forward(self, template, source):
        if self.fusable(template, source):
            with on_device_of(template, source):
                return self._forward_fused(template, source)
        source_features = self.feature_model(source)                # [B x C x N]
        template_features = self.feature_model(template)            # [B x C x N]
        return self.find_mask(source_features, template_features)

    def _head_fused(self, feats, g):
        """h3 over feats [R,Ct,N] with the other cloud's global feature g [R,Cg] as a per-cloud shift of h3[0] -> masks [R,N]"""
        h0, h1, h2, last = self.h3[0], self.h3[1], self.h3[2], self.h3[3]
        R, Ct, N = feats.shape
        w0 = h0.conv.weight
        if Ct + g.shape[1] != w0.shape[1]:
            raise RuntimeError(f"h3 takes {w0.shape[1]} channels, the feature model gives {Ct} + {g.shape[1]}")
        wt, wg, scale, shift = _fused.conv_column_blocks(h0.conv, h0.bn, Ct, scale_block=1)      # wg carries the BN scale
        x = _fused.pointwise_conv(feats, wt, scale, _fused.rows_affine(g, wg, shift), relu=False)
        if h0.active == True:      # noqa: E712
            mish_(x)
        x = h2.fused(h1.fused(x))
        return torch.sigmoid(F.conv1d(x, last.weight, last.bias)).view(R, N)

    def _forward_fused(self, template, source):
        fm = self.feature_model
        B = template.shape[0]
        stacked = template.shape == source.shape
        if stacked:
            both = f32c(fm(torch.cat([source, template], dim=0)))          # [2B,Ct,N]: the source's rows, then the template's
            rows = torch.cat([both.amax(dim=2), both.mean(dim=2)], dim=1)  # [2B,2Ct]
        else:
            sf, tf = f32c(fm(source)), f32c(fm(template))
            rows = torch.cat([torch.cat([f.amax(dim=2), f.mean(dim=2)], dim=1) for f in (sf, tf)], dim=0)
        rows = self.global_feat_1.fused(rows)
        rows = self.global_feat_2.fused(rows)
        rows = self.global_feat_3.fused(rows, swap=True)                   # the template's vector first: it goes with the source's points
        if stacked:
            masks = self._head_fused(both, rows)
            return masks[B:], masks[:B]
        return self._head_fused(tf, rows[B:]), self._head_fused(sf, rows[:B])


class MaskNet2(nn.Module):
    def __init__(self, feature_model=None, is_training=True):
        super().__init__()
        self.maskNet = PointNetMask(feature_model=feature_model if feature_model is not None else PointNet(use_bn=True))
        self.is_training = is_training

    index_points = staticmethod(MaskNet.index_points)      # points [B,N,C], idx [B,S] -> [B,S,C]: the same helper as MaskNet's

    def forward(self, template, source, point_selection='threshold', mask_threshold=0.5):
        if template.shape[0] != 1 or source.shape[0] != 1:
            raise ValueError("MaskNet2.forward selects mask > threshold of a single pair (B == 1); use maskNet(template, source) for the masks of a batch")
        fused = self.maskNet.fusable(template, source)
        template_mask, source_mask = self.maskNet(template, source)   # B, N

        picked = []
        for mask, cloud in ((template_mask, template), (source_mask, source)):
            got = None
            if fused:
                with on_device_of(cloud):
                    got = mask_select(mask.contiguous(), cloud, 0, mask_threshold)
            if got is None:
                idx = torch.nonzero(mask[0] > mask_threshold).view(1, -1)
                got = idx, cloud[:, idx[0], 0:3]
            picked.append(got)
        (self.template_idx, masked_template), (self.source_idx, masked_source) = picked
        return masked_template, masked_source, template_mask, source_mask
