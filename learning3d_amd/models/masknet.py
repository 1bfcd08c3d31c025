"""Drop-in for learning3d/models/masknet.py on MI355X: MaskNet, the front end that picks the points of a full template which
belong to a partial source (reference: models/masknet.py:7-77; examples/test_masknet.py hands its masked template to the
registration networks).  Same constructor arguments, attribute names and state_dict keys as the reference
(maskNet.feature_model.*, maskNet.h3.{0,2,4,6,8}.*), so its checkpoints load with strict=True.

One deliberate difference: each instance gets a fresh PointNet when no feature model is passed.  The reference's default argument
(`feature_model=PointNet(use_bn=True)`) is evaluated once, so all its default-constructed instances share ONE module, an accident
of the default-argument rule; the keys are the same either way.

With device fp32 clouds, BatchNorm on running statistics and nothing to differentiate (_fused.can_fuse), the forward is
  * the source's pooled feature without its conv5 map (PointNet.forward_pooled),
  * h3[0] over the template's features alone: the source half of its input is the same vector for every point of a cloud, so
    W0 [t ; g] + b0 = W0[:, :Ct] t + (W0[:, Ct:] g + b0), a per-cloud shift from l3d_linear_rows -- half of the reference's largest
    GEMM and its [B,2048,N] concatenation are gone,
  * h3[2], h3[4] on the conv kernels (the f16x2 chain through plane images where its tiles fit, else the fp32-level kernels),
  * h3[6..9] as one l3d_mask_tail launch (the [B,128,N] map is never written),
  * the selection and the gather as one l3d_mask_select launch.
Anything else (CPU tensors, autograd, train-mode BatchNorm) takes the reference's op sequence in torch.

Order of the selected points: the reference's torch.topk(sorted=False) leaves it unspecified (it differs between CPU and GPU).
Here mask_idx is ascending on every route; on the fused route ties at the k-th value go to the lowest index (l3d_masknet.h)."""
import torch
import torch.nn as nn

from .._lib import call, f32c, on_device_of
from . import _fused
from .pointnet import PointNet
from .pooling import Pooling

FUSED = True                 # False: the op sequence for every input (A/B: tools/masknet_bench.py)
MASK_SELECT_MAX_N = 16384    # l3d_mask_select: a cloud's keys live in one workgroup's LDS


def mask_select(mask, points, k=0, threshold=0.5):
    """l3d_mask_select: mask [B,N], points [B,N,3] -> (idx int64, points[idx]) with idx ascending per cloud.  k > 0: the k largest
    mask values of every cloud ([B,k]; ties to the lowest index, NaN above every number); k == 0 (B == 1): mask > threshold
    ([1,count]: one host read of the count, the output's shape depends on the data).  None when the kernel does not take the shape."""
    B, N = mask.shape
    if N > MASK_SELECT_MAX_N or points.dim() != 3 or points.shape[2] != 3 or (k == 0 and B != 1):
        return None
    mask, points = f32c(mask), f32c(points)
    rows = k if k > 0 else N
    idx = torch.empty((B, rows), dtype=torch.int64, device=mask.device)
    out = torch.empty((B, rows, 3), dtype=torch.float32, device=mask.device)
    count = torch.empty(B, dtype=torch.int32, device=mask.device)
    call("l3d_mask_select", mask, points, B, N, int(k), float(threshold), idx, out, count)
    if k == 0:
        c = int(count[0])
        idx, out = idx[:, :c], out[:, :c]
    return idx, out


class PointNetMask(nn.Module):
    def __init__(self, template_feature_size=1024, source_feature_size=1024, feature_model=None):
        super().__init__()
        self.feature_model = feature_model if feature_model is not None else PointNet()
        self.pooling = Pooling()

        input_size = template_feature_size + source_feature_size
        self.h3 = nn.Sequential(nn.Conv1d(input_size, 1024, 1), nn.ReLU(),
                                nn.Conv1d(1024, 512, 1), nn.ReLU(),
                                nn.Conv1d(512, 256, 1), nn.ReLU(),
                                nn.Conv1d(256, 128, 1), nn.ReLU(),
                                nn.Conv1d(128, 1, 1), nn.Sigmoid())

    def find_mask(self, x, t_out_h1):
        batch_size, _, num_points = t_out_h1.size()
        x = x.unsqueeze(2)
        x = x.repeat(1, 1, num_points)
        x = torch.cat([t_out_h1, x], dim=1)
        x = self.h3(x)
        return x.view(batch_size, -1)

    def fusable(self, *tensors):
        """device fp32 tensors, BatchNorm on running statistics, nothing to differentiate"""
        return FUSED and _fused.fusable(self, *tensors)

    def forward(self, template, source):
        if self.fusable(template, source):
            with on_device_of(template, source):
                return _fused.run_guarded(template.device, lambda: self._forward_fused(template, source))
        source_features = self.feature_model(source)                # [B x C x N]
        template_features = self.feature_model(template)            # [B x C x N]
        source_features = self.pooling(source_features)
        return self.find_mask(source_features, template_features)

    def _forward_fused(self, template, source):
        fm = self.feature_model
        g = fm.forward_pooled(source) if hasattr(fm, "forward_pooled") else None
        if g is None:
            g = self.pooling(fm(source))
        tf = f32c(fm(template))                                        # [B,Ct,N]
        B, Ct, N = tf.shape
        conv0, conv2, conv4, conv6, conv8 = (self.h3[i] for i in (0, 2, 4, 6, 8))
        w0 = conv0.weight
        C0 = w0.shape[0]
        if g.shape[1] + Ct != w0.shape[1]:
            raise RuntimeError(f"h3 takes {w0.shape[1]} channels, the feature model gives {Ct} + {g.shape[1]}")
        wt, wg, _, b0 = _fused.conv_column_blocks(conv0, None, Ct)
        # the source half of h3[0], the same for every point of a cloud: a per-cloud shift [B,C0]
        shift = _fused.rows_affine(g, wg, b0)
        w2, _, b2 = _fused.fold_conv_bn(conv2)
        w4, _, b4 = _fused.fold_conv_bn(conv4)
        C2, C4 = w2.shape[0], w4.shape[0]
        if (_fused.gemm_arith() == "f16x2" and _fused.SPLIT_BF16
                and all(_fused.f16_eligible(ci, co, N) for ci, co in ((Ct, C0), (C0, C2), (C2, C4)))):
            store = self.__dict__.setdefault("_l3d_images", {})

            # keyed by the parameters themselves (a derived tensor's address can come back after a rebuild)
            def image(name, src, w):
                return _fused.cached(store, name, [src], lambda: _fused.split_weights_f16(w), extra=(Ct,))
            img = _fused.split_rows_f16(tf, channel_first=True)
            img, _ = _fused.pointwise_conv_f16_pool(img, B, N, image("h3.0.f16", w0, wt), Ct, C0, None, shift, relu=True,
                                                    out_planes=True, pool=False)
            img, _ = _fused.pointwise_conv_f16_pool(img, B, N, image("h3.2.f16", conv2.weight, w2), C0, C2, None, b2, relu=True,
                                                    out_planes=True, pool=False)
            x = _fused.pointwise_conv_f16(img, B, N, image("h3.4.f16", conv4.weight, w4), C2, C4, None, b4, relu=True)
        else:
            x = _fused.pointwise_conv(tf, wt, None, shift, relu=True)
            x = _fused.pointwise_conv(x, w2, None, b2, relu=True)
            x = _fused.pointwise_conv(x, w4, None, b4, relu=True)
        w6, _, b6 = _fused.fold_conv_bn(conv6)
        w8, _, b8 = _fused.fold_conv_bn(conv8)
        H = w6.shape[0]
        if w8.shape[0] != 1 or b6 is None or b8 is None:
            raise RuntimeError("l3d_mask_tail takes a head that ends in Conv1d(H, 1) with biases")
        mask = torch.empty((B, N), dtype=torch.float32, device=x.device)
        call("l3d_mask_tail", x, w6, b6, w8.reshape(-1), b8, B, C4, H, N, mask)
        return mask


class MaskNet(nn.Module):
    def __init__(self, feature_model=None, is_training=True):
        super().__init__()
        self.maskNet = PointNetMask(feature_model=feature_model if feature_model is not None else PointNet(use_bn=True))
        self.is_training = is_training

    @staticmethod
    def index_points(points, idx):
        """
        Input:
            points: input points data, [B, N, C]
            idx: sample index data, [B, S]
        Return:
            new_points:, indexed points data, [B, S, C]
        """
        device = points.device
        B = points.shape[0]
        view_shape = list(idx.shape)
        view_shape[1:] = [1] * (len(view_shape) - 1)
        repeat_shape = list(idx.shape)
        repeat_shape[0] = 1
        batch_indices = torch.arange(B, dtype=torch.long).to(device).view(view_shape).repeat(repeat_shape)
        new_points = points[batch_indices, idx, :]
        return new_points

    # This function is only useful for testing with a single pair of point clouds.
    @staticmethod
    def find_index(mask_val):
        mask_idx = torch.nonzero((mask_val[0] > 0.5) * 1.0)
        return mask_idx.view(1, -1)

    def forward(self, template, source, point_selection='threshold'):
        topk = point_selection == 'topk' or self.is_training
        if not topk and point_selection != 'threshold':
            raise ValueError("point_selection is 'topk' or 'threshold'")
        fused = self.maskNet.fusable(template, source)
        mask = self.maskNet(template, source)

        if fused:
            with on_device_of(template):
                picked = mask_select(mask, template, source.shape[1] if topk else 0, 0.5)
            if picked is not None:
                self.mask_idx, template = picked
                return template, mask
        if topk:
            _, self.mask_idx = torch.topk(mask, source.shape[1], dim=1, sorted=False)
            self.mask_idx = torch.sort(self.mask_idx, dim=1)[0]       # the documented order, on every route
        else:
            self.mask_idx = self.find_index(mask)

        template = self.index_points(template, self.mask_idx)
        return template, mask
