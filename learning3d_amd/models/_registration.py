"""Host side of registration.hip for the iterative registration models (pointnetlk.py, pcrnet.py): the PointNet pass whose first
layer poses its cloud on the fly, and thin wrappers of the loop kernels.  Everything here only launches on the current stream:
no host read, no allocation whose size depends on data, so a loop built from these calls can be captured in one graph."""
import torch

from .._lib import call, f32c, require_gpu
from . import _fused
from .pointnet import PointNet


def usable(model, feature_model, pooling, *tensors):
    """May the fused loop run: device fp32 [B,N,3] clouds, the package's PointNet ('bnc', global feature, five folded layers)
    under a max pool, BatchNorm on running statistics, nothing to differentiate."""
    if not all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.shape[2] == 3 for t in tensors):
        return False
    if type(feature_model) is not PointNet or not feature_model.global_feat or feature_model.input_shape != "bnc":
        return False
    if pooling.pool_type != 'max' or feature_model.conv1.weight.dtype != torch.float32:
        return False
    return _fused.can_fuse(model, *tensors)


def identity(B, device):
    return torch.eye(4, dtype=torch.float32, device=device).repeat(B, 1, 1)


def posed_features(feature_model, cloud, T=None, dt=None, want_features=True, want_cloud=False):
    """cloud [B,N,3] under transforms T [B,Tn,4,4] (or the 6 finite-difference transforms of dt [6]) -> (pooled PointNet features
    [B Tn, emb] or None, posed clouds [B Tn, N, 3] or None).  Layer 1 is l3d_reg_pose_first_layer; layers 2-4 and conv5 + max run
    on the fp32 matrix cores (mlp.hip) -- not the bf16x3 or f16x2 kernels: the Jacobian divides feature differences by dt."""
    B, N, _ = cloud.shape
    Tn = 6 if dt is not None else T.shape[1]
    stack = [_fused.fold_conv_bn(c, b) for c, b in feature_model._stack()]
    w1, sc1, sh1 = stack[0]
    C1 = w1.shape[0]
    y = torch.empty((B * Tn, C1, N), dtype=torch.float32, device=cloud.device) if want_features else None
    posed = torch.empty((B * Tn, N, 3), dtype=torch.float32, device=cloud.device) if want_cloud else None
    call("l3d_reg_pose_first_layer", cloud, T, dt, B, Tn, N, w1, sc1, sh1, C1, 1, y, posed)
    if not want_features:
        return None, posed
    x = y
    for w, sc, sh in stack[1:-1]:
        x = _fused.pointwise_conv(x, w, sc, sh, relu=True, split=False)
    w, sc, sh = stack[-1]
    if N % 64 == 0:
        part = torch.empty((B * Tn, w.shape[0], N // 64), dtype=torch.float32, device=cloud.device)
        call("l3d_pointwise_conv", x, 0, w, sc, sh, 0, B * Tn, w.shape[1], w.shape[0], N, 1, 64, part, tag="[maxpool]")
        return part.max(dim=2)[0], posed
    return _fused.pointwise_conv(x, w, sc, sh, relu=True, split=False).max(dim=2)[0], posed


def jac_pinv(f0, f, dt, singular):
    """f0 [B,K], f [B 6,K], dt [6], singular int32 [1 + B] (zeroed) -> pinv [B,6,K]"""
    B, K = f0.shape
    pinv = torch.empty((B, 6, K), dtype=torch.float32, device=f0.device)
    call("l3d_reg_jac_pinv", f0, f, dt, B, K, pinv, singular)
    return pinv


def iclk_step(f, f0, pinv, step, maxiter, xtol, singular, ws, state, est_T, series, r):
    B, K = f0.shape
    call("l3d_reg_iclk_step", f, f0, pinv, B, K, step, maxiter, float(xtol), singular, ws, state, est_T, series, r)


def quat_update(pose7, first, est_R, est_t, est_T):
    call("l3d_reg_quat_update", pose7, pose7.shape[0], int(first), est_R, est_t, est_T)


def prepare(*clouds):
    require_gpu(*clouds)
    return [f32c(c) for c in clouds]
