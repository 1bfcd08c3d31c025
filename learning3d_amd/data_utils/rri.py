"""RRI features of DeepGMR's input (reference: data_utils/dataloaders.py:121-147, knn_idx / get_rri): per point and neighbour the
four rotation-invariant numbers (|p|, |q|, the angle between p and q, the smallest positive angle from q's tangent component to
another neighbour's, about p).

rri_features(points [B,N,3], k) on a device fp32 tensor is two launches: l3d_knn_graph with k + 1 neighbours, whose first column --
the point itself -- is dropped as the reference drops it from cKDTree.query(k + 1), and l3d_rri_features.  On CPU tensors, and on
device tensors of another dtype (fp64: neighbours and features both in fp64), it is the reference's arithmetic restated for a
batch in torch, with the [N,k,k,3] cross-product tensor replaced by the scalar triple product written out over [B,N,k,k].  get_rri(pts, k) is the reference's numpy signature on top of it.

Differences from the reference: the neighbours come from the exact squared distances (CPU) or the kNN kernel's ranking (device)
instead of a k-d tree, so they can differ where two distances tie within rounding; the device kernel forms the geometry in fp64 and
rounds once, so it is closer to get_rri in fp64 than get_rri in fp32 is."""
import math

import numpy as np
import torch

from .._lib import call, f32c, on_device_of


def knn_idx(points, k):
    """points [B,N,3] -> int64 [B,N,k]: the k nearest other points, nearest first (the reference's cKDTree.query(k + 1)[:, 1:])"""
    B, N, _ = points.shape
    if k + 1 > N:
        raise ValueError(f"rri features with k = {k} need at least {k + 1} points, got {N}")
    if points.is_cuda and points.dtype == torch.float32:           # other dtypes are ranked in their own precision, below
        x = f32c(points)
        idx = torch.empty((B, N, k + 1), dtype=torch.int64, device=x.device)
        with on_device_of(x):
            call("l3d_knn_graph", x, B, N, k + 1, idx)
        return idx[:, :, 1:].contiguous()
    d = ((points[:, :, None, :] - points[:, None, :, :]) ** 2).sum(-1)
    return torch.topk(d, k + 1, dim=2, largest=False, sorted=True)[1][:, :, 1:].contiguous()


def rri_geometry(points, idx):
    """get_rri's intermediate quantities (:129-142) for a batch in torch: -> rp, rq, theta [B,N,k,1] and psi [B,N,k,k], psi[.., a, b]
    the angle from T_a to T_b about p, in [0, 2 pi)"""
    B, N, _ = points.shape
    k = idx.shape[2]
    q = torch.gather(points[:, None].expand(B, N, N, 3), 2, idx[..., None].expand(B, N, k, 3))      # [B,N,k,3]
    p = points[:, :, None, :].expand(B, N, k, 3)
    rp = torch.linalg.norm(p, dim=-1, keepdim=True)
    rq = torch.linalg.norm(q, dim=-1, keepdim=True)
    pn, qn = p / rp, q / rq
    dot = (pn * qn).sum(-1, keepdim=True)
    theta = torch.acos(dot.clamp(-1, 1))
    T = q - dot * p
    Ta, Tb = T[:, :, :, None, :], T[:, :, None, :, :]                     # psi[.., a, b] from (T_b x T_a) . pn and T_b . T_a
    n = pn[:, :, :1, None, :]
    sin_psi = ((Tb[..., 1] * Ta[..., 2] - Tb[..., 2] * Ta[..., 1]) * n[..., 0]
               + (Tb[..., 2] * Ta[..., 0] - Tb[..., 0] * Ta[..., 2]) * n[..., 1]
               + (Tb[..., 0] * Ta[..., 1] - Tb[..., 1] * Ta[..., 0]) * n[..., 2])
    cos_psi = (Tb * Ta).sum(-1)
    return rp, rq, theta, torch.remainder(torch.atan2(sin_psi, cos_psi), 2 * math.pi)


def rri_from_idx(points, idx, channel_first=False):
    """points [B,N,3] (used as given), idx int64 [B,N,k] -> [B,N,4k] (or [B,4k,N]): l3d_rri_features on a device fp32 tensor, the
    torch restatement of get_rri (:129-147) otherwise"""
    B, N, _ = points.shape
    k = idx.shape[2]
    if points.is_cuda and points.dtype == torch.float32:
        x = f32c(points)
        feat = torch.empty((B, 4 * k, N) if channel_first else (B, N, 4 * k), dtype=torch.float32, device=x.device)
        with on_device_of(x):
            call("l3d_rri_features", x, idx.contiguous(), B, N, k, int(channel_first), feat)
        return feat
    rp, rq, theta, psi = rri_geometry(points, idx)
    phi = torch.kthvalue(psi, 2, dim=-1, keepdim=True)[0]                 # the second smallest over b, self (psi = 0) included
    feat = torch.cat([rp, rq, theta, phi], dim=-1).reshape(B, N, 4 * k)
    return feat.transpose(1, 2).contiguous() if channel_first else feat


def rri_features(points, k, center=True, channel_first=False):
    """points [B,N,3] -> RRI features [B,N,4k], neighbour-major (rp, rq, theta, phi); channel_first: [B,4k,N], what DeepGMR's first
    conv reads.  center: subtract each cloud's centroid first (the reference's dataset does, data_utils/dataloaders.py:316-317)."""
    if points.dim() != 3 or points.shape[2] != 3:
        raise ValueError("rri_features expects points of shape [B, N, 3]")
    with torch.no_grad():
        x = points - points.mean(dim=1, keepdim=True) if center else points
        return rri_from_idx(x, knn_idx(x, k), channel_first)


def get_rri(pts, k):
    """the reference's signature: pts numpy [N,3] (used as given) -> numpy [N,4k], in pts' dtype"""
    x = torch.from_numpy(np.ascontiguousarray(pts))[None]
    return rri_features(x, k, center=False)[0].numpy()
