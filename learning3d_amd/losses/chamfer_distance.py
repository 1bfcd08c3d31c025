"""Drop-in for learning3d/losses/chamfer_distance.py + losses/cuda/chamfer_distance/ on MI355X.

reference: losses/chamfer_distance.py:34-51 (chamfer_distance / ChamferDistanceLoss) and
losses/cuda/chamfer_distance/chamfer_distance.py:14-66 (ChamferDistanceFunction / ChamferDistance).
The reference JIT-compiles a CUDA extension on first use and silently falls back to an O(B*N*M*3)
torch broadcast when that fails (:36-42); here the native path is the only path.
"""
import torch
import torch.nn as nn

from .._lib import call, f32c, lib, require_gpu


class ChamferDistanceFunction(torch.autograd.Function):
    """dist1 [B,N], dist2 [B,M] squared NN distances; backward == cd.backward_cuda (deterministic)."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        batchsize, n, _ = xyz1.size()
        _, m, _ = xyz2.size()
        xyz1 = f32c(xyz1)
        xyz2 = f32c(xyz2)
        dev = xyz1.device
        dist1 = torch.empty(batchsize, n, dtype=torch.float32, device=dev)
        dist2 = torch.empty(batchsize, m, dtype=torch.float32, device=dev)
        idx1 = torch.empty(batchsize, n, dtype=torch.int32, device=dev)
        idx2 = torch.empty(batchsize, m, dtype=torch.int32, device=dev)
        call("l3d_chamfer_forward", xyz1, xyz2, batchsize, n, m, dist1, dist2, idx1, idx2)
        ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
        return dist1, dist2

    @staticmethod
    def backward(ctx, graddist1, graddist2):
        xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
        graddist1 = f32c(graddist1)
        graddist2 = f32c(graddist2)
        b, n, _ = xyz1.shape
        m = xyz2.shape[1]
        gradxyz1 = torch.empty_like(xyz1)
        gradxyz2 = torch.empty_like(xyz2)
        call("l3d_chamfer_backward", xyz1, xyz2, b, n, m, graddist1, graddist2, idx1, idx2, gradxyz1, gradxyz2)
        return gradxyz1, gradxyz2


class ChamferDistance(torch.nn.Module):
    def forward(self, xyz1, xyz2):
        return ChamferDistanceFunction.apply(xyz1, xyz2)


def chamfer_partials(dist1, dist2):
    """Device fp64 tensor [4] = (sum sqrt(dist1), sum sqrt(dist2), #dist1, #dist2): the per-shard
    partial sums the multi-GPU path all-gathers (forward-only helper; no autograd, no host sync)."""
    dist1, dist2 = f32c(dist1), f32c(dist2)                  # the kernels read dense fp32 with 16-byte loads
    B, N = dist1.shape
    M = dist2.shape[1]
    part = torch.empty(4, dtype=torch.float64, device=dist1.device)
    call("l3d_chamfer_partials", dist1, dist2, B, N, M, part)
    return part


_LL_WS = {}


def chamfer_loss_local(dist1, dist2):
    """One rank, one launch: the same partial sums and the same combine as chamfer_combine(chamfer_partials(...)),
    spread over up to 64 workgroups (l3d_chamfer_loss_local_mb; workspace cached per device and stream)."""
    require_gpu(dist1, dist2)
    dist1, dist2 = f32c(dist1), f32c(dist2)
    B, N = dist1.shape
    M = dist2.shape[1]
    key = (dist1.device.index, torch.cuda.current_stream(dist1.device).cuda_stream)
    from .. import _lib
    hit = _LL_WS.get(key)
    if hit is None or hit[1] != _lib.FAILED_CALLS:
        # the kernel's last block re-arms the workspace's ticket; after ANY failed C-ABI call (a launch that may have aborted
        # before doing so) the workspace is zeroed again instead of trusting it
        ws = hit[0].zero_() if hit is not None else torch.zeros(lib().l3d_chamfer_loss_local_ws_bytes(), dtype=torch.uint8, device=dist1.device)
        _LL_WS[key] = (ws, _lib.FAILED_CALLS)
    ws = _LL_WS[key][0]
    part = torch.empty(4, dtype=torch.float64, device=dist1.device)
    loss = torch.empty((), dtype=torch.float32, device=dist1.device)
    call("l3d_chamfer_loss_local_mb", dist1, dist2, B, N, M, ws, part, loss)
    return loss


_FL_WS = {}


def chamfer_forward_loss(template, source, want="loss"):
    """The no-grad forward of ChamferDistanceLoss as ONE launch (l3d_chamfer_forward_loss): NN search of both directions and the loss
    tail.  Returns the fp32 loss scalar (want="loss"), this rank's fp64 partial sums [4] (want="partials": what a multi-GPU run
    all-gathers, == chamfer_partials(dist1, dist2)), or (loss, partials, dist1, dist2, idx1, idx2) (want="all")."""
    require_gpu(template, source)
    xyz1, xyz2 = f32c(template), f32c(source)
    B, N, _ = xyz1.shape
    M = xyz2.shape[1]
    dev = xyz1.device
    from .. import _lib
    nbytes = lib().l3d_chamfer_forward_loss_ws_bytes(B, N, M)
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    hit = _FL_WS.get(key)
    if hit is None or hit[1] != _lib.FAILED_CALLS or hit[0].numel() < nbytes:
        # the kernel's last workgroup re-arms the ticket; after ANY failed C-ABI call the workspace is zeroed again instead of trusted
        ws = hit[0].zero_() if hit is not None and hit[0].numel() >= nbytes else torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        _FL_WS[key] = (ws, _lib.FAILED_CALLS)
    ws = _FL_WS[key][0]
    dist1 = torch.empty(B, N, dtype=torch.float32, device=dev)
    dist2 = torch.empty(B, M, dtype=torch.float32, device=dev)
    idx1 = torch.empty(B, N, dtype=torch.int32, device=dev)
    idx2 = torch.empty(B, M, dtype=torch.int32, device=dev)
    part = torch.empty(4, dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    call("l3d_chamfer_forward_loss", xyz1, xyz2, B, N, M, dist1, dist2, idx1, idx2, ws, part, loss)
    if want == "loss":
        return loss
    if want == "partials":
        return part
    return loss, part, dist1, dist2, idx1, idx2


def chamfer_combine(partials):
    """partials: fp64 [world,4] (or [4]) device tensor -> fp32 scalar loss tensor (on device)."""
    require_gpu(partials)
    if partials.dtype != torch.float64:
        raise TypeError("chamfer_combine expects the fp64 partial sums of chamfer_partials")
    partials = partials.contiguous().view(-1, 4)
    loss = torch.empty((), dtype=torch.float32, device=partials.device)
    call("l3d_chamfer_combine", partials, partials.shape[0], loss)
    return loss


def chamfer_distance(template: torch.Tensor, source: torch.Tensor):
    """reference: losses/chamfer_distance.py:34-43 -- (mean sqrt d1 + mean sqrt d2) / 2, one scalar
    over the whole batch."""
    from .._lib import on_device_of
    with on_device_of(template, source):               # tensors on a GPU other than the current one: switch for the call
        if torch.is_grad_enabled() and (template.requires_grad or source.requires_grad):
            cost_p0_p1, cost_p1_p0 = ChamferDistance()(template, source)
            cost_p0_p1 = torch.mean(torch.sqrt(cost_p0_p1))
            cost_p1_p0 = torch.mean(torch.sqrt(cost_p1_p0))
            return (cost_p0_p1 + cost_p1_p0) / 2.0
        return chamfer_forward_loss(template, source)           # search + loss tail, one launch (two for the large-cloud kernels)


def chamfer(a, b):
    """reference: losses/chamfer_distance.py:21-31 (the torch fallback): same value, native path."""
    return chamfer_distance(a, b)


class ChamferDistanceLoss(nn.Module):
    def __init__(self):
        super(ChamferDistanceLoss, self).__init__()

    def forward(self, template, source):
        return chamfer_distance(template, source)
