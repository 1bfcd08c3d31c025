"""ms and peak memory of an RPMNet training step (1024 points with normals in both clouds, 64 neighbours) on PPFNet's differentiable HIP
route against the op sequence of the same build (_fused.TRAIN_HIP = False: torch convolutions, F.group_norm, ReLU and max under
autograd -- what every build before this route ran):

  features   forward + backward of the feature network alone on one cloud (a random cotangent)
  step       a whole step: RPMNet forward with 2 iterations, FrobeniusNormLoss(est_T, igt) plus the mean of perm_matrices' row sums as
             a stand-in for an inlier term, backward, Adam
  kernels    each streaming kernel of rpmnet_train.hip alone at the pre-pool shape [B,96 or 192,64 * points], with the bytes it has to
             move (from the shapes) over its time

The two sides of each pair run interleaved, round by round, so that clock and thermal drift hits both alike; medians over the
rounds.  Peak memory is torch.cuda.max_memory_allocated over one warm round of each side, above what was allocated before it.

    python tools/rpmnet_train_bench.py [--batch 8 32] [--points 1024] [--rounds 5]
Prints one JSON line per batch size."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learning3d_amd.losses import FrobeniusNormLoss                   # noqa: E402
from learning3d_amd.models import RPMNet, _fused, ppfnet               # noqa: E402


def timed(fn, hip, reps=1):
    _fused.TRAIN_HIP = hip
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    finally:
        _fused.TRAIN_HIP = True


def peak(fn, hip):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    timed(fn, hip)
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def kernel_rates(B, C, K, N, dev, rounds):
    """-> {kernel: (ms, GB/s)} at y [B,C,K N]: the bytes are the [B,C,P] tensors each kernel has to read and write"""
    P = K * N
    g = torch.Generator(device=dev).manual_seed(1)
    y = torch.randn((B, C, P), device=dev, generator=g)
    du = torch.randn((B, C, P), device=dev, generator=g)
    dpool = torch.randn((B, C, N), device=dev, generator=g)
    gamma = torch.rand((C,), device=dev, generator=g) * 2 - 0.7
    y64 = y.double()
    moments = torch.stack([y64.sum(2), (y64 * y64).sum(2)], -1).contiguous()
    del y64
    norm = torch.nn.GroupNorm(8, C).to(dev)
    with torch.no_grad():
        norm.weight.copy_(gamma)
    a, s = ppfnet.gn_affine(moments, norm, P)
    stat = ppfnet.gn_mean_rstd(moments, 8, P, norm.eps)
    widx = ppfnet.gn_pool_winner(y, a, K)
    part = torch.empty((B, C, 2), dtype=torch.float64, device=dev)
    m = torch.zeros((B, 8, 2), dtype=torch.float64, device=dev)
    ws = torch.empty(ppfnet._lib.lib().l3d_gn_backward_workspace_bytes(B, C, P) // 8, dtype=torch.float64, device=dev)
    out = torch.empty_like(y)
    tensor = B * C * P * 4
    call = ppfnet.call
    cases = {
        "gn_backward_stats": (2 * tensor, lambda: call("l3d_gn_backward_stats", du, None, 0, y, a, s, stat, B, C, 8, P, part, ws)),
        "gn_backward_stats_pooled": (2 * B * C * N * 4 + B * C * N, lambda: call("l3d_gn_backward_stats", dpool, widx, K, y, a, s, stat, B, C, 8,
                                                                                 P, part, ws)),
        "gn_backward_apply": (3 * tensor, lambda: call("l3d_gn_backward_apply", du, None, 0, y, a, s, stat, gamma, m, B, C, 8, P, out)),
        "gn_backward_apply_pooled": (2 * tensor, lambda: call("l3d_gn_backward_apply", dpool, widx, K, y, a, s, stat, gamma, m, B, C, 8, P, out)),
        "gn_pool_winner": (tensor, lambda: call("l3d_gn_pool_winner", y, a, B, C, K, N, widx)),
        "gn_relu": (2 * tensor, lambda: call("l3d_gn_relu", y, a, s, B, C, P, out)),
    }
    res = {}
    for name, (nbytes, fn) in cases.items():
        timed(fn, True)
        ms = statistics.median(timed(fn, True, 5) for _ in range(rounds))
        res[name] = {"ms": round(ms, 4), "GB_per_s": round(nbytes / ms / 1e6, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N = a.points
    for B in a.batch:
        torch.manual_seed(0)
        net = RPMNet().train().to(dev)
        fx = net.feat_extractor
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)
        xyz = torch.rand(B, N, 3, device=dev) * 2 - 1
        nrm = torch.nn.functional.normalize(torch.randn(B, N, 3, device=dev), dim=-1)
        ang = torch.tensor(0.5)
        R = torch.tensor([[ang.cos(), -ang.sin(), 0.0], [ang.sin(), ang.cos(), 0.0], [0.0, 0.0, 1.0]], device=dev)
        template = torch.cat([xyz, nrm], dim=-1)
        source = torch.cat([xyz @ R.t() + 0.1, nrm @ R.t()], dim=-1)
        igt = torch.eye(4, device=dev).repeat(B, 1, 1)
        igt[:, :3, :3], igt[:, :3, 3] = R, 0.1
        cot = torch.randn(B, N, fx.postpool[6].out_channels, device=dev)
        loss_fn = FrobeniusNormLoss()

        def features():
            net.zero_grad(set_to_none=True)
            (fx(xyz, nrm) * cot).sum().backward()

        def step():
            opt.zero_grad(set_to_none=True)
            res = net(template, source, 2)
            rows = torch.stack([pm.sum(2).mean() for pm in res["perm_matrices"]]).mean()
            (loss_fn(res["est_T"], igt) + rows).backward()
            opt.step()

        line = {"batch": B, "points": N, "neighbors": fx.n_sample, "rounds": a.rounds}
        for name, fn in (("features", features), ("step", step)):
            ms = {True: [], False: []}
            for hip in (True, False):
                timed(fn, hip)                            # warm-up: caches, lazy module loads, the allocator's blocks
            for _ in range(a.rounds):
                for hip in (True, False):
                    ms[hip].append(timed(fn, hip))
            line[name + "_ms_hip"] = round(statistics.median(ms[True]), 3)
            line[name + "_ms_op_sequence"] = round(statistics.median(ms[False]), 3)
            line[name + "_peak_mib_hip"] = round(peak(fn, True), 1)
            line[name + "_peak_mib_op_sequence"] = round(peak(fn, False), 1)
        if not a.no_kernels:
            del net, opt
            torch.cuda.empty_cache()
            line["kernels_c96"] = kernel_rates(B, 96, fx.n_sample, N, dev, a.rounds)
            line["kernels_c192"] = kernel_rates(B, 192, fx.n_sample, N, dev, a.rounds)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
