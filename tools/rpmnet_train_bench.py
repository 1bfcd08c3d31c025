"""ms and peak memory of an RPMNet training step (1024 points with normals in both clouds, 64 neighbours) on PPFNet's differentiable HIP
route against the op sequence of the same build (_fused.TRAIN_HIP = False: torch convolutions, F.group_norm, ReLU and max under
autograd -- what every build before this route ran):

  features   forward + backward of the feature network alone on one cloud (a random cotangent)
  step       a whole step: RPMNet forward with 2 iterations, FrobeniusNormLoss(est_T, igt) plus the mean of perm_matrices' row sums as
             a stand-in for an inlier term, backward, Adam
  kernels    each streaming kernel of rpmnet_train.hip alone at the pre-pool shape [B,96 or 192,64 * points], with the bytes it has to
             move (from the shapes) over its time
  matching   the matching stage (affinity, Sinkhorn, exp, row sums, weighted template) on RPMNet._Match against torch autograd of the
             same build (rpmnet.MATCH_HIP = False, PPFNet's HIP route on on both sides):
               matching_*        forward + backward of the stage alone at [B,points,points], the step's cotangents
               step_match_*      the whole step with MATCH_HIP on and off
               matching_kernels  l3d_sinkhorn_slack_keep and l3d_sinkhorn_slack_backward alone.  The backward is one entry point;
                                 its passes are told apart by n_iters: 0 is the first row pass and the output pass, and a further
                                 iteration adds one row and one column reduction and two exponentials per element of the output
                                 pass.  Bytes: log_alpha once per pass, the dense cotangent and dist where a pass reads them, d_out
               split             forward + backward of each other part of an iteration alone at the step's shapes:
                                 ParameterPredictionNet, the feature distance, the weighted Kabsch step
  param      ParameterPredictionNet's pre-pool stack on its HIP route against torch autograd of the same build (rpmnet.PARAM_HIP =
             False, every other route on on both sides), [median, min, max] over the rounds:
               param_net_*       forward + backward of the network alone at J = K = points
               step_param_*      the whole step with PARAM_HIP on and off

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
from learning3d_amd.models import RPMNet, _fused, ppfnet, rpmnet       # noqa: E402


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


def with_switch(fn, switch, on):
    """fn with rpmnet.<switch> = on"""
    def run():
        prev = getattr(rpmnet, switch)
        setattr(rpmnet, switch, on)
        try:
            fn()
        finally:
            setattr(rpmnet, switch, prev)
    return run


def pair(line, name, fn, rounds, switch="MATCH_HIP"):
    """ms (median, min, max) and peak of fn with the switch (MATCH_HIP, PARAM_HIP) on and off, interleaved round by round"""
    sides = {"hip": with_switch(fn, switch, True), "torch": with_switch(fn, switch, False)}
    ms = {k: [] for k in sides}
    for f in sides.values():
        timed(f, True)
    for _ in range(rounds):
        for k, f in sides.items():
            ms[k].append(timed(f, True))
    for k, f in sides.items():
        line[f"{name}_ms_{k}"] = [round(statistics.median(ms[k]), 3), round(min(ms[k]), 3), round(max(ms[k]), 3)]
        line[f"{name}_peak_mib_{k}"] = round(peak(f, True), 1)


def matching_kernels(B, N, dev, rounds, n_iters=5):
    """-> {case: (ms, GB/s)} of the two entry points alone at [B,N,N]"""
    g = torch.Generator(device=dev).manual_seed(2)
    dist = torch.rand((B, N, N), device=dev, generator=g) * 2
    beta, alpha = torch.rand(B, device=dev, generator=g) + 1, torch.rand(B, device=dev, generator=g) * 0.5 + 0.5
    x = torch.rand((B, N, 3), device=dev, generator=g)
    A = (-beta[:, None, None] * (dist - alpha[:, None, None])).contiguous()
    dp, dr, dw = torch.randn((B, N, N), device=dev, generator=g), torch.randn((B, N), device=dev, generator=g), torch.randn((B, N, 3), device=dev, generator=g)
    tensor = B * N * N * 4
    pots = {n: rpmnet.sinkhorn_slack_keep(A, n, x)[3] for n in (0, 1, n_iters)}

    def back(n):
        return lambda: rpmnet.sinkhorn_slack_backward(A, pots[n], x, 1e-5, d_perm=dp, d_rowsum=dr, d_weighted=dw, dist=dist, beta=beta,
                                                      alpha=alpha, want_beta=True, want_alpha=True)
    # passes over log_alpha: keep 2 n + 1 (+ perm written); backward 3 + 2 n - 1 for n >= 1, 2 for n = 0; d_perm in the row, column and
    # output pass, dist and d_out in the output pass
    cases = {"sinkhorn_slack_keep": ((2 * n_iters + 2) * tensor, lambda: rpmnet.sinkhorn_slack_keep(A, n_iters, x)),
             "sinkhorn_slack_backward_n0": ((2 + 2 + 2) * tensor, back(0)),
             "sinkhorn_slack_backward_n1": ((4 + 3 + 2) * tensor, back(1)),
             f"sinkhorn_slack_backward_n{n_iters}": ((2 * n_iters + 2 + 3 + 2) * tensor, back(n_iters))}
    res = {}
    for name, (nbytes, fn) in cases.items():
        timed(fn, True)
        ms = statistics.median(timed(fn, True, 5) for _ in range(rounds))
        res[name] = {"ms": round(ms, 4), "GB_per_s": round(nbytes / ms / 1e6, 1)}
    per_iter = (res[f"sinkhorn_slack_backward_n{n_iters}"]["ms"] - res["sinkhorn_slack_backward_n1"]["ms"]) / (n_iters - 1)
    res["backward_ms_per_further_iteration"] = round(per_iter, 4)
    return res


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
    ap.add_argument("--no-matching", action="store_true")
    ap.add_argument("--no-param", action="store_true")
    ap.add_argument("--no-routes", action="store_true", help="skip the TRAIN_HIP on / off pairs (features, step)")
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
        for name, fn in (() if a.no_routes else (("features", features), ("step", step))):
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
        if not a.no_param:
            moved_src = xyz @ R.t() + 0.1

            def param_net():
                net.zero_grad(set_to_none=True)
                beta, alpha = net.weights_net([moved_src, xyz])
                (beta.sum() + alpha.sum()).backward()

            pair(line, "param_net", param_net, a.rounds, "PARAM_HIP")
            pair(line, "step_param", step, a.rounds, "PARAM_HIP")
        if not a.no_matching:
            dist0 = torch.rand(B, N, N, device=dev) * 2
            feat_s = torch.nn.functional.normalize(torch.randn(B, N, fx.postpool[6].out_channels, device=dev), dim=-1)
            feat_t = torch.nn.functional.normalize(torch.randn(B, N, fx.postpool[6].out_channels, device=dev), dim=-1)
            wts = torch.rand(B, N, device=dev)
            moved = xyz @ R.t() + 0.1

            def matching():
                d = dist0.clone().requires_grad_()
                beta = torch.full((B,), 1.5, device=dev, requires_grad=True)
                alpha = torch.full((B,), 0.6, device=dev, requires_grad=True)
                _, perm, rowsum, wt = net.match_stage(d, beta, alpha, xyz)
                rows = rowsum if rowsum is not None else torch.sum(perm, dim=2)
                (perm.sum(2).mean() + (wt * wt).sum() + (rows * wts).sum()).backward()

            def parameter_net():
                net.zero_grad(set_to_none=True)
                beta, alpha = net.weights_net([moved, xyz])
                (beta.sum() + alpha.sum()).backward()

            def feature_distance():
                fs, ft = feat_s.clone().requires_grad_(), feat_t.clone().requires_grad_()
                (rpmnet.match_features(fs, ft) * dist0).sum().backward()

            def kabsch():
                w, b = wts.clone().requires_grad_(), xyz.clone().requires_grad_()
                rpmnet.compute_rigid_transform(moved, b, w).sum().backward()

            pair(line, "matching", matching, a.rounds)
            pair(line, "step_match", step, a.rounds)
            split = {}
            for name, fn in (("parameter_net", parameter_net), ("feature_distance", feature_distance), ("kabsch", kabsch)):
                timed(fn, True)
                split[name + "_ms"] = round(statistics.median(timed(fn, True) for _ in range(a.rounds)), 3)
            line["split"] = split
            line["matching_kernels"] = matching_kernels(B, N, dev, a.rounds, net.num_sk_iter)
        if not a.no_kernels:
            del net, opt
            torch.cuda.empty_cache()
            line["kernels_c96"] = kernel_rates(B, 96, fx.n_sample, N, dev, a.rounds)
            line["kernels_c192"] = kernel_rates(B, 192, fx.n_sample, N, dev, a.rounds)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
