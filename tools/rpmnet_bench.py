"""ms per eval forward of RPMNet (B 32, 1024 points with normals in both clouds, max_iterations 1, 2 and 5) on the fused route
against the op-sequence route of the same build, and the kernels of rpmnet.hip alone against the torch ops they replace
(l3d_gn_affine is not timed separately: it runs behind every l3d_gn_conv of the pre-pool stack).  The two sides of each pair run
interleaved, round by round, so that clock and thermal drift hits both alike; medians over the rounds.
param_net_* and fused_iters*_param_*: ParameterPredictionNet alone (no_grad) and the whole fused forward with rpmnet.PARAM_HIP on and
off, everything else fused on both sides; [median, min, max] over the rounds.

    python tools/rpmnet_bench.py [--batch 32] [--points 1024] [--rounds 10]
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learning3d_amd.models import RPMNet, ppfnet, rpmnet              # noqa: E402
from learning3d_amd.utils import ppfnet_util                           # noqa: E402


def timed(fn, fused, reps):
    rpmnet.FUSED = fused
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn(fused)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    finally:
        rpmnet.FUSED = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--iterations", type=int, nargs="+", default=[1, 2, 5])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, N = a.batch, a.points
    net = RPMNet().eval().to(dev)
    fx = net.feat_extractor
    K = fx.n_sample
    xyz = torch.rand(B, N, 3, device=dev) * 2 - 1
    nrm = torch.nn.functional.normalize(torch.randn(B, N, 3, device=dev), dim=-1)
    ang = torch.tensor(0.5)
    R = torch.tensor([[ang.cos(), -ang.sin(), 0.0], [ang.sin(), ang.cos(), 0.0], [0.0, 0.0, 1.0]], device=dev)
    template = torch.cat([xyz, nrm], dim=-1)
    source = torch.cat([xyz @ R.t() + 0.1, nrm @ R.t()], dim=-1)
    with torch.no_grad():
        idx = ppfnet_util.query_ball_point(fx.radius, K, xyz, xyz, itself_indices=torch.arange(N, device=dev)[None].repeat(B, 1))
        grouped = ppfnet.ppf_group(xyz, nrm, idx)
    affinity = torch.randn(B, N, N, device=dev) * 3
    weights = torch.rand(B, N, device=dev)

    def group(fused):
        if fused:
            ppfnet.ppf_group(xyz, nrm, idx)
        else:
            # the torch ops behind the ball query, on the same precomputed idx
            d = ppfnet._index_points(xyz, idx) - xyz[:, :, None, :]
            nr, ni = nrm[:, :, None, :], ppfnet._index_points(nrm, idx)
            angle = ppfnet_util.angle
            ppf = torch.stack([angle(nr, d), angle(ni, d), angle(nr, ni), torch.norm(d, dim=-1)], dim=-1)
            torch.cat([xyz[:, :, None, :].expand(-1, -1, K, -1), d, ppf], -1).permute(0, 3, 2, 1).contiguous()

    def prepool(fused):
        if fused:
            x = grouped.view(B, 10, K * N)
            y, _, _, m = ppfnet.gn_conv(x, None, None, fx.prepool[0].weight, fx.prepool[0].bias)
            s = ppfnet.gn_affine(m, fx.prepool[1], K * N)
            y, _, _, m = ppfnet.gn_conv(y, *s, fx.prepool[3].weight, fx.prepool[3].bias)
            s = ppfnet.gn_affine(m, fx.prepool[4], K * N)
            ppfnet.gn_conv(y, *s, fx.prepool[6].weight, fx.prepool[6].bias, pool=K, want_y=False)
        else:
            fx.prepool(grouped).max(dim=2)

    cases = {f"rpmnet_iters{n}": (lambda fused, n=n: net(template, source, n)) for n in a.iterations}
    cases.update({"ppf_group": group, "prepool_stack": prepool,
                  "sinkhorn": lambda fused: rpmnet.sinkhorn(affinity, 5),
                  "rigid_transform": lambda fused: rpmnet.rigid_transform_weighted(xyz, xyz, weights) if fused
                  else rpmnet.compute_rigid_transform(xyz, xyz, weights)})
    res = {name: {True: [], False: []} for name in cases}
    with torch.no_grad():
        for name, fn in cases.items():
            for fused in (True, False):
                timed(fn, fused, 1)                       # warm-up: caches, lazy module loads
            for _ in range(a.rounds):
                for fused in (True, False):
                    res[name][fused].append(timed(fn, fused, a.reps))
    med = lambda v: round(statistics.median(v), 4)      # noqa: E731
    line = {"batch": B, "points": N, "neighbors": K, "rounds": a.rounds}
    for name in cases:
        line[name + "_ms_fused"] = med(res[name][True])
        line[name + "_ms_op_sequence"] = med(res[name][False])

    # PARAM_HIP on / off, FUSED on on both sides
    wn, moved = net.weights_net, xyz @ R.t() + 0.1

    def param_net():
        if rpmnet.PARAM_HIP:
            wn.fused_forward([moved, xyz])
        else:
            wn([moved, xyz])
    ab = {"param_net": param_net}
    ab.update({f"fused_iters{n}_param": (lambda n=n: net(template, source, n)) for n in a.iterations})
    sides = {"hip": True, "torch": False}
    ms = {name: {k: [] for k in sides} for name in ab}
    with torch.no_grad():
        for name, fn in ab.items():
            for rounds in (1, a.rounds):                  # one warm-up round, then the timed ones
                for r in range(rounds):
                    for k, on in sides.items():
                        rpmnet.PARAM_HIP = on
                        try:
                            t = timed(lambda fused: fn(), True, a.reps)
                        finally:
                            rpmnet.PARAM_HIP = True
                        if rounds > 1:
                            ms[name][k].append(t)
    for name in ab:
        for k in sides:
            line[f"{name}_ms_{k}"] = [med(ms[name][k]), round(min(ms[name][k]), 4), round(max(ms[name][k]), 4)]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
