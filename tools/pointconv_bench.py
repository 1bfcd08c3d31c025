"""ms per eval forward of the PointConv network (B 32, 1024 points, embedding and classifier) on the fused route against the
op-sequence route of the same build, and l3d_pointconv_aggregate alone at the three layers' shapes against the torch ops it
replaces (DensityNet, the broadcast product, WeightNet, the per-centre matmuls) and against its HBM bound: feat read once, out
written once, at --hbm-tbs TB/s.  The two sides of each pair run interleaved, round by round, so that clock and thermal drift
hits both alike; medians over the rounds.

    python tools/pointconv_bench.py [--batch 32] [--points 1024] [--rounds 10]
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learning3d_amd.models import create_pointconv                     # noqa: E402
from learning3d_amd.utils import pointconv_util as PU                  # noqa: E402


def timed(fn, fused, reps):
    PU.FUSED = fused
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn(fused)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    finally:
        PU.FUSED = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM bandwidth the bound is stated against, TB/s")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, N = a.batch, a.points
    Net = create_pointconv()
    emb = Net(input_channel_dim=3).eval().to(dev)
    cls = Net(input_channel_dim=6, classifier=True).eval().to(dev)
    x3 = torch.rand(B, N, 3, device=dev) - 0.5
    x6 = torch.cat([x3, torch.nn.functional.normalize(torch.randn(B, N, 3, device=dev), dim=-1)], dim=-1)
    cases = {"embedding": lambda fused: emb(x3), "classifier": lambda fused: cls(x6)}
    bound = {}
    for name, sa, S, K in (("aggregate_sa1", emb.sa1, 512, 32), ("aggregate_sa2", emb.sa2, 128, 64), ("aggregate_sa3", emb.sa3, 1, emb.sa2.npoint)):
        Cc = sa.mlp_convs[-1].out_channels
        feat = torch.relu(torch.randn(B, Cc, K, S, device=dev))
        gxyz = (torch.rand(B, S, K, 3, device=dev) - 0.5) * 0.3
        ginv = torch.rand(B, S, K, device=dev) + 0.5
        wn, dn = PU._packed_net(sa.weightnet), PU._packed_net(sa.densitynet)

        def run(fused, sa=sa, feat=feat, gxyz=gxyz, ginv=ginv, wn=wn, dn=dn, S=S):
            if fused:
                PU.pointconv_aggregate(feat, gxyz, ginv, wn, dn)
            else:
                scale = (ginv / ginv.max(dim=2, keepdim=True)[0])[:, :, :, None]
                y = feat * sa.densitynet(scale.permute(0, 3, 2, 1))
                w = sa.weightnet(gxyz.permute(0, 3, 2, 1))
                torch.matmul(y.permute(0, 3, 1, 2), w.permute(0, 3, 2, 1)).view(feat.shape[0], S, -1)
        cases[name] = run
        nbytes = 4 * (feat.numel() + 16 * B * Cc * S + gxyz.numel() + ginv.numel())
        bound[name] = (nbytes, nbytes / (a.hbm_tbs * 1e12) * 1e3)
    res = {name: {True: [], False: []} for name in cases}
    with torch.no_grad():
        for name, fn in cases.items():
            for fused in (True, False):
                timed(fn, fused, 1)                       # warm-up: caches, lazy module loads
            for _ in range(a.rounds):
                for fused in (True, False):
                    res[name][fused].append(timed(fn, fused, a.reps))
    med = lambda v: round(statistics.median(v), 4)      # noqa: E731
    line = {"batch": B, "points": N, "rounds": a.rounds, "hbm_tbs": a.hbm_tbs}
    for name in cases:
        line[name + "_ms_fused"] = med(res[name][True])
        line[name + "_ms_op_sequence"] = med(res[name][False])
        if name in bound:
            line[name + "_mbytes"] = round(bound[name][0] / 1e6, 1)
            line[name + "_ms_hbm_bound"] = round(bound[name][1], 4)
            line[name + "_gbs"] = round(bound[name][0] / 1e9 / (line[name + "_ms_fused"] * 1e-3), 0)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
