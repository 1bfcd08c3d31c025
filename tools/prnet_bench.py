"""ms per eval forward of PRNet (the reference's default: B 32, 768 points, 512 keypoints, emb 512, 3 iterations) on the fused route
against the op-sequence route of the same build, and the two new entry points alone at that shape against the torch ops they
replace: l3d_soft_correspondence_pair against one score matmul, a last-axis softmax of the [B,K,K] scores and of their transposed
copy, and two matmuls behind transposed copies (less than the reference's two head calls, which form the scores twice; the
cheapest torch form measured, see `pair`); l3d_prnet_keypoints against add, norm, topk, sort and the gathers and means.  The two sides of each pair run interleaved, round by round, so that
clock and thermal drift hits both alike; medians over the rounds.

    python tools/prnet_bench.py [--batch 32] [--points 768] [--keypoints 512] [--emb 512] [--iters 3] [--rounds 10]
Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learning3d_amd.models import prnet as P                           # noqa: E402


def timed(fn, fused, reps):
    P.FUSED = fused
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn(fused)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    finally:
        P.FUSED = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=768)
    ap.add_argument("--keypoints", type=int, default=512)
    ap.add_argument("--emb", type=int, default=512)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, N, K, C = a.batch, a.points, a.keypoints, a.emb
    net = P.PRNet(emb_dims=C, num_keypoints=K, num_subsampled_points=N, num_iters=a.iters).eval().to(dev)
    with torch.no_grad():
        net.temp_net.nn[9].bias.fill_(5.0)                    # a temperature inside the clamp, a peaked softmax
    tgt = torch.rand(B, N, 3, device=dev) - 0.5
    src = tgt[:, torch.randperm(N, device=dev)] + 0.05
    emb, emb_p = torch.randn(B, C, N, device=dev), torch.randn(B, C, N, device=dev)
    xyz = src.permute(0, 2, 1).contiguous()
    se, te = torch.randn(B, C, K, device=dev), torch.randn(B, C, K, device=dev)
    ps, pt = torch.rand(B, 3, K, device=dev), torch.rand(B, 3, K, device=dev)
    temp = torch.full((B,), 5.0, device=dev)

    def pair(fused):
        if fused:
            return P.soft_correspondence_pair(se, te, ps, pt, temp)
        scaled = temp.view(B, 1, 1) * (torch.matmul(se.transpose(2, 1).contiguous(), te) / math.sqrt(C))
        # one score matrix for both directions (the reference's two head calls form it twice).  The second direction softmaxes a
        # transposed copy along its last axis: measured, that is torch's cheapest form -- softmax(scaled, dim=1) on the same scores
        # without the copy took the whole baseline from 0.329 to 0.607 ms at the default shape
        return (torch.matmul(pt, torch.softmax(scaled, dim=2).transpose(2, 1).contiguous()),
                torch.matmul(ps, torch.softmax(scaled.transpose(2, 1).contiguous(), dim=2).transpose(2, 1).contiguous()))

    def keypoints(fused):
        if fused:
            return P.keypoints(emb, emb_p, xyz, K)
        e = emb + emb_p
        idx = torch.topk(torch.norm(e, dim=1, keepdim=True), k=K, dim=2, sorted=False)[1].sort(dim=2)[0]
        e_k = torch.gather(e, 2, idx.repeat(1, C, 1))
        return torch.gather(xyz, 2, idx.repeat(1, 3, 1)), e_k, e_k.mean(dim=2)

    cases = {"forward": lambda fused: net(src, tgt), "softcorr_pair": pair, "keypoints": keypoints}
    res = {name: {True: [], False: []} for name in cases}
    with torch.no_grad():
        for name, fn in cases.items():
            for fused in (True, False):
                timed(fn, fused, 1)                       # warm-up: caches, lazy module loads
            for _ in range(a.rounds):
                for fused in (True, False):
                    res[name][fused].append(timed(fn, fused, a.reps))
        # where the fused forward's time goes: HIP-event spans around its stages, one forward
        from learning3d_amd.models import _fused
        _fused.TIMER = _fused.StageTimer(only={"prnet_embed", "prnet_attention", "prnet_keypoints", "prnet_temperature",
                                               "prnet_softcorr_pair", "prnet_kabsch"})
        try:
            net(src, tgt)
            torch.cuda.synchronize()
            stages = {k: round(v * a.iters, 4) for k, v in _fused.TIMER.mean_ms().items()}
        finally:
            _fused.TIMER = None
    med = lambda v: round(statistics.median(v), 4)      # noqa: E731
    line = {"batch": B, "points": N, "keypoints": K, "emb": C, "iters": a.iters, "rounds": a.rounds}
    for name in cases:
        line[name + "_ms_fused"] = med(res[name][True])
        line[name + "_ms_op_sequence"] = med(res[name][False])
    line["fused_forward_stage_ms"] = stages
    print(json.dumps(line))


if __name__ == "__main__":
    main()
