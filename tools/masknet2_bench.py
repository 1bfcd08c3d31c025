"""ms per eval forward of MaskNet2's mask network (B 32, 1024 points in both clouds) on the fused route against the op-sequence route of
the same build, and of l3d_self_attention_shared alone, per width of the feature model (32, 64, 128, 224) on [2B,D,N], against the
three torch ops it replaces (bmm, softmax, bmm) plus the axpy.  The two sides of each pair run interleaved, round by round, so that
clock and thermal drift hits both alike; medians over the rounds.

    python tools/masknet2_bench.py [--batch 32] [--points 1024] [--rounds 10]
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learning3d_amd import _lib                                          # noqa: E402
from learning3d_amd.models import MaskNet2                               # noqa: E402
from learning3d_amd.models import masknet2                               # noqa: E402

WIDTHS = (32, 64, 128, 224)


def timed(fn, fused, reps):
    masknet2.FUSED = fused
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn(fused)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    finally:
        masknet2.FUSED = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=10, help="launches per timed window of the attention kernel alone")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, N = a.batch, a.points
    net = MaskNet2(is_training=False).eval().to(dev)
    with torch.no_grad():
        for m in net.modules():
            if hasattr(m, "beta"):
                m.beta.fill_(0.1)                         # the reference's initial 0 would make every attention a no-op in value
    template, source = torch.rand(B, N, 3, device=dev) * 2 - 1, torch.rand(B, N, 3, device=dev) * 2 - 1
    beta = torch.full((1,), 0.1, device=dev)
    cases = {"masknet2": lambda fused: net.maskNet(template, source)}

    def attention(D):
        q = torch.randn(2 * B, D, N, device=dev) * (4.0 / D) ** 0.5        # logits of a few units, as behind BatchNorm + Mish
        out = torch.empty_like(q)

        def run(fused):
            if fused:
                _lib.call("l3d_self_attention_shared", q, beta, 2 * B, D, N, out)
            else:
                p = torch.softmax(torch.bmm(q.permute(0, 2, 1), q), dim=-1)
                torch.add(q, torch.bmm(q, p.permute(0, 2, 1)), alpha=0.1)
        return run
    for D in WIDTHS:
        cases[f"attention_d{D}"] = attention(D)
    res = {name: {True: [], False: []} for name in cases}
    with torch.no_grad():
        for name, fn in cases.items():
            reps = a.reps if name == "masknet2" else a.kernel_reps
            for fused in (True, False):
                timed(fn, fused, 1)                       # warm-up: caches, lazy module loads
            for _ in range(a.rounds):
                for fused in (True, False):
                    res[name][fused].append(timed(fn, fused, reps))
    med = lambda v: round(statistics.median(v), 4)      # noqa: E731
    line = {"batch": B, "points": N, "rounds": a.rounds}
    for name in cases:
        line[name + "_ms_fused"] = med(res[name][True])
        line[name + "_ms_op_sequence"] = med(res[name][False])
    flops = 4.0 * 2 * B * N * N * sum((32, 64, 64, 128, 224))
    line["attention_gflop_per_forward"] = round(flops / 1e9, 1)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
