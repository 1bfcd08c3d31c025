"""ms per eval forward of MaskNet (B 32, template 1024 points, source 768) on the fused route against the op-sequence route of the
same build, of Segmentation (B 32, N 1024, 40 classes) likewise, and of the two MaskNet kernels alone: l3d_mask_tail on
[B,256,Nt] against the two torch convs + ReLU + sigmoid it replaces, l3d_mask_select against torch.topk + sort + index_points.
The two sides of each pair run interleaved, round by round, so that clock and thermal drift hits both alike; medians over the rounds.

    python tools/masknet_bench.py [--batch 32] [--rounds 10]
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learning3d_amd import _lib                                          # noqa: E402
from learning3d_amd.models import MaskNet, PointNet, Segmentation        # noqa: E402
from learning3d_amd.models import masknet, segmentation                  # noqa: E402


def timed(fn, fused, reps):
    masknet.FUSED = segmentation.FUSED = fused
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn(fused)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    finally:
        masknet.FUSED = segmentation.FUSED = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--template", type=int, default=1024)
    ap.add_argument("--source", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=50, help="launches per timed window of the two kernels alone")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, Nt, Ns = a.batch, a.template, a.source
    net = MaskNet(is_training=False).eval().to(dev)
    seg = Segmentation(PointNet(global_feat=False, use_bn=True)).eval().to(dev)
    template = torch.rand(B, Nt, 3, device=dev) * 2 - 1
    source = template[:, torch.randperm(Nt, device=dev)[:Ns]].contiguous()
    h3 = net.maskNet.h3
    x = torch.randn(B, 256, Nt, device=dev)
    mask = torch.rand(B, Nt, device=dev)
    w6, b6 = h3[6].weight.detach().reshape(128, 256).contiguous(), h3[6].bias.detach()
    w8, b8 = h3[8].weight.detach().reshape(128).contiguous(), h3[8].bias.detach()
    out = torch.empty(B, Nt, device=dev)

    def tail(fused):
        if fused:
            _lib.call("l3d_mask_tail", x, w6, b6, w8, b8, B, 256, 128, Nt, out)
        else:
            h3[6:](x)

    def select(fused):
        if fused:
            masknet.mask_select(mask, template, Ns)
        else:
            idx = torch.topk(mask, Ns, dim=1, sorted=False)[1].sort(dim=1)[0]
            MaskNet.index_points(template, idx)
    cases = {"masknet": lambda fused: net(template, source, "topk"), "segmentation": lambda fused: seg(template), "tail": tail,
             "select": select}
    res = {name: {True: [], False: []} for name in cases}
    with torch.no_grad():
        for name, fn in cases.items():
            reps = a.kernel_reps if name in ("tail", "select") else a.reps
            for fused in (True, False):
                timed(fn, fused, 1)                       # warm-up: caches, lazy module loads
            for _ in range(a.rounds):
                for fused in (True, False):
                    res[name][fused].append(timed(fn, fused, reps))
    med = lambda v: round(statistics.median(v), 4)
    line = {"batch": B, "template_points": Nt, "source_points": Ns, "rounds": a.rounds}
    for name in cases:
        line[name + "_ms_fused"] = med(res[name][True])
        line[name + "_ms_op_sequence"] = med(res[name][False])
    print(json.dumps(line))


if __name__ == "__main__":
    main()
