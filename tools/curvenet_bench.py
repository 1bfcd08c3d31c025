"""ms per eval forward of CurveNet ('default', B 32, N 1024) on the fused route against the op-sequence route of the same build,
and of one curve grouping (cic11's shape: C 16, k 20, 100 curves x 5 steps) alone.  The two routes run interleaved, round by
round, so that clock and thermal drift hits both alike; medians over the rounds.

    python tools/curvenet_bench.py [--batch 32] [--rounds 10]
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learning3d_amd.models import CurveNet                      # noqa: E402
from learning3d_amd.utils import curvenet_util as cu            # noqa: E402
from learning3d_amd.utils.model_common_utils import knn         # noqa: E402


def timed(fn, fused, reps):
    cu.FUSED_WALK = fused
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    finally:
        cu.FUSED_WALK = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = CurveNet().eval().to(dev)
    cloud = torch.rand(a.batch, 1024, 3, device=dev) * 2 - 1
    grp = cu.CurveGrouping(16, 20, 100, 5).eval().to(dev)
    x, xyz = torch.randn(a.batch, 16, 1024, device=dev), cloud.transpose(1, 2).contiguous()
    res = {"net": {True: [], False: []}, "walk": {True: [], False: []}}
    with torch.no_grad():
        idx = knn(xyz, 20, add_one_to_k=True)[:, :, 1:].contiguous()
        cases = {"net": lambda: net(cloud), "walk": lambda: grp(x, xyz, idx)}
        for name, fn in cases.items():
            for fused in (True, False):
                timed(fn, fused, 1)                       # warm-up: caches, lazy module loads
            for _ in range(a.rounds):
                for fused in (True, False):
                    res[name][fused].append(timed(fn, fused, a.reps))
    med = lambda v: round(statistics.median(v), 4)
    print(json.dumps({"batch": a.batch, "points": 1024, "rounds": a.rounds,
                      "forward_ms_fused": med(res["net"][True]), "forward_ms_op_sequence": med(res["net"][False]),
                      "grouping_ms_fused": med(res["walk"][True]), "grouping_ms_op_sequence": med(res["walk"][False])}))


if __name__ == "__main__":
    main()
