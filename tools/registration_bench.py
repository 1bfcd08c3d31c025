"""ms per forward of PointNetLK (maxiter 10) and iPCRNet (max_iteration 8) at B 32, N 1024: the fused route (registration.hip)
against the op-sequence route of the same build on the same GPU, interleaved; and the number of kernel launches of one forward of
each route, counted by rocprofv3 --kernel-trace --stats in fresh child processes (launches of 2 forwards minus launches of 1).

    python tools/registration_bench.py [--reps 20] [--no-launch-count] [--out FILE.json]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(model, B=32, N=1024):
    import numpy as np
    import torch
    from learning3d_amd.models import PointNet, PointNetLK, iPCRNet
    from learning3d_amd.ops import se3
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    tpl = (torch.rand(B, N, 3, generator=g) * 2 - 1) * torch.tensor([1.0, 0.6, 0.3])
    src = se3.transform(se3.exp(torch.randn(B, 6, generator=g) * 0.1).unsqueeze(1), tpl)
    torch.manual_seed(3)
    if model == "pnlk":
        net = PointNetLK(PointNet(emb_dims=1024, use_bn=True))
        w = os.path.join(ROOT, "tests", "golden", "pnlk_trained_weights.npz")
        net.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in np.load(w).items()}, strict=True)
        run = lambda: net(tpl_d, src_d, maxiter=10)            # noqa: E731
    else:
        net = iPCRNet(PointNet(emb_dims=1024))
        run = lambda: net(tpl_d, src_d, max_iteration=8)       # noqa: E731
    net = net.eval().to(dev)
    tpl_d, src_d = tpl.to(dev), src.to(dev)
    return run


def forwards(model, route, n):
    import torch
    from learning3d_amd.models import pointnetlk
    pointnetlk.FUSED_LOOP = route == "fused"
    run = make(model)
    with torch.no_grad():
        for _ in range(n):
            run()
    torch.cuda.synchronize()


def time_routes(model, reps):
    import torch
    from learning3d_amd.models import pointnetlk
    run = make(model)
    times = {"fused": [], "opseq": []}
    with torch.no_grad():
        for rep in range(reps + 3):
            for route in ("fused", "opseq"):
                pointnetlk.FUSED_LOOP = route == "fused"
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run()
                b.record()
                torch.cuda.synchronize()
                if rep >= 3:
                    times[route].append(a.elapsed_time(b))
    pointnetlk.FUSED_LOOP = True
    return {r: {"median_ms": sorted(t)[len(t) // 2], "min_ms": min(t)} for r, t in times.items()}


def count_launches(model, route):
    counts = []
    for n in (1, 2):
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                   "--child", model, route, str(n)]
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240)
            total = 0
            for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                with open(path) as f:
                    total += sum(int(row["Calls"]) for row in csv.DictReader(f))
            if total == 0:                               # no statistics file: count the trace's rows
                for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                    with open(path) as f:
                        total += sum(1 for _ in csv.DictReader(f))
            counts.append(total)
    return counts[1] - counts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=3)
    a = ap.parse_args()
    if a.child:
        forwards(a.child[0], a.child[1], int(a.child[2]))
        return
    out = {"B": 32, "N": 1024}
    for model in ("pnlk", "ipcrnet"):
        out[model] = time_routes(model, a.reps)
        if not a.no_launch_count:
            for route in ("fused", "opseq"):
                out[model][route]["launches_per_forward"] = count_launches(model, route)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
