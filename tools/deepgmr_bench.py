"""ms per eval forward of DeepGMR (B 32, 1024 points in both clouds, k 20, J 16, d_model 1024) on the fused route against the
op-sequence route of the same build, in both input formats ([B,N,3+4k] with the features given, [B,N,3] with the features computed
inside); rri_features alone on the device against the CPU get_rri of the same batch (one cloud after another, as a dataset worker
computes them); and the three kernels of deepgmr.hip alone against the torch op sequences they replace.  The two sides of each pair
run interleaved, round by round, so that clock and thermal drift hits both alike; medians over the rounds.  The CPU get_rri is
timed once per round with the wall clock.

    python tools/deepgmr_bench.py [--batch 32] [--points 1024] [--neighbors 20] [--clusters 16] [--rounds 10]
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learning3d_amd.data_utils import get_rri, rri_features             # noqa: E402
from learning3d_amd.data_utils.rri import knn_idx, rri_from_idx, rri_geometry         # noqa: E402
from learning3d_amd.models import DeepGMR                                # noqa: E402
from learning3d_amd.models import deepgmr                                # noqa: E402


def timed(fn, fused, reps):
    deepgmr.FUSED = fused
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn(fused)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    finally:
        deepgmr.FUSED = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--neighbors", type=int, default=20)
    ap.add_argument("--clusters", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=10, help="launches per timed window of a kernel alone")
    ap.add_argument("--cpu-clouds", type=int, default=4, help="clouds of the batch the CPU get_rri is timed on (scaled to the batch)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, N, k, J = a.batch, a.points, a.neighbors, a.clusters
    net = DeepGMR(use_rri=True, nearest_neighbors=k, n_clusters=J).eval().to(dev)
    template = torch.rand(B, N, 3, device=dev) * 2 - 1
    ang = torch.tensor(0.6)
    R = torch.tensor([[ang.cos(), -ang.sin(), 0.0], [ang.sin(), ang.cos(), 0.0], [0.0, 0.0, 1.0]], device=dev)
    source = template @ R.t() + 0.3
    with torch.no_grad():
        tf, sf = (torch.cat([c, rri_features(c, k)], dim=2) for c in (template, source))
    centred = template - template.mean(dim=1, keepdim=True)
    idx = knn_idx(centred, k)
    logits = torch.randn(2 * B, J, N, device=dev)
    pts = torch.cat([template, source])
    gamma, pi, mu, var = deepgmr.gmm_fit(logits, pts)
    sigma = var[:, :, None, None] * torch.eye(3, device=dev)
    cpu = centred.cpu()

    def gmm_params(fused):
        if fused:
            deepgmr.gmm_fit(logits, pts)
        else:
            deepgmr.gmm_params(torch.softmax(logits.transpose(1, 2), dim=2), pts)

    def gmm_register(fused):
        if fused:
            deepgmr.gmm_register_fused(pi[:B], mu[:B], mu[B:], var[B:])
        else:
            deepgmr.gmm_register(pi[:B], mu[:B], mu[B:], sigma[B:])

    def rri_torch():
        # the torch side of the feature kernel: the package's batched restatement of get_rri, on the device in fp32
        rp, rq, theta, psi = rri_geometry(centred, idx)
        return torch.cat([rp, rq, theta, torch.kthvalue(psi, 2, dim=-1, keepdim=True)[0]], dim=-1)

    cases = {"deepgmr_features_given": lambda fused: net(tf, sf),
             "deepgmr_points_only": lambda fused: net(template, source),
             "gmm_params": gmm_params,
             "gmm_register": gmm_register,
             "rri_kernel": lambda fused: rri_from_idx(centred, idx) if fused else rri_torch()}
    res = {name: {True: [], False: []} for name in cases}
    rri_dev, rri_cpu = [], []
    with torch.no_grad():
        for name, fn in cases.items():
            reps = a.reps if name.startswith("deepgmr") else a.kernel_reps
            for fused in (True, False):
                timed(fn, fused, 1)                       # warm-up: caches, lazy module loads
            for _ in range(a.rounds):
                for fused in (True, False):
                    res[name][fused].append(timed(fn, fused, reps))
        for _ in range(a.rounds):
            rri_dev.append(timed(lambda fused: rri_features(template, k), True, a.kernel_reps))
            t0 = time.perf_counter()
            for b in range(min(a.cpu_clouds, B)):
                get_rri(cpu[b].numpy(), k)
            rri_cpu.append((time.perf_counter() - t0) * 1e3 * B / min(a.cpu_clouds, B))
    med = lambda v: round(statistics.median(v), 4)      # noqa: E731
    line = {"batch": B, "points": N, "neighbors": k, "clusters": J, "rounds": a.rounds}
    for name in cases:
        line[name + "_ms_fused"] = med(res[name][True])
        line[name + "_ms_op_sequence"] = med(res[name][False])
    line["rri_features_ms_device"] = med(rri_dev)
    line["rri_features_ms_cpu_get_rri"] = med(rri_cpu)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
