#!/usr/bin/env python3
"""Chamfer forward, us per call: exact per-pair kernel (variant 2) vs matrix-core ranking + exact refinement (variant 3) vs grid
pruning (variant 4, up to 2048 points).  Every (shape, variant) is captured as a graph of CALLS back-to-back launches and the
graph replayed REPS times: the line gives the fastest and the slowest replay, so a difference between two variants can be held
against the runs' own spread (the dispatch window of l3d_chamfer_forward_variant is where variant 4's slowest beats variant 2's
fastest)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learning3d_amd._lib import check, lib, ptr, stream_ptr      # noqa: E402

CALLS, REPS = 20, 7


def replay_us(fn):
    """[us per call] of REPS replays of a graph of CALLS launches of fn"""
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / CALLS * 1e3)
    return out


for B, N in ((32, 128), (32, 256), (32, 512), (32, 1024), (32, 2048), (16, 4096), (8, 16384), (64, 16384)):
    a, b = torch.rand(B, N, 3, device="cuda") - 0.5, torch.rand(B, N, 3, device="cuda") - 0.5
    d1, d2 = torch.empty(B, N, device="cuda"), torch.empty(B, N, device="cuda")
    i1, i2 = torch.empty(B, N, dtype=torch.int32, device="cuda"), torch.empty(B, N, dtype=torch.int32, device="cuda")
    for v, name in ((2, "packed-exact"), (3, "mfma-ranked"), (4, "grid-pruned")):
        if (v == 3 and N < 1024) or (v == 4 and N > 2048):
            continue
        t = replay_us(lambda: check(lib().l3d_chamfer_forward_variant(ptr(a), ptr(b), B, N, N, ptr(d1), ptr(d2), ptr(i1), ptr(i2), v, stream_ptr()), "cd"))
        print(f"chamfer_fwd B{B} N{N} {name:13s} {min(t):10.1f} .. {max(t):8.1f} us  {2.0 * B * N * N / min(t) / 1e3:9.1f} Gpair/s", flush=True)
