"""ms per call of l3d_crop_select (the source's launch of a partial + noisy batch: nearest mode, mask, gather and fused jitter) against
torch's cheapest equivalent on the device -- fp64 squared distances in the kernel's association, topk(sorted=True), a gather of
the rows, a scatter for the mask, and the clamped noise added -- and ms per batch of ResidentRegistrationFeed with partial_source,
partial_template, noise and masks on, with the same crops done by those torch ops, and with the options off.  B 32, K 768, N 1024 and
2048 by default.  The sides of a comparison run interleaved, round by round, so that clock and thermal drift hits them alike;
medians over the rounds, and the spread (min .. max) beside them.  Both sides are checked to give the same bits before anything is
timed.

    python tools/partial_feed_bench.py [--batch 32] [--points 1024 2048] [--keep 768] [--rounds 10] [--reps 200] [--epochs 4]
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learning3d_amd import _lib                                        # noqa: E402
from learning3d_amd.data_utils import ResidentRegistrationFeed          # noqa: E402
from learning3d_amd.data_utils import partial as P                     # noqa: E402

CLIP = 0.05


def torch_crop(points, view, K, noise=None, sigma=None):
    """the same crop in torch ops: -> (mask [B,N], out [B,K,C])"""
    d = points[:, :, :3].double() - view[:, None, :]
    key = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    idx = torch.topk(key, K, dim=1, largest=False, sorted=True)[1]
    out = torch.gather(points, 1, idx[:, :, None].expand(-1, -1, points.shape[2]))
    mask = torch.zeros(points.shape[:2], dtype=torch.float32, device=points.device).scatter_(1, idx, 1.0)
    if noise is not None:
        out = out + (sigma[:, None, None] * noise).clamp(-CLIP, CLIP)
    return mask, out


class TorchCropFeed(ResidentRegistrationFeed):
    """the feed with its crops done by torch_crop (nearest mode only): the baseline of the whole batch"""

    def crop_batch(self, template, source, draws):
        s_mask, source = torch_crop(source, draws["source"], self.num_kept, draws.get("noise"), draws.get("sigma"))
        t_mask, template = torch_crop(template, draws["template"], self.num_kept)
        return template, source, (t_mask, s_mask)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def interleaved(sides, rounds, reps):
    """{name: fn} -> {name: [ms per call, one per round]}"""
    res = {name: [] for name in sides}
    for fn in sides.values():
        timed(fn, 2)                                      # warm-up: code objects, the allocator's blocks
    for _ in range(rounds):
        for name, fn in sides.items():
            res[name].append(timed(fn, reps))
    return res


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--keep", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--batches", type=int, default=8, help="batches per epoch of the feed's dataset")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("partial_feed_bench.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    B, K = a.batch, a.keep
    line = {"batch": B, "keep": K, "rounds": a.rounds, "reps": a.reps, "shapes": {}}
    for N in a.points:
        g = torch.Generator(device=dev).manual_seed(N)
        points = torch.rand((B, N, 3), device=dev, generator=g) * 2 - 1
        view = P.draw_views(B, dev, g)
        noise = torch.randn((B, K, 3), device=dev, generator=g)
        sigma = P.JITTER_SCALE * torch.rand((B,), device=dev, generator=g)

        def kernel():
            return P.crop_select(points, view, _lib.L3D_CROP_NEAREST, K, noise=noise, sigma=sigma, clip=CLIP, want_idx=False)

        def baseline():
            return torch_crop(points, view, K, noise, sigma)
        (_, m0, o0), (m1, o1) = kernel(), baseline()
        same = bool(torch.equal(m0, m1) and torch.equal(o0, o1))
        res = interleaved({"crop_select": kernel, "torch_ops": baseline}, a.rounds, a.reps)

        data = torch.rand((B * a.batches, N, 3), device=dev, generator=g) * 2 - 1
        on = dict(partial_source=True, partial_template=True, num_subsampled_points=K, noise=True, masks=True)
        feeds = {"feed_partial_noise_masks": ResidentRegistrationFeed(data, batch_size=B, num_points=N, seed=1, **on),
                 "feed_same_crops_in_torch_ops": TorchCropFeed(data, batch_size=B, num_points=N, seed=1, **on),
                 "feed_options_off": ResidentRegistrationFeed(data, batch_size=B, num_points=N, seed=1)}
        first = {name: next(iter(f)) for name, f in feeds.items()}
        for f in feeds.values():
            f.epoch = 0
        same_feed = all(torch.equal(x, y) for x, y in zip(first["feed_partial_noise_masks"], first["feed_same_crops_in_torch_ops"])
                        if x is not None)

        def epoch(feed):
            def run():
                for _ in feed:
                    pass
            return run
        fres = interleaved({name: epoch(f) for name, f in feeds.items()}, a.rounds, a.epochs)
        shape = {"kernel_and_torch_ops_same_bits": same, "feed_and_torch_feed_same_bits": same_feed}
        shape.update({name: summary(v) for name, v in res.items()})
        shape.update({name + "_per_batch": summary([t / a.batches for t in v]) for name, v in fres.items()})
        line["shapes"][f"N{N}"] = shape
    print(json.dumps(line))


if __name__ == "__main__":
    main()
