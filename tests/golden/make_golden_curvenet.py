"""Fixtures of CurveNet (the curve walk and one CIC block's gradients), from the REFERENCE on the CPU:

    python tests/golden/make_golden_curvenet.py

Needs the reference checkout make_golden.py reads.  Writes, next to this file, curve_walk.npz, curvenet_grad.npz and
curvenet_seeded.npz: arrays only.  Every result is stored twice, computed in fp32 and in fp64 (`net.double()`).

The walk picks a point per step with an arg-max, and one flipped pick changes the rest of its curve.  So the reference module's
gumbel_softmax is wrapped to record every step's logits, and each curve gets its MARGIN: the smallest gap between its two
largest fp64 logits over its steps.  Tests compare only curves whose margin exceeds tau, and tau is measured here, per fixture:
32 x the largest |fp32 logit - fp64 logit| the reference itself shows on steps that both runs reached over the same points (32:
room for another summation order over at most 2 C = 64 terms).  Asserted below: at most 5 % of a shape's curves sit at or below
tau, the attention gap between the last selected and the first unselected start point exceeds tau, no two logits of a step tie,
and for curvenet_grad the weight seed is stepped from a fixed start until EVERY curve clears tau.

curvenet_seeded.npz (the whole classifier, 'default', B 2, N 1024) follows the per-shape rule, block by block: inside the network the
walks are far less decided than the stand-alone ones (a block's tau is 4e-6 to 1e-4 there, because the fp32 run's walk INPUTS already
differ from the fp64 run's), and no seeded weight set was found that every one of the 800 curves clears.  The weight seed is stepped
until, in each of the four blocks, the fp32 and fp64 runs start from the same list, walk identical paths, and at most 5 % of the
curves sit at or below tau.  Each block's start list (in the run's order), paths, margins and tau are stored; the tests hand the
walks those start lists, require the paths above tau, and compare the 40 logits when the curves at or below tau agree as well.

Curves are keyed by their start point: torch.topk(sorted=False) returns the selected points in no particular order, so every
per-curve array is stored in ascending order of the start index within its cloud.  The ORDER of the start points is an input of
the walk all the same: the reference views the momentum softmax [bs,2,n] as [bs,1,n,2] without transposing it (:147), so the curve at
position q of the list blends with the values at flat positions 2 q and 2 q + 1 of its cloud's [2][n] array -- other curves'.
`start_run` holds the start points in the order the reference's run had them; a walk started from that list reproduces its paths.
(torch.topk(sorted=False) orders its output differently on a GPU, so there the reference itself walks other curves.)"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg            # noqa: E402
from seeded import seeded_params    # noqa: E402

TAU_FACTOR = 32.0
WALK_SHAPES = ((2, 128, 16, 20, 100, 5), (3, 256, 32, 20, 100, 5), (2, 64, 32, 8, 10, 30), (1, 72, 16, 20, 10, 5))    # B N C k curves length
GROUPING_SEED, AGGREGATION_SEED = 5200, 5300
NET_SEED_START, GRAD_SEED_START = 6000, 7000


def save(name, **arrs):
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"  {name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) < (1 << 20)


class Recorder:
    """Wraps the reference module's gumbel_softmax (logits of every step), batched_index_select (the point picked),
    Walk.forward (the start points) and CurveGrouping.forward (the start-point attention) while a model runs."""

    def __init__(self, cu):
        self.cu = cu
        self.walks = []

    def __enter__(self):
        cu, rec = self.cu, self
        self.saved = (cu.gumbel_softmax, cu.batched_index_select, cu.Walk.forward, cu.CurveGrouping.forward)
        gs, bis, wf, gf = self.saved

        def gumbel(logits, dim, temperature=1):
            rec.walks[-1]["logits"].append(logits.detach().clone())
            return gs(logits, dim, temperature)

        def select(input, dim, index):
            out = bis(input, dim, index)
            rec.walks[-1]["pick"].append(out.detach().clone().view(-1))
            return out

        def walk_forward(self_, xyz, x, adj, cur):
            rec.walks[-1].update(start=cur.detach().clone().view(x.shape[0], -1), N=x.shape[2], logits=[], pick=[])
            return wf(self_, xyz, x, adj, cur)

        def grouping_forward(self_, x, xyz, idx):
            rec.walks.append({"att": torch.sigmoid(self_.att(x)).detach().view(x.shape[0], -1)})
            return gf(self_, x, xyz, idx)
        cu.gumbel_softmax, cu.batched_index_select, cu.Walk.forward, cu.CurveGrouping.forward = gumbel, select, walk_forward, grouping_forward
        return self

    def __exit__(self, *exc):
        cu = self.cu
        cu.gumbel_softmax, cu.batched_index_select, cu.Walk.forward, cu.CurveGrouping.forward = self.saved
        return False

    def blocks(self):
        """per walk: start [B,n] ascending, path [B,n,L], logits [B,n,L,k], att [B,N], order [B,n] (the sort of the run's own order)"""
        out = []
        for wk in self.walks:
            start, N = wk["start"], wk["N"]
            B, n = start.shape
            order = torch.argsort(start, dim=1)
            logits = torch.stack([l.view(B, n, -1) for l in wk["logits"]], dim=2)                         # B, n, L, k
            path = torch.stack([p.view(B, n) for p in wk["pick"]], dim=2) - (torch.arange(B) * N).view(B, 1, 1)
            take = lambda t: torch.gather(t, 1, order.view(B, n, *[1] * (t.dim() - 2)).expand_as(t))
            out.append({"start": take(start), "path": take(path), "logits": take(logits), "att": wk["att"], "order": order, "start_run": start})
        return out


def judge(b32, b64, what, all_clear=False, in_net=False):
    """tau, per-curve margins and the asserted conditions for one walk run in fp32 (b32) and fp64 (b64).  Returns (tau, margin
    [B,n], number of curves at or below tau), or None when all_clear is asked for and a curve does not clear tau.  in_net (a block
    inside the classifier, whose tests hand the walk the stored start list): None unless the two runs start from the same list, walk
    identical paths and leave at most 5 % of the curves at or below tau; the selection gap is printed, not required."""
    if in_net and not torch.equal(b32["start_run"], b64["start_run"]):
        print(f"  {what}: the fp32 and fp64 runs start from different lists")
        return None
    assert torch.equal(b32["start"], b64["start"]), what + ": the fp32 and fp64 runs select different start points"
    assert torch.equal(b32["start_run"], b64["start_run"]), what + ": the fp32 and fp64 runs order their start points differently"
    same = (b32["path"] == b64["path"]).long()
    reached = torch.cat((torch.ones_like(same[:, :, :1]), torch.cumprod(same, dim=2)[:, :, :-1]), dim=2).bool()    # both runs stood on the same point
    diff = (b32["logits"].double() - b64["logits"]).abs()
    tau = TAU_FACTOR * float(diff[reached].max())
    top2 = b64["logits"].topk(2, dim=-1)[0]
    margins = top2[..., 0] - top2[..., 1]
    assert float(margins.min()) > 0, what + ": two logits tie exactly"
    margin = margins.min(dim=2)[0]
    low = int((margin <= tau).sum())
    n, N = b64["start"].shape[1], b64["att"].shape[1]
    gap = np.inf
    if n < N:
        s = b64["att"].sort(dim=1, descending=True)[0]
        gap = float((s[:, n - 1] - s[:, n]).min())
    agree = bool(torch.equal(b32["path"], b64["path"]))
    print(f"  {what}: tau {tau:.2e}, smallest margin {float(margin.min()):.2e}, curves at or below tau {low} of {margin.numel()}, "
          f"selection gap {gap:.2e}, fp32 and fp64 paths identical: {agree}")
    if all_clear and (low > 0 or gap <= tau):
        return None
    if in_net:
        return (tau, margin, low) if agree and low <= 0.05 * margin.numel() else None
    assert low <= 0.05 * margin.numel(), what + ": more than 5 % of the curves are at or below tau"
    assert gap > tau, what + ": the start-point selection is within tau"
    return tau, margin, low


def main():
    torch.set_num_threads(4)
    mg.import_reference()
    from learning3d.utils import curvenet_util as cu
    from learning3d.utils.model_common_utils import knn
    from learning3d.models import CurveNet
    gen = torch.Generator().manual_seed(20261)

    # ---- the walk alone (CurveGrouping) and the aggregation behind it, at four shapes
    arrs = {"shapes": np.array(WALK_SHAPES)}
    for si, (B, N, C, k, cn, cl) in enumerate(WALK_SHAPES):
        x = torch.randn(B, C, N, generator=gen)
        xyz = torch.rand(B, 3, N, generator=gen) * 2 - 1
        idx = knn(xyz, k, add_one_to_k=True)[:, :, 1:].contiguous()
        res = {}
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            grp = seeded_params(cu.CurveGrouping(C, k, cn, cl), GROUPING_SEED + si).eval().to(dtype)
            agg = seeded_params(cu.CurveAggregation(C), AGGREGATION_SEED + si).eval().to(dtype)
            with Recorder(cu) as rec, torch.no_grad():
                curves = grp(x.to(dtype), xyz.to(dtype), idx)
                out = agg(x.to(dtype), curves)
            blk = rec.blocks()[0]
            order = blk["order"]
            blk["curves"] = torch.gather(curves, 2, order.view(B, 1, cn, 1).expand_as(curves))          # keyed by start index
            blk["agg"] = out
            res[tag] = blk
        tau, margin, _ = judge(res["f32"], res["f64"], f"walk shape {si} {WALK_SHAPES[si]}")
        p = f"s{si}."
        arrs.update({p + "x": x, p + "xyz": xyz, p + "idx": idx, p + "start": res["f64"]["start"], p + "start_run": res["f64"]["start_run"], p + "tau": tau, p + "margin": margin,
                     p + "f64.path": res["f64"]["path"].to(torch.int32), p + "f32.path": res["f32"]["path"].to(torch.int32),
                     p + "f64.curves": res["f64"]["curves"], p + "f32.curves": res["f32"]["curves"],
                     p + "f64.agg": res["f64"]["agg"], p + "f32.agg": res["f32"]["agg"]})
    cic = cu.CIC(npoint=128, radius=0.05, k=20, in_channels=32, output_channels=64, bottleneck_ratio=2, mlp_num=1, curve_config=[100, 5])
    arrs["cic_keys"] = np.array(list(cic.state_dict().keys()))
    arrs["grouping_keys"] = np.array(list(cu.CurveGrouping(16, 20, 100, 5).state_dict().keys()))
    arrs["curvenet_keys"] = np.array(list(CurveNet(num_classes=40, k=20, setting='default').state_dict().keys()))
    arrs["aggregation_keys"] = np.array(list(cu.CurveAggregation(16).state_dict().keys()))
    save("curve_walk", **arrs)

    # ---- one CIC block at the first walk shape, train-mode autograd
    B, N, C, k, cn, cl = WALK_SHAPES[0]
    feat = torch.randn(B, 2 * C, N, generator=gen)
    xyz = torch.rand(B, 3, N, generator=gen) * 2 - 1
    for seed in range(GRAD_SEED_START, GRAD_SEED_START + 200):
        res = {}
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            blk = seeded_params(cu.CIC(npoint=N, radius=0.05, k=k, in_channels=2 * C, output_channels=64, bottleneck_ratio=2, mlp_num=1,
                                       curve_config=[cn, cl]), seed).train().to(dtype)
            torch.set_default_dtype(dtype)         # the reference builds index offsets and distances in the default dtype
            with Recorder(cu) as rec:
                _, out = blk(xyz.to(dtype), feat.to(dtype))
                loss = (out ** 2).mean()
                loss.backward()
            torch.set_default_dtype(torch.float32)
            res[tag] = (loss.detach(), blk.conv1[0].weight.grad, blk.curvegrouping.walk.agent_mlp[0].weight.grad, rec.blocks()[0], out.detach())
        v = judge(res["f32"][3], res["f64"][3], f"CIC gradient seed {seed}", all_clear=True)
        if v is not None:
            break
    else:
        raise AssertionError("no weight seed lets every curve clear tau")
    arrs = {"x": feat, "xyz": xyz, "seed": seed, "tau": v[0]}
    for tag in ("f32", "f64"):
        arrs.update({tag + ".loss": res[tag][0], tag + ".grad_conv1": res[tag][1], tag + ".grad_agent": res[tag][2], tag + ".out": res[tag][4],
                     tag + ".path": res[tag][3]["path"].to(torch.int32)})
    arrs["start"] = res["f64"][3]["start"].to(torch.int32)
    save("curvenet_grad", **arrs)

    # ---- the whole classifier, setting 'default', B 2, N 1024 (the reference hard-codes npoint = 1024 in stages 1-2)
    cloud = torch.rand(2, 1024, 3, generator=gen) * 2 - 1
    cloud = cloud / cloud.norm(dim=2).max(dim=1)[0].view(2, 1, 1)
    for seed in range(NET_SEED_START, NET_SEED_START + 2000):
        res = {}
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            net = seeded_params(CurveNet(num_classes=40, k=20, setting='default'), seed).eval().to(dtype)
            torch.set_default_dtype(dtype)         # the reference's farthest_point_sample makes its distances with torch.ones(): the default dtype
            with Recorder(cu) as rec, torch.no_grad():
                logits = net(cloud.to(dtype))
            torch.set_default_dtype(torch.float32)
            res[tag] = (logits, rec.blocks())
        verdicts = [judge(a, b, f"CurveNet seed {seed} walk {i}", in_net=True) for i, (a, b) in enumerate(zip(res["f32"][1], res["f64"][1]))]
        if all(v is not None for v in verdicts):
            break
    else:
        raise AssertionError("no weight seed meets the per-block rule")
    assert len(verdicts) == 4
    arrs = {"input": cloud, "seed": seed, "f32.logits": res["f32"][0], "f64.logits": res["f64"][0]}
    for i, (v, blk) in enumerate(zip(verdicts, res["f64"][1])):
        arrs.update({f"w{i}.start_run": blk["start_run"].to(torch.int32), f"w{i}.start": blk["start"].to(torch.int32),
                     f"w{i}.path": blk["path"].to(torch.int32), f"w{i}.margin": v[1], f"w{i}.tau": v[0]})
    print("  CurveNet seed", seed, "logit gap fp32 / fp64", float((res["f32"][0].double() - res["f64"][0]).abs().max()))
    save("curvenet_seeded", **arrs)


if __name__ == "__main__":
    main()
