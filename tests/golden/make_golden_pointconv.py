"""Fixture of the PointConv network and its set-abstraction layers, from the REFERENCE on the CPU:

    python tests/golden/make_golden_pointconv.py

Needs the reference checkout make_golden.py reads.  Writes pointconv_seeded.npz next to this file: arrays and lists of names only.
It calls the reference's own classes and copies none of its code: models.pointconv.PointConvDensityClsSsg and
utils.pointconv_util.PointConvDensitySetAbstraction / PointConvSetAbstraction.  Everything is run in fp32 and in fp64
(`copy.deepcopy(net).double()`, the same fp32 inputs cast up, inside torch.set_default_dtype(torch.float64) because the
reference's farthest_point_sample builds its distances in the default dtype).  Per quantity: the fp64 value and
gap = max |fp32 - fp64|.  Tensors of more than 4096 values are stored as `<name>_s64`, the flattened fp64 tensor at flat[::stride],
stride = ceil(numel / 2048), beside their gap; the tests rebuild the whole fp64 tensors with this package's op sequence in fp64
on the CPU, which tests/test_pointconv_cpu.py first holds to 1e-9 against everything stored here.  Weights come from
seeded_params and are not stored.

Rescaling (pointconv_fixture.rescale, applied to every seeded model here and in the tests): every Conv2d weight times
CONV_FACTOR = 2.0, because U(+-1/sqrt(fan_in)) weights shrink the signal layer by layer until the outputs are their biases; the
last DensityNet BatchNorm's bias set to DN_BIAS = 0.5, because a one-channel BatchNorm + ReLU with the seeded U(+-0.1) bias can
die on every neighbour.

Cases (pointconv_fixture.MODEL_CASES, LAYER_CASES).  Whole model at B 2, N 1024, points uniform in [-0.5,0.5]^3 with unit normals:
m1 input_channel_dim 3, embedding only; m2 input_channel_dim 6 with the classifier.  Layers: d0-d3 PointConvDensitySetAbstraction
(N 96 S 24 K 5 mlp [16,32]; N 70 S 70 K 16 points=None; group_all N 37 mlp [32,48]; group_all N 200 points=None mlp [16]),
p0, p1 PointConvSetAbstraction (N 96 S 24 K 5; group_all N 37).  One backward, of d0: the gradients of
sum(out * loss_weights) with respect to every parameter, per parameter the fp64 value and the gap.
The state_dict key lists and shapes of both model variants.

The seed is stepped until all of these hold, and what was found is printed:
  * FPS: the reference's indices are equal in fp32 and fp64 in every layer of every case;
  * kNN: the reference's neighbour sets are equal in fp32 and fp64 in every layer of every case, and the K-th and (K+1)-th
    expanded squared distances of every centre are at least 32 * 2^-24 * (|p|^2 + |q|^2) apart (the larger of the two pairs'),
    so this package's kernels group the same neighbours;
  * DensityNet alive: in every layer its output is positive on at least 25 % of the (centre, neighbour) pairs and spans at least
    5 % of its maximum;
  * layer output alive: at least 25 % of every set-abstraction layer's output is greater than 0;
  * every stored gap is greater than 0."""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg            # noqa: E402
import pointconv_fixture as pf      # noqa: E402

SEED_START = 5200
MAX_SEEDS = 200         # most seeds fall at the geometry-only screen, which costs a second
MARGIN = 32.0 * 2.0 ** -24
WHOLE = 4096


def both(fn32, fn64):
    with torch.no_grad():
        r32 = fn32()
        torch.set_default_dtype(torch.float64)
        try:
            r64 = fn64()
        finally:
            torch.set_default_dtype(torch.float32)
    return r32, r64


class Recorder:
    """records what the reference's farthest_point_sample and knn_point return, and what every DensityNet returns"""

    def __init__(self, PU):
        self.PU, self.fps, self.knn, self.dens = PU, [], [], []
        self.orig = (PU.farthest_point_sample, PU.knn_point, PU.DensityNet.forward)

    def __enter__(self):
        fps0, knn0, dn0 = self.orig
        rec = self

        def fps(xyz, npoint):
            out = fps0(xyz, npoint)
            rec.fps.append(out.clone())
            return out

        def knn(nsample, xyz, new_xyz):
            out = knn0(nsample, xyz, new_xyz)
            rec.knn.append((out.sort(dim=-1)[0], xyz.detach().double(), new_xyz.detach().double(), nsample))
            return out

        def dn(module, x):
            out = dn0(module, x)
            rec.dens.append(out.detach().double())
            return out
        self.PU.farthest_point_sample, self.PU.knn_point, self.PU.DensityNet.forward = fps, knn, dn
        return self

    def __exit__(self, *exc):
        self.PU.farthest_point_sample, self.PU.knn_point, self.PU.DensityNet.forward = self.orig
        return False


def knn_margin(xyz, new_xyz, K):
    """the smallest (d[K] - d[K-1]) / (|p|^2 + |q|^2) over the centres, in fp64 on the expanded form"""
    n2, q2 = (xyz ** 2).sum(-1), (new_xyz ** 2).sum(-1)
    d = q2[:, :, None] + n2[:, None, :] - 2 * new_xyz @ xyz.transpose(1, 2)
    if K >= xyz.shape[1]:
        return float("inf")
    ds, ix = d.sort(dim=-1)
    scale = q2[:, :, None] + torch.gather(n2[:, None, :].expand_as(d), 2, ix[:, :, K - 1:K + 1])
    return float(((ds[:, :, K] - ds[:, :, K - 1]) / scale.max(dim=-1)[0]).min())


def geometry_ok(r32, r64, notes, what):
    ok = len(r32.fps) == len(r64.fps) and all(torch.equal(a, b) for a, b in zip(r32.fps, r64.fps))
    ok_knn = all(torch.equal(a[0], b[0]) for a, b in zip(r32.knn, r64.knn))
    margin = min([knn_margin(x, q, K) for _, x, q, K in r64.knn] or [float("inf")])
    alive = []
    for d in r64.dens:
        alive.append((float((d > 0).double().mean()), float((d.max() - d.min()) / d.max()) if float(d.max()) > 0 else 0.0))
    ok_d = all(p >= 0.25 and s >= 0.05 for p, s in alive)
    notes.append(f"{what}: FPS equal {ok}, kNN sets equal {ok_knn}, smallest kNN margin {margin / MARGIN:.1f} x the bar, DensityNet "
                 "(positive share, span) " + " ".join(f"({p:.2f}, {s:.2f})" for p, s in alive))
    return ok and ok_knn and margin >= MARGIN and ok_d


def put(out, key, v32, v64):
    v32, v64 = torch.as_tensor(v32), torch.as_tensor(v64)
    g = float((v32.double() - v64).abs().max())
    out[key + "_gap"] = g
    if v64.numel() > WHOLE:
        out[key + "_s64"] = pf.sampled(v64).clone()
    else:
        out[key + "_64"] = v64
    return g


def prescreen(seed):
    """the whole-model clouds' geometry without the network: FPS in fp32 and fp64 and the kNN margins of sa1 and sa2"""
    from learning3d_amd.utils import pointconv_util as mine
    xyz = pf.model_cloud(seed)[:, :, :3].contiguous()
    worst = float("inf")
    for S, K in ((512, 32), (128, 64)):
        f32, f64 = mine._t_farthest_point_sample(xyz, S), mine._t_farthest_point_sample(xyz.double(), S)
        if not torch.equal(f32, f64):
            return 0.0
        new = mine._t_index_points(xyz, f32)
        worst = min(worst, knn_margin(xyz.double(), new.double(), K))
        xyz = new
    return worst


def main():
    torch.set_num_threads(8)
    mg.import_reference()
    import learning3d.models.pointconv as Pm
    import learning3d.utils.pointconv_util as PU
    seed = SEED_START
    while True:
        out, notes, ok = {}, [], True
        m = prescreen(seed)
        notes.append(f"seed {seed}: whole-model kNN margin {m / MARGIN:.1f} x the bar (geometry only)")
        ok = m >= MARGIN
        if ok:
            for name, _, _, _, _, _, _, _, group_all in pf.LAYER_CASES:
                net = pf.build_layer(PU, name, seed)
                net64 = copy.deepcopy(net).double()
                xyz, pts = pf.layer_inputs(name, seed)
                with Recorder(PU) as r32:
                    o32 = net(xyz, pts)
                torch.set_default_dtype(torch.float64)
                try:
                    with Recorder(PU) as r64:
                        o64 = net64(xyz.double(), None if pts is None else pts.double())
                finally:
                    torch.set_default_dtype(torch.float32)
                ok = geometry_ok(r32, r64, notes, f"layer {name}") and ok
                if group_all:
                    g1 = put(out, f"{name}_xyz", o32[0].detach(), o64[0].detach())      # the cloud's mean
                else:
                    g1, out[f"{name}_xyz_64"] = 0.0, o64[0].detach()                    # a selection of input points: exact, no gap
                    assert torch.equal(o32[0].double(), o64[0])
                g2 = put(out, f"{name}_points", o32[1].detach(), o64[1].detach())
                share = float((o64[1] > 0).double().mean())
                notes.append(f"layer {name}: gaps xyz {g1:.1e} points {g2:.1e}, output > 0 on {share:.2f}, |out| max {float(o64[1].abs().max()):.2f}")
                ok = ok and share >= 0.25 and g2 > 0 and (g1 > 0 or not group_all)
                if name == pf.BACKWARD_CASE:
                    wts = pf.loss_weights(o32[1].shape, seed)
                    (o32[1] * wts).sum().backward()
                    (o64[1] * wts.double()).sum().backward()
                    names = [k for k, p in net.named_parameters()]
                    for (k, p), (_, p64) in zip(net.named_parameters(), net64.named_parameters()):
                        g = put(out, f"grad_{k}", p.grad, p64.grad)
                        ok = ok and g > 0
                    out["grad_names"] = np.array(names)
                    notes.append("backward of " + name + ": gaps " + " ".join(f"{out[f'grad_{k}_gap']:.1e}" for k in names))
                if not ok:
                    break
        if ok:
            cloud = pf.model_cloud(seed)
            for name, dim, classifier in pf.MODEL_CASES:
                net = pf.build_model(Pm.PointConvDensityClsSsg, name, seed)
                net64 = copy.deepcopy(net).double()
                x = cloud[:, :, :dim].contiguous()
                with Recorder(PU) as r32, torch.no_grad():
                    o32 = pf.run_model(net, x)
                torch.set_default_dtype(torch.float64)
                try:
                    with Recorder(PU) as r64, torch.no_grad():
                        o64 = pf.run_model(net64, x.double())
                finally:
                    torch.set_default_dtype(torch.float32)
                ok = geometry_ok(r32, r64, notes, f"model {name}") and ok
                for q in pf.MODEL_QUANTITIES:
                    if q in o64:
                        g = put(out, f"{name}_{q}", o32[q], o64[q])
                        share = float((o64[q] > 0).double().mean())
                        notes.append(f"model {name} {q}: gap {g:.1e}, > 0 on {share:.2f}, |.| max {float(o64[q].abs().max()):.2f}")
                        ok = ok and g > 0 and (q == "logp" or share >= 0.25)
                if classifier:
                    same = torch.equal(o32["logp"].argmax(-1), o64["logp"].argmax(-1))
                    top = o64["logp"].topk(2, dim=-1)[0]
                    notes.append(f"model {name}: arg-max equal in fp32 and fp64 {same}, top-2 log-probability distance {float((top[:, 0] - top[:, 1]).min()):.2e}")
                    ok = ok and same and float((top[:, 0] - top[:, 1]).min()) > 100 * out[f"{name}_logp_gap"]
                out[f"{name}_state_keys"] = np.array(list(net.state_dict().keys()))
                out[f"{name}_state_shapes"] = np.array([str(tuple(v.shape)) for v in net.state_dict().values()])
                if not ok:
                    break
        print("\n".join("  " + n for n in notes) + ("" if ok else "\n  -- next seed"), flush=True)
        if ok:
            break
        seed += 1
        assert seed < SEED_START + MAX_SEEDS, "no seed met the conditions"
    out.update(seed=seed, cloud=pf.model_cloud(seed), conv_factor=pf.CONV_FACTOR, dn_bias=pf.DN_BIAS,
               model_cases=np.array([c[0] for c in pf.MODEL_CASES]), layer_cases=np.array([c[0] for c in pf.LAYER_CASES]))
    arrs = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, "pointconv_seeded.npz")
    np.savez_compressed(path, **arrs)
    print(f"  pointconv_seeded.npz  {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
