"""Fixtures of MaskNet and Segmentation, from the REFERENCE on the CPU:

    python tests/golden/make_golden_masknet.py

Needs the reference checkout make_golden.py reads.  Writes, next to this file, masknet_seeded.npz and segmentation_seeded.npz:
arrays and lists of names only.  Every result is stored twice, computed in fp32 and in fp64 (`net.double()` of the same weights).

Weights: seeded_params(net, seed), then every 3-d tensor of the state (the conv weights) times 2.45.  Without the factor the
ten ReLU layers shrink the signal until every mask value of a cloud lies within 6e-5 of the others and 6-22 % of the points sit within
32 x the fp32-to-fp64 gap of the top-k boundary; with it the masks span 0.18-0.94 and under 1 % do.  The tests rebuild the weights
from the stored seed with the same two steps (a MaskNet's state is 14 MB), and hold their key list against the stored one.

Clouds: template U(-1,1)^3, source = a random Ns-subset of the template's points.

Per case: gap = max |mask32 - mask64|, tau = 32 gap (room for another summation order), the boundary of every cloud (the midpoint
of its k-th and (k+1)-th largest fp64 values; 0.5 in threshold mode) and the sorted fp64 index sets.  Asserted here: at most 5 % of a
cloud's points lie within tau of its boundary (the seed is stepped until that holds), and the fp32 and fp64 sets agree outside that
band.  In threshold mode the seeded final bias decides all or nothing (count 0 or Nt), so h3.8.bias is moved by minus the median
fp64 logit of the cloud; the value is stored (`bias`)."""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg            # noqa: E402
from seeded import seeded_params    # noqa: E402

TAU_FACTOR = 32.0
WEIGHT_FACTOR = 2.45
SEED_START = 8000
MASK_CASES = (("a", 2, 256, 192, "topk"), ("b", 2, 512, 256, "topk"), ("c", 2, 200, 150, "topk"), ("d", 1, 256, 128, "threshold"))
SEG_CASES = (("bn_256", True, 2, 256), ("bn_200", True, 2, 200), ("plain_256", False, 2, 256), ("plain_200", False, 2, 200))
SEG_CLASSES = 5


def scaled_seeded_params(net, seed):
    seeded_params(net, seed)
    with torch.no_grad():
        for v in net.state_dict().values():
            if v.dim() == 3:
                v.mul_(WEIGHT_FACTOR)
    return net


def clouds(seed, B, Nt, Ns):
    g = torch.Generator().manual_seed(seed)
    template = torch.rand((B, Nt, 3), generator=g) * 2 - 1
    source = torch.stack([template[b][torch.randperm(Nt, generator=g)[:Ns]] for b in range(B)])
    return template, source


def mask_case(Mo, seed, B, Nt, Ns, mode):
    """-> dict of arrays, or None when more than 5 % of a cloud's points are within tau of its boundary"""
    net = scaled_seeded_params(Mo.MaskNet(feature_model=Mo.PointNet(use_bn=True), is_training=False), seed).eval()
    template, source = clouds(seed + 500, B, Nt, Ns)
    bias = float(net.maskNet.h3[8].bias.detach()[0])
    if mode == "threshold":
        seen = []
        net64 = copy.deepcopy(net).double()
        hook = net64.maskNet.h3[8].register_forward_hook(lambda m, i, o: seen.append(o.detach()))
        with torch.no_grad():
            net64(template.double(), source.double(), "topk")
        hook.remove()
        with torch.no_grad():
            net.maskNet.h3[8].bias.sub_(float(seen[0][0].reshape(-1).median()))
        bias = float(net.maskNet.h3[8].bias.detach()[0])
    net64 = copy.deepcopy(net).double()
    with torch.no_grad():
        _, m32 = net(template, source, mode)
        _, m64 = net64(template.double(), source.double(), mode)
    gap = float((m32.double() - m64).abs().max())
    tau = TAU_FACTOR * gap
    if mode == "topk":
        s = m64.sort(dim=1, descending=True)[0]
        boundary = 0.5 * (s[:, Ns - 1] + s[:, Ns])
    else:
        boundary = torch.full((B,), 0.5, dtype=torch.float64)
    near = (m64 - boundary[:, None]).abs() <= tau
    worst = float(near.double().mean(dim=1).max())
    sets64 = [torch.nonzero(m64[b] > boundary[b]).reshape(-1) for b in range(B)]
    sets32 = [torch.nonzero(m32[b].double() > boundary[b]).reshape(-1) for b in range(B)]
    print(f"  seed {seed} {(B, Nt, Ns)} {mode}: masks {float(m64.min()):.3f} .. {float(m64.max()):.3f}, gap {gap:.2e}, tau {tau:.2e}, "
          f"within tau of the boundary at most {100 * worst:.2f} % of a cloud, counts {[len(s) for s in sets64]}")
    if worst > 0.05:
        return None
    for b in range(B):
        far = ~near[b]
        assert torch.equal((m32[b].double() > boundary[b])[far], (m64[b] > boundary[b])[far]), "fp32 and fp64 sets differ outside the band"
        if mode == "topk":
            assert len(sets64[b]) == Ns
    if mode == "topk":
        idx64 = torch.stack(sets64)
    else:
        assert 0 < len(sets64[0]) < Nt
        idx64 = sets64[0].reshape(1, -1)
    return dict(seed=seed, template=template, source=source, mask32=m32, mask64=m64, gap=gap, tau=tau, boundary=boundary, idx64=idx64,
                idx32=torch.stack(sets32) if mode == "topk" else sets32[0].reshape(1, -1), bias=bias,
                threshold_mode=int(mode == "threshold")), list(net.state_dict().keys())


def main():
    torch.set_num_threads(4)
    _, _, Mo, _ = mg.import_reference()
    out, keys = {}, None
    seed = SEED_START
    for name, B, Nt, Ns, mode in MASK_CASES:
        while True:
            got = mask_case(Mo, seed, B, Nt, Ns, mode)
            seed += 1
            if got is not None:
                break
        arrs, keys = got
        out.update({f"{name}_{k}": v for k, v in arrs.items()})
    out["cases"] = np.array([c[0] for c in MASK_CASES])
    out["state_keys"] = np.array(keys)
    out["weight_factor"] = WEIGHT_FACTOR
    save("masknet_seeded", **out)

    out = {}
    for i, (name, use_bn, B, N) in enumerate(SEG_CASES):
        seed = SEED_START + 100 + i
        net = scaled_seeded_params(Mo.Segmentation(Mo.PointNet(global_feat=False, use_bn=use_bn), num_classes=SEG_CLASSES), seed).eval()
        x = torch.rand((B, N, 3), generator=torch.Generator().manual_seed(seed + 500)) * 2 - 1
        with torch.no_grad():
            y32 = net(x)
            y64 = copy.deepcopy(net).double()(x.double())
        gap = float((y32.double() - y64).abs().max())
        print(f"  segmentation {name}: logits {float(y64.min()):.3f} .. {float(y64.max()):.3f}, gap {gap:.2e}")
        out.update({f"{name}_seed": seed, f"{name}_x": x, f"{name}_out32": y32, f"{name}_out64": y64, f"{name}_gap": gap,
                    f"{name}_use_bn": int(use_bn), f"{name}_state_keys": np.array(list(net.state_dict().keys()))})
    out["cases"] = np.array([c[0] for c in SEG_CASES])
    out["num_classes"] = SEG_CLASSES
    out["weight_factor"] = WEIGHT_FACTOR
    save("segmentation_seeded", **out)


def save(name, **arrs):
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"  {name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
