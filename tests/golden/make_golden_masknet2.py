"""Fixture of MaskNet2, from the REFERENCE on the CPU:

    python tests/golden/make_golden_masknet2.py

Needs the reference checkout make_golden.py reads.  Writes masknet2_seeded.npz next to this file: arrays and lists of names only.
Every mask is stored twice, computed in fp32 and in fp64 (`net.double()` of the same weights).

Weights: seeded_params(net, seed); every 3-d tensor of the state (the conv weights) times WEIGHT_FACTOR; every `beta` set to BETA
(the reference initialises them to 0, which switches all eight attention layers off); the final bias moved by minus the median fp64
template logit, so that the 0.5 threshold cuts through the cloud (the value is stored, `bias`).  With factor 1 the masks are flat
within 0.003 and the last layer's |energy| stays under 13, which tests nothing; factor 2 with beta >= 0.5 saturates every mask to 1.
The tests rebuild the weights from the stored seed, factor, beta and bias, and hold their key list against the stored one.

Clouds: template and source are two random N-subsets of one parent cloud of 3N/2 points, U(-1,1)^3.

Per case: both masks, gap = max |mask32 - mask64| per mask, tau = 32 gap (room for another summation order), the sorted fp64 index
sets of mask > 0.5, and the largest |energy| of the last Self_Attn layer.  Asserted here, the seed being stepped until all hold: each
mask spans at least 0.05; the largest last-layer |energy| lies in [30, 1000] (the unscaled logits are large, and still far from
fp32's range); gap > 0; at most 5 % of a cloud's points lie within tau of 0.5; the fp32 and fp64 sets agree outside that band.
Case `c` (B 1) goes through the reference's MaskNet2.forward, whose masked clouds must be the clouds at the stored sets."""
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
WEIGHT_FACTOR = 2.0
BETA = 0.1
SEED_START = 8100
CASES = (("a", 2, 256, "maskNet"), ("b", 2, 200, "maskNet"), ("c", 1, 256, "forward"))


def prepared(net, seed):
    seeded_params(net, seed)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            if v.dim() == 3:
                v.mul_(WEIGHT_FACTOR)
            if k.endswith(".beta"):
                v.fill_(BETA)
    return net


def clouds(seed, B, N):
    g = torch.Generator().manual_seed(seed)
    parent = torch.rand((B, 3 * N // 2, 3), generator=g) * 2 - 1
    pick = lambda: torch.stack([parent[b][torch.randperm(parent.shape[1], generator=g)[:N]] for b in range(B)])      # noqa: E731
    return pick(), pick()


def case(M2, seed, B, N, mode):
    """-> (dict of arrays, state keys), or None when one of the fixture's conditions fails for this seed"""
    net = prepared(M2.MaskNet2(feature_model=M2.PointNet(use_bn=True), is_training=False), seed).eval()
    template, source = clouds(seed + 500, B, N)
    last = net.maskNet.h3[3]
    seen, energy = [], []
    net64 = copy.deepcopy(net).double()
    hooks = [net64.maskNet.h3[3].register_forward_hook(lambda m, i, o: seen.append(o.detach())),
             net64.maskNet.feature_model.conv5.query_conv.register_forward_hook(
                 lambda m, i, o: energy.append(float(torch.bmm(o.permute(0, 2, 1), o).abs().max())))]
    with torch.no_grad():
        net64.maskNet(template.double(), source.double())
    for h in hooks:
        h.remove()
    with torch.no_grad():
        last.bias.sub_(float(seen[0].reshape(-1).median()))              # seen[0]: the template's logits (find_mask runs them first)
    bias = float(last.bias.detach()[0])
    net64 = copy.deepcopy(net).double()
    with torch.no_grad():
        if mode == "forward":
            mt32, ms32, t32, s32 = net(template, source)
            mt64, ms64, t64, s64 = net64(template.double(), source.double())
        else:
            t32, s32 = net.maskNet(template, source)
            t64, s64 = net64.maskNet(template.double(), source.double())
    out = dict(seed=seed, template=template, source=source, bias=bias, energy=max(energy))
    ok = 30.0 <= max(energy) <= 1000.0
    note = []
    for name, m32, m64 in (("t", t32, t64), ("s", s32, s64)):
        gap = float((m32.double() - m64).abs().max())
        tau = TAU_FACTOR * gap
        near = (m64 - 0.5).abs() <= tau
        worst = float(near.double().mean(dim=1).max())
        span = float((m64.max(dim=1)[0] - m64.min(dim=1)[0]).min())
        sets_agree = all(torch.equal((m32[b].double() > 0.5)[~near[b]], (m64[b] > 0.5)[~near[b]]) for b in range(B))
        counts = [int((m64[b] > 0.5).sum()) for b in range(B)]
        note.append(f"{name}: {float(m64.min()):.3f} .. {float(m64.max()):.3f} span {span:.3f} gap {gap:.2e} near {100 * worst:.2f} % counts {counts}")
        ok = ok and span >= 0.05 and gap > 0 and worst <= 0.05 and sets_agree and all(0 < c < N for c in counts)
        out.update({f"{name}_mask32": m32, f"{name}_mask64": m64, f"{name}_gap": gap, f"{name}_tau": tau})
        if mode == "forward":
            idx = torch.nonzero(m64[0] > 0.5).reshape(1, -1)
            out[f"{name}_idx64"] = idx
    print(f"  seed {seed} {(B, N)} {mode}: last-layer |energy| {max(energy):.1f}; " + "; ".join(note) + ("" if ok else "  -- next seed"))
    if not ok:
        return None
    if mode == "forward":
        assert torch.equal(mt64, template.double()[:, out["t_idx64"][0]]) and torch.equal(ms64, source.double()[:, out["s_idx64"][0]])
    return out, list(net.state_dict().keys())


def main():
    torch.set_num_threads(4)
    mg.import_reference()
    import learning3d.models.masknet2 as M2
    out, keys, seed = {}, None, SEED_START
    for name, B, N, mode in CASES:
        while True:
            got = case(M2, seed, B, N, mode)
            seed += 1
            if got is not None:
                break
        arrs, keys = got
        out.update({f"{name}_{k}": v for k, v in arrs.items()})
    assert len(keys) == 76
    out["cases"] = np.array([c[0] for c in CASES])
    out["state_keys"] = np.array(keys)
    out["weight_factor"] = WEIGHT_FACTOR
    out["beta"] = BETA
    arrs = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, "masknet2_seeded.npz")
    np.savez_compressed(path, **arrs)
    print(f"  masknet2_seeded.npz  {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
