"""Fixture of PRNet, from the REFERENCE on the CPU:

    python tests/golden/make_golden_prnet.py

Needs the reference checkout make_golden.py reads.  Writes prnet_seeded.npz next to this file: arrays and lists of names only.  It
calls the reference's own classes (models.prnet.PRNet and what it is made of) and copies none of their code.  Weights come from
seeded_params and are not stored.

The reference cannot run its forward in fp64 (its head and loop build float32 constants), so per case and quantity:
  * temperature, disparity, emb_k_src (iteration 0) and temperature_it<i> (every iteration): `_64` is the reference's own
    predict_embedding in fp64 -- for iteration i > 0 on the source cloud this package's fp64 op sequence has transformed so far;
  * R_ab0, t_ab0, R_ba0, t_ba0 (the head in iteration 0), est_R, est_t, transformed_source, loss: `_64` is this package's CPU op
    sequence in fp64, which tests/test_prnet_cpu.py holds to 1e-9 against the values of the first kind;
  * `_ref32` is the reference's fp32 value and `_gap` = max |_ref32 - _64|, for every quantity.  Tensors of more than 2048 values
    are stored as samples flat[::stride] (prnet_fixture.sampled); the gap is taken over the whole tensor.
One backward, of m4's loss (eval-mode BatchNorm, autograd on): per parameter that receives a gradient the reference's fp32 gradient,
this package's fp64 gradient and the gap.  The state_dict key lists and shapes of every case.

Rescaling and cases: prnet_fixture.rescale, prnet_fixture.CASES.

The seed is stepped (at most MAX_SEEDS) until, for every case and every iteration, all of these hold -- conditions on the inputs,
met by the reference alone -- and what was found is printed:
  * the reference's keypoint sets are equal in fp32 and fp64;
  * the K-th and (K+1)-th squared norms (fp64) differ by at least 32 * 2^-24 of the larger;
  * the feature-space kNN sets of every DGCNN layer are equal in fp32 and fp64 (the reference's `knn`, wrapped);
  * the temperature is strictly inside the clamp;
  * every H has (s2 + s3) >= 0.05 s1;
  * every stored gap is > 0."""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg            # noqa: E402
import prnet_fixture as pf          # noqa: E402

SEED_START = 7100
MAX_SEEDS = 200
MARGIN = 32.0 * 2.0 ** -24


class KnnRecorder:
    """records the neighbour sets the reference's `knn` returns (utils/model_common_utils.py; get_graph_feature calls it)"""

    def __init__(self, MCU):
        self.MCU, self.sets, self.orig = MCU, [], MCU.knn

    def __enter__(self):
        def knn(x, k, *a, **kw):
            out = self.orig(x, k, *a, **kw)
            self.sets.append(out.sort(dim=-1)[0])
            return out
        self.MCU.knn = knn
        return self

    def __exit__(self, *exc):
        self.MCU.knn = self.orig
        return False


def norm_margin(emb, K):
    """(k-th - (k+1)-th squared norm) / the larger, smallest over the clouds; emb [B,C,N] fp64"""
    sq = (emb ** 2).sum(dim=1).sort(dim=1, descending=True)[0]
    if K >= sq.shape[1]:
        return float("inf")
    return float(((sq[:, K - 1] - sq[:, K]) / sq[:, K - 1]).min())


def put(out, key, v32, v64):
    v32, v64 = torch.as_tensor(v32).detach(), torch.as_tensor(v64).detach()
    g = float((v32.double() - v64).abs().max())
    out[key + "_gap"] = g
    out[key + "_64"] = pf.sampled(v64).clone()
    out[key + "_ref32"] = pf.sampled(v32).clone()
    return g


def one_case(Pm, MCU, name, seed, out, notes):
    from learning3d_amd.models.prnet import PRNet as Mine
    _, (_, _, _, emb, N, K, iters, _, with_gt) = pf.case(name)
    src, tgt, Rab, tab = pf.clouds(name, seed)
    gt32 = (Rab, tab) if with_gt else (None, None)
    gt64 = tuple(None if t is None else t.double() for t in gt32)
    ref = pf.build_model(Pm.PRNet, name, seed)
    ref64 = copy.deepcopy(ref).double()
    mine64 = pf.build_model(Mine, name, seed).double()
    ok = True

    with torch.no_grad():
        with KnnRecorder(MCU) as k32:
            q32, h32 = pf.run(ref, name, src, tgt, *gt32)
        # this package's op sequence in fp64, recording the source cloud every iteration starts from
        starts, spam0 = [], mine64.spam
        mine64.spam = lambda s, t: (starts.append(s.clone()), spam0(s, t))[1]
        q64, h64 = pf.run(mine64, name, src.double(), tgt.double(), *gt64)
        # the reference's predict_embedding in fp64 on those clouds
        with KnnRecorder(MCU) as k64, pf.Hooks(ref64) as r64:
            for s in starts:
                ref64.predict_embedding(s, tgt.double().permute(0, 2, 1))
    e64 = r64.quantities()

    sets32, sets64 = h32.keypoint_sets(), r64.keypoint_sets()
    same_kp = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(sets32, sets64)) and len(sets32) == len(sets64)
    margin = min([min(norm_margin(a[2], K), norm_margin(a[3], K)) for a, _ in r64.kp] or [float("inf")])
    same_knn = len(k32.sets) == len(k64.sets) and all(torch.equal(a, b) for a, b in zip(k32.sets, k64.sets))
    temps = torch.cat([o[0].reshape(-1) for o in r64.temp] + [o[0].reshape(-1).double() for o in h32.temp])
    inside = bool((temps > 0.01).all() and (temps < 100.0).all())
    ratios = []
    for a, _ in h64.head:
        s = torch.linalg.svdvals(pf.head_H(*a))
        ratios.append(float(((s[:, 1] + s[:, 2]) / s[:, 0]).min()))
    notes.append(f"{name}: keypoint sets equal {same_kp}, norm margin {margin / MARGIN:.1f} x the bar, kNN sets equal {same_knn} "
                 f"({len(k32.sets)} graphs), temperature {float(temps.min()):.2f} .. {float(temps.max()):.2f}, "
                 f"(s2 + s3) / s1 >= {min(ratios):.3f}")
    ok = same_kp and margin >= MARGIN and same_knn and inside and min(ratios) >= 0.05

    gaps = []
    for q in pf.EMBED0 + tuple(f"temperature_it{i}" for i in range(iters)):
        if q32.get(q) is not None:
            gaps.append((q, put(out, f"{name}_{q}", q32[q], e64[q])))
    for q in pf.HEAD0 + pf.FINAL:
        if q in q32:
            gaps.append((q, put(out, f"{name}_{q}", q32[q], q64[q])))
    notes.append(f"{name}: gaps " + " ".join(f"{q} {g:.1e}" for q, g in gaps))
    ok = ok and all(g > 0 for _, g in gaps)
    if sets64:
        out[f"{name}_kp_src"], out[f"{name}_kp_tgt"] = sets64[0]
    out[f"{name}_state_keys"] = np.array(list(ref.state_dict().keys()))
    out[f"{name}_state_shapes"] = np.array([str(tuple(v.shape)) for v in ref.state_dict().values()])

    if ok and with_gt:
        # one backward of the loss: the reference in fp32, this package's op sequence in fp64
        mine64.spam = spam0
        ref.zero_grad()
        ref(src, tgt, *gt32)["loss"].backward()
        mine64(src.double(), tgt.double(), *gt64)["loss"].backward()
        p64 = dict(mine64.named_parameters())
        names = [k for k, p in ref.named_parameters() if p.grad is not None and p64[k].grad is not None and float(p.grad.abs().max()) > 0]
        gg = [put(out, f"grad_{k}", dict(ref.named_parameters())[k].grad, p64[k].grad) for k in names]
        out["grad_names"], out["grad_case"] = np.array(names), name
        notes.append(f"backward of {name}: {len(names)} parameters, gaps {min(gg):.1e} .. {max(gg):.1e}")
        ok = ok and all(g > 0 for g in gg)
    return ok


def main():
    torch.set_num_threads(8)
    mg.import_reference()
    import learning3d.models.prnet as Pm
    import learning3d.utils.model_common_utils as MCU
    seed = SEED_START
    while True:
        out, notes, ok = {}, [f"seed {seed}"], True
        for c in pf.CASES:
            ok = one_case(Pm, MCU, c[0], seed, out, notes)
            if not ok:
                break
        print("\n".join("  " + n for n in notes) + ("" if ok else "\n  -- next seed"), flush=True)
        if ok:
            break
        seed += 1
        assert seed < SEED_START + MAX_SEEDS, "no seed met the conditions"
    out.update(seed=seed, cases=np.array([c[0] for c in pf.CASES]), temp_bias=np.array([c[7] for c in pf.CASES]))
    arrs = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, "prnet_seeded.npz")
    np.savez_compressed(path, **arrs)
    print(f"  prnet_seeded.npz  {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
