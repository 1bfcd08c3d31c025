"""Fixture of DeepGMR, from the REFERENCE on the CPU:

    python tests/golden/make_golden_deepgmr.py

Needs the reference checkout make_golden.py reads.  Writes deepgmr_seeded.npz next to this file: arrays and lists of names only.
It calls the reference's own functions and copies none of its code: data_utils.dataloaders.get_rri per cloud; models.deepgmr.PointNet
with `deepgmr.args = Namespace(d_model=..., n_clusters=...)` set from outside (its constructor reads that undefined global);
gmm_params and gmm_register composed as DeepGMR.forward composes them (:134-151; the forward itself reads undefined names).
Everything is computed twice, in fp32 and in fp64 (`net.double()` of the same weights, the same fp32 clouds cast up; the fp64 run
of gmm_register inside torch.set_default_dtype(torch.float64), because it builds its constants in the default dtype).

Weights: seeded_params(net, seed), then every 3-d tensor of the state (the conv weights) times a weight factor.  With factor 1
gamma is flat, Ms nearly singular and the reference's own fp32 T is 6e-3 from fp64, which tests nothing; with factor 3 components
can come out empty.  Seed and factor are stepped (factor through FACTORS, then the next seed) until, for the case,
  * T's fp32-to-fp64 gap is <= 1e-4 (both T), every pi >= 1e-3, gamma spans at least 0.2 per cloud,
  * the singular values of both Ms are pairwise separated by >= 1e-2 of the largest, every gap is > 0,
  * unstable phi entries <= 1 % of entries and unstable points <= 2 % of points (below).
What was found is printed and stored.  The tests rebuild the weights from the stored seed and factor.

Clouds: the template is U(-1,1)^3, the source the template rotated about z (0.6 rad, + 0.1 per batch element) and shifted by 0.3.
Features are get_rri of each cloud minus its fp32 centroid (the stored `*_centred` arrays), as the reference's dataset computes
them.  Cases a and b feed the network the reference's fp32 features in both precisions (the [B,N,3+4k] input format); case c is the
[B,N,3] format, where the features belong to the computation: its fp64 run centres the stored fp32 cloud in fp64 and uses
get_rri in fp64 on that, which is the computation a model in fp64 performs on the stored input.  Because case c's neighbours are
searched again by whoever consumes the fixture, its template points are redrawn until no point of either cloud is unstable.

Per case and cloud (t = template, s = source): the cloud, the centred cloud, the reference's kNN indices (int16), the features,
logits and gamma in fp32 and fp64 (packed: deepgmr_fixture.py says how, and load_case there rebuilds them), pi, mu, sigma and both
T as fp32 and as fp64, and each quantity's gap = max |fp32 - fp64| (per feature column kind for the features: rp, rq, theta, phi).
  unstable phi entries: in fp64 some b != a has psi_ab within tau_phi = 32 gap_phi of 0 or 2 pi (the wrap is the function's only
    discontinuity), from deepgmr_fixture.rri_restated_fp64, written from the formulas (the reference returns no psi).
  unstable points: in fp64, two consecutive squared distances among the point's first k + 2 neighbours, self included, differ by
    less than 32 * 2^-24 * (|p|^2 + |q|^2), or the point's first neighbour is not itself.
One backward (case b's template against its source jittered by U(-0.02, 0.02) per coordinate, `bw_source`, with the reference's
features of it: on the exact copy the loss is 1e-13 and its gradient rounding noise) of mse(est_T @ igt, I) +
mse(est_T_inverse @ igt^-1, I) through the reference's functions in fp32 and fp64: per parameter the gradient gap over ALL entries, and the fp64 gradient at the entries flat[::stride], stride = ceil(numel / 512)."""
import copy
import math
import os
import sys
from argparse import Namespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg            # noqa: E402
from seeded import seeded_params    # noqa: E402
import deepgmr_fixture as fx        # noqa: E402

TAU_FACTOR = 32.0
FACTORS = (2.0, 2.5, 3.0)
SEED_START = 9100
GRAD_SAMPLES = 512
#         name B   N   k   J  d_model  input
CASES = (("a", 2, 256, 20, 16, 1024, "features"), ("b", 2, 200, 8, 5, 256, "features"), ("c", 1, 256, 20, 16, 256, "points"))
BACKWARD_CASE = "b"
JITTER = 0.02


def motion(B):
    ang = 0.6 + 0.1 * torch.arange(B, dtype=torch.float64)
    R = torch.zeros(B, 3, 3, dtype=torch.float64)
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = ang.cos(), -ang.sin(), ang.sin(), ang.cos(), 1.0
    igt = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)
    igt[:, :3, :3] = R
    igt[:, :3, 3] = 0.3
    return igt.float()                   # source = template * igt


def unstable_points(c64, k):
    """c64 [N,3] fp64 -> bool [N]"""
    d = ((c64[:, None] - c64[None]) ** 2).sum(-1)
    val, idx = torch.sort(d, dim=1)
    val, idx = val[:, :k + 2], idx[:, :k + 2]
    n2 = (c64 ** 2).sum(-1)
    scale = n2[:, None] + torch.maximum(n2[idx[:, :-1]], n2[idx[:, 1:]])
    close = ((val[:, 1:] - val[:, :-1]) < TAU_FACTOR * 2.0 ** -24 * scale).any(dim=1)
    return close | (idx[:, 0] != torch.arange(c64.shape[0]))


def clouds(seed, B, N, k, stable):
    g = torch.Generator().manual_seed(seed)
    template = torch.rand((B, N, 3), generator=g) * 2 - 1
    igt = motion(B)
    move = lambda t: t @ igt[:, :3, :3].transpose(1, 2) + igt[:, None, :3, 3]      # noqa: E731
    for _ in range(200 if stable else 0):
        source = move(template)
        bad = torch.stack([unstable_points((c - c.mean(0)).double(), k) for cl in (template, source) for c in cl]).view(2, B, N).any(0)
        if not bad.any():
            break
        template[bad] = torch.rand((int(bad.sum()), 3), generator=g) * 2 - 1
    else:
        assert not stable, "no stable cloud found"
    return template, move(template), igt


def rri_reference(D, centred, k):
    """the reference's get_rri per cloud in fp32 and fp64, its kNN indices, and the two masks"""
    out = dict(f32=[], f64=[], idx=[], points=[], psi=[])
    for c in centred:
        c32 = c.numpy()
        out["f32"].append(torch.from_numpy(D.get_rri(c32, k)))
        out["f64"].append(torch.from_numpy(D.get_rri(c32.astype(np.float64), k)))
        idx = torch.from_numpy(np.ascontiguousarray(D.knn_idx(c32.astype(np.float64), k))).long()
        assert np.array_equal(D.knn_idx(c32, k), idx.numpy())
        out["idx"].append(idx)
        out["points"].append(unstable_points(c.double(), k))
        out["psi"].append(fx.rri_restated_fp64(c[None], idx[None])[2][0])              # [N,k,k] fp64
    f32, f64 = torch.stack(out["f32"]), torch.stack(out["f64"])
    assert f32.dtype == torch.float32 and f64.dtype == torch.float64
    B, N = f32.shape[:2]
    diff = (f32.double() - f64).abs().view(B, N, k, 4)
    psi = torch.stack(out["psi"])
    # the masks first, from a first estimate of the phi gap that leaves the wrapped entries (off by 2 pi) out
    gap_phi = float(diff[..., 3][diff[..., 3] < 1.0].max())
    tau_phi = TAU_FACTOR * gap_phi
    off = ~torch.eye(k, dtype=torch.bool)
    near = ((psi < tau_phi) | (psi > 2 * math.pi - tau_phi)) & off
    phi_mask = near.any(dim=-1)                                                         # [B,N,k]
    gaps = [float(diff[..., c].max()) for c in range(3)] + [float(diff[..., 3][~phi_mask].max())]
    assert gaps[3] <= gap_phi
    taus = TAU_FACTOR * np.array(gaps)
    taus[3] = tau_phi                                                                   # the band the mask was drawn with
    return f32, f64, torch.stack(out["idx"]), phi_mask, torch.stack(out["points"]), np.array(gaps), taus


def pipeline(G, net, feats, pts, igt=None):
    """DeepGMR.forward :145-151 from the reference's own functions, both clouds; feats / pts: (template, source)"""
    res = {}
    for name, f, p in (("t", feats[0], pts[0]), ("s", feats[1], pts[1])):
        logits = net(f.transpose(1, 2))
        gamma = torch.softmax(logits, dim=2)
        pi, mu, sigma = G.gmm_params(gamma, p)
        res[name] = dict(logits=logits, gamma=gamma, pi=pi, mu=mu, sigma=sigma)
    res["est_T_inverse"] = G.gmm_register(res["t"]["pi"], res["t"]["mu"], res["s"]["mu"], res["s"]["sigma"])
    res["est_T"] = G.gmm_register(res["s"]["pi"], res["s"]["mu"], res["t"]["mu"], res["t"]["sigma"])
    return res


def singular_gaps(res):
    worst = 1.0
    for a, b in (("t", "s"), ("s", "t")):
        pi, ms, mt, sg = res[a]["pi"], res[a]["mu"], res[b]["mu"], res[b]["sigma"]
        cs, ct = pi.unsqueeze(1) @ ms, pi.unsqueeze(1) @ mt
        Ms = ((pi.unsqueeze(2) * (ms - cs)).unsqueeze(3) @ (mt - ct).unsqueeze(2) / sg[:, :, :1, :1]).sum(dim=1)
        s = torch.linalg.svdvals(Ms)
        worst = min(worst, float(((s[:, :-1] - s[:, 1:]) / s[:, :1]).min()), float((s[:, 2] / s[:, 0]).min()))
    return worst


def run_both(G, net, feats32, feats64, pts, grad=False):
    net64 = copy.deepcopy(net).double()
    ctx = torch.enable_grad if grad else torch.no_grad
    with ctx():
        r32 = pipeline(G, net, feats32, pts)
        torch.set_default_dtype(torch.float64)
        try:
            r64 = pipeline(G, net64, feats64, [p.double() for p in pts])
        finally:
            torch.set_default_dtype(torch.float32)
    return r32, r64, net64


def case(G, D, name, B, N, k, J, d_model, fmt, seed, factor):
    template, source, igt = clouds(seed + 500, B, N, k, stable=fmt == "points")
    out = dict(seed=seed, factor=factor, igt=igt)
    feats32, feats64, feats_ref, notes, ok = [], [], [], [], True
    for cn, cloud in (("t", template), ("s", source)):
        centred = cloud - cloud.mean(dim=1, keepdim=True)
        f32, f64, idx, phi_mask, pt_mask, gaps, taus = rri_reference(D, centred, k)
        feats32.append(f32)
        feats_ref.append(f32)
        if fmt == "points":
            # the features belong to the computation: the fp64 run centres the stored fp32 cloud in fp64, as a model in fp64 does
            c64 = cloud.double() - cloud.double().mean(dim=1, keepdim=True)
            feats64.append(torch.stack([torch.from_numpy(D.get_rri(c.numpy(), k)) for c in c64]))
        else:
            feats64.append(f32.double())
        phi_share, pt_share = float(phi_mask.double().mean()), float(pt_mask.double().mean())
        ok = ok and phi_share <= 0.01 and pt_share <= (0.0 if fmt == "points" else 0.02) and bool((gaps > 0).all())
        notes.append(f"{cn}: rri gaps {gaps[0]:.1e} {gaps[1]:.1e} {gaps[2]:.1e} {gaps[3]:.1e}, unstable phi {100 * phi_share:.2f} % points {100 * pt_share:.2f} %")
        out.update({f"{cn}_cloud": cloud, f"{cn}_centred": centred, f"{cn}_idx": idx.to(torch.int16), f"{cn}_feat_gap": gaps,
                    f"{cn}_feat_tau": taus, f"{cn}_phi_unstable": phi_mask, f"{cn}_point_unstable": pt_mask})
        exact = fx.pack_feat64(out, cn, f32.numpy(), f64.numpy(), gaps)
        assert exact[:3].all() and exact[3][~phi_mask.numpy()].all()      # only entries across the wrap are clipped
    out["s_idx_delta"] = out.pop("s_idx") - out["t_idx"]
    fx.pack_pair32(out, "featkm", fx.kind_major(feats_ref[0].numpy()), fx.kind_major(feats_ref[1].numpy()))
    G.args = Namespace(d_model=d_model, n_clusters=J)
    net = seeded_params(G.PointNet(use_rri=True, nearest_neighbors=k), seed).eval()
    with torch.no_grad():
        for v in net.state_dict().values():
            if v.dim() == 3:
                v.mul_(factor)
    pts = (template, source)
    r32, r64, _ = run_both(G, net, feats32, feats64, pts)
    fx.pack_pair32(out, "logits", r32["t"]["logits"].numpy(), r32["s"]["logits"].numpy())
    for cn in ("t", "s"):
        for q in ("logits", "gamma"):
            v32, v64 = r32[cn][q], r64[cn][q]
            out[f"{cn}_{q}_gap"] = float((v32.double() - v64).abs().max())
            if q == "gamma":
                fx.pack_gamma(out, cn, v32.numpy(), v64.numpy())
            else:
                fx.pack_q64(out, f"{cn}_{q}", v32.numpy(), v64.numpy(), out[f"{cn}_{q}_gap"])
        for q in ("pi", "mu", "sigma"):
            v32, v64 = r32[cn][q], r64[cn][q]
            out.update({f"{cn}_{q}32": v32, f"{cn}_{q}64": v64, f"{cn}_{q}_gap": float((v32.double() - v64).abs().max())})
        g64 = r64[cn]["gamma"]
        span = float((g64.amax(dim=(1, 2)) - g64.amin(dim=(1, 2))).min())
        pimin = float(r64[cn]["pi"].min())
        ok = ok and span >= 0.2 and pimin >= 1e-3
        notes.append(f"{cn}: gamma span {span:.3f} max {float(g64.max()):.3f}, pi min {pimin:.1e}")
    for q in ("est_T", "est_T_inverse"):
        gap = float((r32[q].double() - r64[q]).abs().max())
        out.update({f"{q}32": r32[q], f"{q}64": r64[q], f"{q}_gap": gap})
        ok = ok and 0 < gap <= 1e-4
        notes.append(f"{q} gap {gap:.1e}")
    sgap = singular_gaps(r64)
    planted = float((r64["est_T"] - igt.double().inverse()).abs().max())      # template = source * est_T, source = template * igt
    ok = ok and sgap >= 1e-2 and all(v > 0 for kk, v in out.items() if kk.endswith("_gap") and isinstance(v, float))
    print(f"  case {name} seed {seed} factor {factor}: " + "; ".join(notes) + f"; singular separation {sgap:.3f}; |est_T - igt^-1| {planted:.1e}"
          + ("" if ok else "  -- next"))
    if not ok:
        return None
    out["singular_separation"] = sgap
    if name == BACKWARD_CASE:
        # an exact rigid copy puts the loss at its minimum (1e-13) and leaves rounding noise for a gradient: the backward runs on a
        # jittered source, whose features are the reference's again
        g = torch.Generator().manual_seed(seed + 900)
        jittered = source + JITTER * (torch.rand(source.shape, generator=g) * 2 - 1)
        jf32 = rri_reference(D, jittered - jittered.mean(dim=1, keepdim=True), k)[0]
        out.update(bw_source=jittered, bw_s_feat32=jf32)
        out.update(backward(G, net, [feats32[0], jf32], [feats64[0], jf32.double()], (template, jittered), igt))
    return out, list(net.state_dict().keys())


def backward(G, net, feats32, feats64, pts, igt):
    grads = {}
    net = copy.deepcopy(net)
    for p in net.parameters():
        p.grad = None
    r32, r64, net64 = run_both(G, net, feats32, feats64, pts, grad=True)
    for r, m, ig in ((r32, net, igt), (r64, net64, igt.double())):
        eye = torch.eye(4, dtype=ig.dtype).expand_as(ig)
        loss = torch.nn.functional.mse_loss(r["est_T"] @ ig, eye) + torch.nn.functional.mse_loss(r["est_T_inverse"] @ ig.inverse(), eye)
        loss.backward()
        grads[ig.dtype] = {n: p.grad.detach().clone() for n, p in m.named_parameters()}, float(loss.detach())
    (g32, l32), (g64, l64) = grads[torch.float32], grads[torch.float64]
    names = list(g32)
    out = dict(grad_names=np.array(names), grad_loss32=l32, grad_loss64=l64,
               grad_gap=np.array([float((g32[n].double() - g64[n]).abs().max()) for n in names]),
               grad_scale=np.array([float(g64[n].abs().max()) for n in names]))
    for i, n in enumerate(names):
        stride = -(-g64[n].numel() // GRAD_SAMPLES)
        out[f"grad64_{i}"] = g64[n].reshape(-1)[::stride].clone()
    out["grad_stride"] = np.array([-(-g64[n].numel() // GRAD_SAMPLES) for n in names])
    assert (out["grad_gap"] > 0).all()
    rel = out["grad_gap"] / out["grad_scale"]
    print(f"  backward: loss {l64:.3e}, gradient gap / scale per parameter {rel.min():.1e} .. {rel.max():.1e}")
    return out


def main():
    torch.set_num_threads(4)
    mg.import_reference()
    import learning3d.data_utils.dataloaders as D
    import learning3d.models.deepgmr as G
    out, seed = {}, SEED_START
    for name, B, N, k, J, d_model, fmt in CASES:
        got = None
        while got is None:
            for factor in FACTORS:
                got = case(G, D, name, B, N, k, J, d_model, fmt, seed, factor)
                if got is not None:
                    break
            seed += 1
        arrs, keys = got
        out.update({f"{name}_{k_}": v for k_, v in arrs.items()})
        assert len(keys) == 44
    out["cases"] = np.array([c[0] for c in CASES])
    out["case_shapes"] = np.array([c[1:6] for c in CASES])
    out["case_inputs"] = np.array([c[6] for c in CASES])
    out["state_keys"] = np.array(keys)
    out["tau_factor"] = TAU_FACTOR
    arrs = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, "deepgmr_seeded.npz")
    np.savez_compressed(path, **arrs)
    print(f"  deepgmr_seeded.npz  {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
