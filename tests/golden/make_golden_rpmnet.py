"""Fixture of RPMNet and PPFNet, from the REFERENCE on the CPU:

    python tests/golden/make_golden_rpmnet.py

Needs the reference checkout make_golden.py reads.  Writes rpmnet_seeded.npz next to this file: arrays and lists of names only.
It calls the reference's own functions and copies none of its code: models.rpmnet.RPMNet / sinkhorn / compute_rigid_transform,
models.ppfnet.PPFNet and utils.ppfnet_util.sample_and_group_multi.  Everything is run in fp32 and in fp64
(`copy.deepcopy(net).double()`, the same fp32 inputs cast up, inside torch.set_default_dtype(torch.float64) because split_normals
builds its zero normals in the default dtype).  Per quantity: gap = max |fp32 - fp64| (relative to the fp64 value for
perm_matrices_init, which spans e^-100..e^100) and the fp64 value.

What is stored of the fp64 value.  A committed file stays under 1 MiB, and the large tensors (a [B,J,K] matrix per iteration, the
[B,N,K,10] grouped features, the [B,C,K,N] layer outputs) would be megabytes.  They are stored as `<name>_s64`: the flattened
fp64 tensor at flat[::stride], stride = ceil(numel / 2048), beside their gap and their shape.  Everything else (transforms,
est_T, weighted template points, beta, alpha, every Sinkhorn and Kabsch case) is stored whole in fp64.  The tests rebuild the
whole fp64 tensors by running this package's op sequence in fp64 on the CPU, which tests/test_rpmnet_cpu.py first holds to 1e-9
against everything stored here, samples included (rpmnet_fixture.py).

Whole-model cases, weights seeded_params(net, seed), then every GroupNorm weight of the feature network times GN_FACTOR = 10:
seeded_params draws 1-d tensors from U(-0.1, 0.1), and with GroupNorm scales that small every layer's output is its bias plus a
tenth of the signal, the unit features of all points coincide (affinity span 0.006 at beta 30, permutation maximum 0.006) and
est_T is an ill-conditioned Kabsch of a flat permutation.  With scales of U(-1, 1), both signs, the permutation peaks.
  a  template 160 points with normals, source its first 128 points rotated and shifted; PPFNet(num_neighbors=16), 2 iterations;
     weights_net.postpool[-1].bias[0] = 30, so that beta ~ 30 and the affinities span more than a hundred (with the default bias
     the permutation is flat, its maximum 0.012, and tests nothing)
  b  the same clouds and seed with num_neighbors=64
  c  the xyz columns alone, [B,N,3]: clouds without normals; num_neighbors=16, 1 iteration
Clouds: half the points uniform in a cube of side 0.35 (dense: their balls of radius 0.3 overflow K), half uniform in [-1,1]^3
(sparse: below K, many alone), unit normals.  The seed is stepped until
  * case a's final permutation has maximum >= 0.5 and a row-sum minimum <= 0.85,
  * in every cloud at least one centre has more than K + 1 points in its ball, one fewer than K and one only itself (K = 16),
  * no pair of points of a cloud has an expanded squared distance within 32 * 2^-24 * (|p|^2 + |q|^2) of radius^2, in either
    iteration's moved source too, so fp32, fp64 and this package's ball query group the same neighbours,
  * every stored gap is > 0 except those of exact quantities (the padded zeros),
and what was found is printed.

Per-function cases: sample_and_group_multi on case a's and case c's template (with its idx, int16); the three pre-pool layer
outputs on case a's template; sinkhorn at (J,K) = (50,70), (130,67), (1,1), (1,64), (65,1) on N(0, 3^2) inputs, one (50,70)
case scaled to +-200, n_iters 5 (n_iters 0 returns the input and needs no record); compute_rigid_transform at M 128 with case
a's first-iteration weights, at M 3, and on a pair whose optimal orthogonal map is a reflection."""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg            # noqa: E402
from seeded import seeded_params    # noqa: E402

SEED_START = 4200
B, N, J = 2, 160, 128
RADIUS = 0.3
SAMPLES = 2048
MARGIN = 32.0 * 2.0 ** -24
BETA_BIAS = 30.0
GN_FACTOR = 10.0
MAX_SEEDS = 20
#         name  K  iterations normals
CASES = (("a", 16, 2, True), ("b", 64, 2, True), ("c", 16, 1, False))
SINKHORN = (("s0", 50, 70, 1.0), ("s1", 130, 67, 1.0), ("s2", 1, 1, 1.0), ("s3", 1, 64, 1.0), ("s4", 65, 1, 1.0), ("wide", 50, 70, None))


def clouds(seed):
    g = torch.Generator().manual_seed(seed)
    dense = torch.rand((B, N // 2, 3), generator=g) * 0.35 - 0.175
    sparse = torch.rand((B, N - N // 2, 3), generator=g) * 2 - 1
    xyz = torch.cat([dense, sparse], dim=1)
    xyz = xyz[:, torch.randperm(N, generator=g)]
    nrm = torch.randn((B, N, 3), generator=g)
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    ang = 0.5 + 0.1 * torch.arange(B, dtype=torch.float64)
    R = torch.zeros(B, 3, 3, dtype=torch.float64)
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = ang.cos(), -ang.sin(), ang.sin(), ang.cos(), 1.0
    R = R.float()
    shift = torch.tensor([0.1, -0.05, 0.08])
    template = torch.cat([xyz, nrm], dim=-1)
    source = torch.cat([xyz[:, :J] @ R.transpose(1, 2) + shift, nrm[:, :J] @ R.transpose(1, 2)], dim=-1)
    return template.contiguous(), source.contiguous()


def ball_ok(xyz32):
    """xyz32 [B,n,3]: the margin around radius^2 in the expanded form, and the three kinds of centre"""
    x = xyz32.double()
    n2 = (x ** 2).sum(-1)
    d = n2[:, :, None] + n2[:, None, :] - 2 * x @ x.transpose(1, 2)
    margin = bool(((d - RADIUS ** 2).abs() > MARGIN * (n2[:, :, None] + n2[:, None, :])).all())
    cnt = (d <= RADIUS ** 2).sum(-1)                                   # the centre included
    kinds = [bool(((cnt > 16 + 1).any(1) & (cnt < 16).any(1) & (cnt == 1).any(1)).all())]
    return margin, kinds[0], cnt


def sampled(v64):
    flat = v64.reshape(-1)
    stride = -(-flat.numel() // SAMPLES)
    return flat[::stride].clone()


def gap_of(v32, v64, relative=False):
    diff = (v32.double() - v64).abs()
    return float((diff / v64.abs()).max() if relative else diff.max())


def both(fn32, fn64):
    with torch.no_grad():
        r32 = fn32()
        torch.set_default_dtype(torch.float64)
        try:
            r64 = fn64()
        finally:
            torch.set_default_dtype(torch.float32)
    return r32, r64


def model_case(Rm, Pm, name, K, iters, normals, seed, template, source, out, notes):
    t = template if normals else template[:, :, :3].contiguous()
    s = source if normals else source[:, :, :3].contiguous()
    net = seeded_params(Rm.RPMNet(feature_model=Pm.PPFNet(num_neighbors=K)), seed).eval()
    with torch.no_grad():
        for m in net.feat_extractor.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.mul_(GN_FACTOR)
    if name == "a":
        with torch.no_grad():
            net.weights_net.postpool[-1].bias[0] = BETA_BIAS
    net64 = copy.deepcopy(net).double()
    r32, r64 = both(lambda: net(t, s, iters), lambda: net64(t.double(), s.double(), iters))
    ok = True
    for q in ("est_T", "beta", "alpha"):
        v32, v64 = torch.as_tensor(r32[q]), torch.as_tensor(r64[q])
        out[f"{name}_{q}_64"], out[f"{name}_{q}_gap"] = v64, gap_of(v32, v64)
    for i in range(iters):
        for q in ("transforms", "weighted_template"):
            out[f"{name}_{q}{i}_64"], out[f"{name}_{q}{i}_gap"] = r64[q][i], gap_of(r32[q][i], r64[q][i])
        for q, rel in (("perm_matrices", False), ("perm_matrices_init", True)):
            out[f"{name}_{q}{i}_s64"], out[f"{name}_{q}{i}_gap"] = sampled(r64[q][i]), gap_of(r32[q][i], r64[q][i], rel)
        # the moved source of the next iteration must group stably too
        moved = Rm.se3_transform(r64["transforms"][i], s[:, :, :3].double()).float()
        ok = ok and ball_ok(moved)[0]
    perm = r64["perm_matrices"][-1]
    pmax, rmin, rmax = float(perm.max()), float(perm.sum(2).min()), float(perm.sum(2).max())
    span = float(torch.log(r64["perm_matrices_init"][0]).max() - torch.log(r64["perm_matrices_init"][0]).min())
    out[f"{name}_perm_max"], out[f"{name}_rowsum_min"] = pmax, rmin
    notes.append(f"case {name}: perm max {pmax:.3f}, row sums {rmin:.2f}-{rmax:.2f}, affinity span {span:.0f}, gaps perm "
                 f"{out[f'{name}_perm_matrices{iters - 1}_gap']:.1e} est_T {out[f'{name}_est_T_gap']:.1e} init (rel) "
                 f"{out[f'{name}_perm_matrices_init{iters - 1}_gap']:.1e} beta {out[f'{name}_beta_gap']:.1e}")
    if name == "a":
        ok = ok and pmax >= 0.5 and rmin <= 0.85
    ok = ok and all(out[k] > 0 for k in out if k.startswith(name + "_") and k.endswith("_gap"))
    return ok, net, net64, r32, r64


def main():
    torch.set_num_threads(4)
    mg.import_reference()
    import learning3d.models.rpmnet as Rm
    import learning3d.models.ppfnet as Pm
    import learning3d.utils.ppfnet_util as U
    seed = SEED_START
    while True:
        out, notes = {}, []
        template, source = clouds(seed)
        m_t, k_t, cnt = ball_ok(template[:, :, :3])
        m_s, k_s, _ = ball_ok(source[:, :, :3])
        ok = m_t and m_s and k_t and k_s
        notes.append(f"seed {seed}: margin {m_t and m_s}, centre kinds {k_t and k_s}; template centres with > 17 in the ball "
                     f"{int((cnt > 17).sum())}, < 16 {int((cnt < 16).sum())}, alone {int((cnt == 1).sum())} of {B * N}")
        keep = {}
        if ok:
            for name, K, iters, normals in CASES:
                good, net, net64, r32, r64 = model_case(Rm, Pm, name, K, iters, normals, seed, template, source, out, notes)
                keep[name] = (net, net64, r32, r64)
                ok = ok and good
                if not ok:
                    break
        print("\n".join("  " + n for n in notes) + ("" if ok else "\n  -- next seed"))
        if ok:
            break
        seed += 1
        assert seed < SEED_START + MAX_SEEDS, "no seed met the conditions"
    out.update(gn_factor=GN_FACTOR, seed=seed, template=template, source=source, beta_bias=BETA_BIAS, radius=RADIUS,
               cases=np.array([c[0] for c in CASES]), case_K=np.array([c[1] for c in CASES]),
               case_iters=np.array([c[2] for c in CASES]), case_normals=np.array([c[3] for c in CASES]))
    net_a = keep["a"][0]
    out["ppfnet_state_keys"] = np.array(list(net_a.feat_extractor.state_dict().keys()))
    out["ppfnet_state_shapes"] = np.array([str(tuple(v.shape)) for v in Pm.PPFNet().state_dict().values()])
    out["rpmnet_state_keys"] = np.array(list(net_a.state_dict().keys()))
    out["rpmnet_state_shapes"] = np.array([str(tuple(v.shape)) for v in Rm.RPMNet(feature_model=Pm.PPFNet()).state_dict().values()])

    # sample_and_group_multi on the templates of cases a and c, and the pre-pool layers on case a's
    for name, normals in (("a", True), ("c", False)):
        xyz = template[:, :, :3].contiguous()
        nrm = template[:, :, 3:].contiguous() if normals else torch.zeros_like(xyz)
        (f32, _, _), (f64, _, _) = both(lambda: U.sample_and_group_multi(-1, RADIUS, 16, xyz, nrm, returnfps=True),
                                        lambda: U.sample_and_group_multi(-1, RADIUS, 16, xyz.double(), nrm.double(), returnfps=True))
        i32 = U.query_ball_point(RADIUS, 16, xyz, xyz, torch.arange(N)[None].repeat(B, 1))
        i64 = U.query_ball_point(RADIUS, 16, xyz.double(), xyz.double(), torch.arange(N)[None].repeat(B, 1))
        assert torch.equal(i32, i64)
        out[f"group_{name}_idx"] = i32.to(torch.int16)
        for q in ("dxyz", "ppf"):
            out[f"group_{name}_{q}_s64"], out[f"group_{name}_{q}_gap"] = sampled(f64[q]), gap_of(f32[q], f64[q])
        pad = (i32 == torch.arange(N)[None, :, None])
        out[f"group_{name}_pad_gap"] = max(gap_of(f32[q][pad], f64[q][pad]) for q in ("dxyz", "ppf"))
        assert out[f"group_{name}_pad_gap"] == 0.0 and float(f64["ppf"][pad].abs().max()) == 0.0
        print(f"  group {name}: gaps dxyz {out[f'group_{name}_dxyz_gap']:.1e} ppf {out[f'group_{name}_ppf_gap']:.1e}, padded slots "
              f"{int(pad.sum())} of {pad.numel()} exact")
    net, net64 = keep["a"][0], keep["a"][1]
    fx32, fx64 = net.feat_extractor, net64.feat_extractor
    xyz, nrm = template[:, :, :3].contiguous(), template[:, :, 3:].contiguous()

    def layers(fx, xyz, nrm):
        f = U.sample_and_group_multi(-1, RADIUS, 16, xyz, nrm)
        x = torch.cat([f['xyz'][:, :, None, :].expand(-1, -1, 16, -1), f['dxyz'], f['ppf']], -1).permute(0, 3, 2, 1)
        res = []
        for i, m in enumerate(fx.prepool):
            x = m(x)
            if i in (0, 3, 6):
                res.append(x)                      # the convolution's output, in front of its GroupNorm
        return res
    l32, l64 = both(lambda: layers(fx32, xyz, nrm), lambda: layers(fx64, xyz.double(), nrm.double()))
    for i in range(3):
        out[f"layer{i}_s64"], out[f"layer{i}_gap"] = sampled(l64[i]), gap_of(l32[i], l64[i])
    print("  pre-pool conv outputs, gaps " + " ".join(f"{out[f'layer{i}_gap']:.1e}" for i in range(3)))

    # sinkhorn
    g = torch.Generator().manual_seed(seed + 77)
    for name, Jc, Kc, scale in SINKHORN:
        x = torch.randn((1, Jc, Kc), generator=g) * 3.0
        if scale is None:
            x = x / x.abs().max() * 200.0
        ref = torch.rand((1, Kc, 3), generator=g) * 2 - 1
        r32, r64 = both(lambda: Rm.sinkhorn(x, 5, slack=True), lambda: Rm.sinkhorn(x.double(), 5, slack=True))
        out.update({f"sk_{name}_in": x, f"sk_{name}_ref": ref, f"sk_{name}_64": r64, f"sk_{name}_gap": gap_of(r32, r64),
                    f"sk_{name}_perm_gap": gap_of(r32.exp(), r64.exp())})
        print(f"  sinkhorn {name} ({Jc},{Kc}): gap log {out[f'sk_{name}_gap']:.1e} perm {out[f'sk_{name}_perm_gap']:.1e}, |in| max {float(x.abs().max()):.0f}")
    out["sinkhorn_cases"] = np.array([c[0] for c in SINKHORN])

    # compute_rigid_transform
    r64a = keep["a"][3]
    w = r64a["perm_matrices"][0].sum(2).float()
    kab = {"k0": (source[:, :, :3].contiguous(), r64a["weighted_template"][0].float(), w)}
    a3 = torch.rand((B, 3, 3), generator=g) * 2 - 1
    kab["k1"] = (a3, a3 @ torch.linalg.qr(torch.randn((B, 3, 3), generator=g))[0] + 0.2, torch.rand((B, 3), generator=g) + 0.5)
    ar = torch.rand((B, 32, 3), generator=g) * 2 - 1
    mirror = torch.diag(torch.tensor([1.0, 1.0, -1.0]))
    kab["k2"] = (ar, ar @ mirror + 0.01 * torch.randn((B, 32, 3), generator=g) + 0.3, torch.rand((B, 32), generator=g) + 0.5)
    for name, (a, b, w) in kab.items():
        r32, r64 = both(lambda: Rm.compute_rigid_transform(a, b, w), lambda: Rm.compute_rigid_transform(a.double(), b.double(), w.double()))
        out.update({f"kab_{name}_a": a, f"kab_{name}_b": b, f"kab_{name}_w": w, f"kab_{name}_64": r64, f"kab_{name}_gap": gap_of(r32, r64)})
        cov_det = float(torch.det((a.double() - a.double().mean(1, keepdim=True)).transpose(1, 2) @ (b.double() - b.double().mean(1, keepdim=True))).max())
        print(f"  kabsch {name} M {a.shape[1]}: gap {out[f'kab_{name}_gap']:.1e}, largest det(cov) {cov_det:.2e}")
    out["kabsch_cases"] = np.array(list(kab))

    arrs = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, "rpmnet_seeded.npz")
    np.savez_compressed(path, **arrs)
    print(f"  rpmnet_seeded.npz  {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
