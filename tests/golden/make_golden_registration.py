"""Fixtures of the iterative registration models (PointNetLK, iPCRNet), from the REFERENCE on the CPU:

    python tests/golden/make_golden_registration.py

Needs the reference checkout make_golden.py reads (its trained PointNetLK checkpoint included).  Writes, next to this file,
se3_ops.npz, pnlk_trained_weights.npz, pnlk_trained.npz, pnlk_pinv.npz, pnlk_cases.npz, pnlk_grad.npz, ipcrnet_seeded.npz and
ipcrnet_seeded_it1.npz: arrays only.  Every model result is stored twice, computed in fp32 and in fp64 (`net.double()`)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg            # noqa: E402
from seeded import seeded_params    # noqa: E402

HEAD_SEED = 4100


def save(name, **arrs):
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"  {name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) < (1 << 20)


def slab_clouds(B, N, gen):
    """points on the surface of a 2 x 1.2 x 0.6 box: a shape with three distinct axes, so that its pose is well determined"""
    p = torch.rand(B, N, 3, generator=gen) * 2 - 1
    ax = torch.randint(0, 3, (B, N), generator=gen)
    bi, ni = torch.arange(B)[:, None], torch.arange(N)[None]
    p[bi, ni, ax] = torch.sign(p[bi, ni, ax])
    return p * torch.tensor([1.0, 0.6, 0.3])


def main():
    torch.set_num_threads(4)
    mg.import_reference()
    from learning3d.models import PointNet, PointNetLK, iPCRNet
    from learning3d.ops import se3, data_utils
    from learning3d.losses import FrobeniusNormLoss, RMSEFeaturesLoss
    gen = torch.Generator().manual_seed(20260)

    # ---- se3 / data_utils values (fp32, the reference's own CPU arithmetic)
    tw = torch.randn(8, 6, generator=gen) * 0.3
    tw[0] = 0
    tw[1, :3] = tw[1, :3] / tw[1, :3].norm() * 0.005          # below the Taylor switch at 0.01
    tw[2, :3] = tw[2, :3] / tw[2, :3].norm() * 0.0099
    tw[3, :3] = tw[3, :3] / tw[3, :3].norm() * 0.0101         # just above it
    tw[4, :3] = tw[4, :3] / tw[4, :3].norm() * 0.02
    pts = torch.rand(8, 40, 3, generator=gen) * 2 - 1
    pts2 = torch.rand(8, 40, 3, generator=gen) + 0.5
    g = se3.exp(tw)
    t1, s1, a0, a1 = data_utils.mean_shift(pts, pts2, True, True)
    post = data_utils.postprocess_data({'est_T': g.clone(), 'est_T_series': torch.stack([g, se3.inverse(g)])}, t1, s1, a0, a1, True, True)
    save("se3_ops", twist=tw, exp=g, inverse=se3.inverse(g), points=pts, points2=pts2, transform=se3.transform(g.unsqueeze(1), pts),
         transform_cf=se3.transform(g, pts.transpose(1, 2).contiguous()), ms_template=t1, ms_source=s1, ms_a0=a0, ms_a1=a1,
         post_T=post['est_T'], post_series=post['est_T_series'])

    # ---- PointNetLK with the trained checkpoint
    sd = torch.load(os.path.join(mg.REF, "pretrained", "exp_pnlk", "models", "best_model.t7"), map_location="cpu", weights_only=False)
    save("pnlk_trained_weights", **{"w." + k: v for k, v in sd.items()})

    def pnlk(dtype, **kw):
        net = PointNetLK(PointNet(emb_dims=1024, use_bn=True), **kw)
        net.load_state_dict(sd, strict=True)
        return net.eval().to(dtype)

    def run(dtype, tpl, src, maxiter=10, **kw):
        net = pnlk(dtype, **kw)
        norms, upd = [], net.update

        def recording(g_, dx):
            norms.append(float(dx.norm(p=2, dim=1).max()))
            return upd(g_, dx)
        net.update = recording
        with torch.no_grad():
            res = net(tpl.to(dtype), src.to(dtype), maxiter=maxiter)
        return res, np.array(norms), net

    def pack(prefix, res, small=False):
        out = {prefix + "est_T": res['est_T'], prefix + "est_T_series": res['est_T_series'], prefix + "itr": res['itr'],
               prefix + "est_R": res['est_R'], prefix + "est_t": res['est_t']}       # est_R / est_t stay in the centred frame
        if not small:
            out[prefix + "transformed_source"] = res['transformed_source']
            out[prefix + "has_r"] = res['r'] is not None
            if res['r'] is not None:
                out[prefix + "r"] = res['r']
        return out

    B, N = 8, 1024
    tpl = slab_clouds(B, N, gen)
    x = torch.randn(B, 6, generator=gen)
    x = x / x.norm(dim=1, keepdim=True) * (0.2 + 0.2 * torch.rand(B, 1, generator=gen))          # twists of norm 0.2 .. 0.4
    src = se3.transform(se3.exp(x).unsqueeze(1), tpl)
    arrs = {"template": tpl, "source": src, "twist": x}
    for tag, dtype in (("f32.", torch.float32), ("f64.", torch.float64)):
        res, _, _ = run(dtype, tpl, src)
        arrs.update(pack(tag, res))
        _, norms, _ = run(dtype, tpl, src, xtol=0.0)                 # never stops: max |dx| of all 10 iterations
        arrs[tag + "dx_norms"] = norms
        res3, _, _ = run(dtype, tpl, src, xtol=1e-3)
        arrs.update(pack(tag + "xtol3.", res3, small=True))
    n64 = arrs["f64.dx_norms"]
    assert all(v > 3e-3 or v < 1e-3 / 3 for v in n64), n64        # itr at xtol 1e-3 is decided by the algorithm, not by rounding
    assert arrs["f32.xtol3.itr"] == arrs["f64.xtol3.itr"]
    print("  max|dx| fp64:", n64, " itr at xtol 1e-3:", arrs["f64.xtol3.itr"], " default xtol:", arrs["f32.itr"], arrs["f64.itr"])
    save("pnlk_trained", **arrs)

    # ---- the pseudo-inverse alone: features of 4 clouds (fp32 reference), its fp32 pinv
    net = pnlk(torch.float32)
    with torch.no_grad():
        t4 = tpl[:4] - tpl[:4].mean(dim=1, keepdim=True)
        f0 = net.pooling(net.feature_model(t4))
        dt = net.dt.expand(4, 6)
        J = net.approx_Jic(t4, f0, dt)                                  # [B,K,6]
        f = f0.unsqueeze(-1) - J * dt.unsqueeze(1)                      # the perturbed features it was made from (to rounding)
        J = (f0.unsqueeze(-1) - f) / dt.unsqueeze(1)
        pinv = net.compute_inverse_jacobian(J, f0, t4)
    save("pnlk_pinv", f0=f0, f=f.transpose(1, 2).contiguous(), dt=net.dt.reshape(6), pinv32=pinv)

    # ---- small cases (B 2, N 96)
    small = slab_clouds(2, 96, gen)
    xs = torch.randn(2, 6, generator=gen) * 0.1
    small_src = se3.transform(se3.exp(xs).unsqueeze(1), small)
    point = torch.full((2, 96, 3), 0.25)                                 # one repeated point: J^T J is exactly singular
    arrs = {"ragged.template": small, "ragged.source": small_src, "same.template": small, "same.source": small.clone(),
            "point.template": point, "point.source": small_src, "nomean.template": small, "nomean.source": small_src}
    for tag, dtype in (("f32.", torch.float32), ("f64.", torch.float64)):
        res, _, _ = run(dtype, small, small_src)
        arrs.update(pack("ragged." + tag, res))
        res, _, net = run(dtype, small, small.clone())
        assert res['itr'] == 1 and net.last_err == 0
        arrs.update(pack("same." + tag, res))
        res, _, net = run(dtype, point, small_src)
        assert res['r'] is None and res['itr'] == 1 and isinstance(net.last_err, RuntimeError), net.last_err
        arrs.update(pack("point." + tag, res))
        res, _, _ = run(dtype, small, small_src, p0_zero_mean=False, p1_zero_mean=False)
        arrs.update(pack("nomean." + tag, res))
    save("pnlk_cases", **arrs)

    # ---- gradients through two iterations (fp64; fp32 alongside)
    arrs = {"template": small, "source": small_src, "igt": se3.exp(xs)}
    for tag, dtype in (("f32.", torch.float32), ("f64.", torch.float64)):
        net = pnlk(dtype)
        res = net(small.to(dtype), small_src.to(dtype), maxiter=2)
        loss = FrobeniusNormLoss()(res['est_T'], se3.exp(xs).to(dtype)) + RMSEFeaturesLoss()(res['r'])
        loss.backward()
        arrs.update({tag + "loss": loss, tag + "grad_conv1": net.feature_model.conv1.weight.grad,
                     tag + "grad_conv5": net.feature_model.conv5.weight.grad, tag + "est_T": res['est_T']})
    save("pnlk_grad", **arrs)

    # ---- iPCRNet: PointNet part from ptnet_checkpoints.npz, head seeded
    ck = np.load(os.path.join(HERE, "ptnet_checkpoints.npz"))
    fm_sd = {k[len("ipcrnet.w."):]: torch.from_numpy(ck[k]) for k in ck.files if k.startswith("ipcrnet.w.")}

    def ipcr(dtype):
        net = iPCRNet(PointNet(emb_dims=1024))
        net.feature_model.load_state_dict(fm_sd, strict=True)
        seeded_params(net.linear, HEAD_SEED)
        return net.eval().to(dtype)
    tpl2 = slab_clouds(B, N, gen)
    x2 = torch.randn(B, 6, generator=gen) * 0.15
    src2 = se3.transform(se3.exp(x2).unsqueeze(1), tpl2)
    for name, iters in (("ipcrnet_seeded", 8), ("ipcrnet_seeded_it1", 1)):
        arrs = {"template": tpl2, "source": src2} if iters == 8 else {}
        for tag, dtype in (("f32.", torch.float32), ("f64.", torch.float64)):
            with torch.no_grad():
                res = ipcr(dtype)(tpl2.to(dtype), src2.to(dtype), max_iteration=iters)
            arrs.update({tag + k: v for k, v in res.items()})
        save(name, **arrs)


if __name__ == "__main__":
    main()
