"""PointNetLK / iPCRNet without a GPU: the SE(3) helpers and both models through the op-sequence route on CPU tensors against
the reference's fp32 results (tests/golden/make_golden_registration.py), gradients against its fp64 ones, checkpoint loading,
and argument validation of registration.hip's entry points."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from seeded import seeded_params      # noqa: E402

HEAD_SEED = 4100                     # make_golden_registration.py


def T(a):
    return torch.from_numpy(np.asarray(a))


def trained_pnlk(golden, **kw):
    from learning3d_amd.models import PointNet, PointNetLK
    w = golden("pnlk_trained_weights")
    net = PointNetLK(PointNet(emb_dims=1024, use_bn=True), **kw)
    net.load_state_dict({k[2:]: T(v) for k, v in w.items()}, strict=True)
    return net.eval()


def seeded_ipcrnet(golden):
    from learning3d_amd.models import PointNet, iPCRNet
    ck = golden("ptnet_checkpoints")
    net = iPCRNet(PointNet(emb_dims=1024))
    net.feature_model.load_state_dict({k[len("ipcrnet.w."):]: T(v) for k, v in ck.items() if k.startswith("ipcrnet.w.")}, strict=True)
    seeded_params(net.linear, HEAD_SEED)
    return net.eval()


def close(got, want, atol, rtol=0.0, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want) - rtol * np.abs(want)
    print(f"{what}: max |got - want| = {np.abs(got - want).max():.3e} (bar {atol:g} + {rtol:g} |want|)")
    assert got.shape == want.shape and err.max() <= atol, what


def test_se3_and_data_utils_match_the_reference(golden):
    from learning3d_amd.ops import se3, data_utils
    z = golden("se3_ops")
    tw, pts, pts2 = T(z["twist"]), T(z["points"]), T(z["points2"])
    norms = tw[:, :3].norm(dim=1)
    assert norms[0] == 0 and (norms[1:3] < 0.01).all() and (norms[3:] > 0.01).all()      # both sides of the Taylor switch, and zero
    g = se3.Exp(tw)
    close(g, z["exp"], 1e-6, what="Exp")
    close(se3.exp(tw), z["exp"], 1e-6, what="exp")
    close(se3.inverse(g), z["inverse"], 1e-6, what="inverse")
    close(se3.transform(g.unsqueeze(1), pts), z["transform"], 1e-6, what="transform points")
    close(se3.transform(g, pts.transpose(1, 2).contiguous()), z["transform_cf"], 1e-6, what="transform channel-first")
    t1, s1, a0, a1 = data_utils.mean_shift(pts, pts2, True, True)
    for got, key in ((t1, "ms_template"), (s1, "ms_source"), (a0, "ms_a0"), (a1, "ms_a1")):
        close(got, z[key], 1e-6, what=key)
    post = data_utils.postprocess_data({'est_T': g.clone(), 'est_T_series': torch.stack([g, se3.inverse(g)])}, t1, s1, a0, a1, True, True)
    close(post['est_T'], z["post_T"], 1e-6, what="postprocess est_T")
    close(post['est_T_series'], z["post_series"], 1e-6, what="postprocess est_T_series")
    t2, s2, b0, b1 = data_utils.mean_shift(pts, pts2, False, False)
    assert t2 is pts and s2 is pts2 and b0.shape == (8, 3, 3) and b1.shape == (8, 3, 3)


def test_exp_gradient_is_the_generator_form():
    """d exp(x)/dx_k is taken as gen_k exp(x) (the reference's ExpMap.backward): at x = 0 that is the exact derivative"""
    from learning3d_amd.ops import se3
    x = torch.zeros(1, 6, dtype=torch.float64, requires_grad=True)
    c = torch.arange(16, dtype=torch.float64).view(1, 4, 4)
    (se3.Exp(x) * c).sum().backward()
    want = torch.tensor([[c[0, 2, 1] - c[0, 1, 2], c[0, 0, 2] - c[0, 2, 0], c[0, 1, 0] - c[0, 0, 1], c[0, 0, 3], c[0, 1, 3], c[0, 2, 3]]])
    assert torch.allclose(x.grad, want, atol=1e-12)


def check_pnlk(res, z, prefix, with_itr):
    close(res['est_T'], z[prefix + "est_T"], 1e-5, what=prefix + "est_T")
    close(res['est_R'], z[prefix + "est_R"], 1e-5, what=prefix + "est_R")          # these two stay in the centred clouds' frame
    close(res['est_t'], z[prefix + "est_t"], 1e-5, what=prefix + "est_t")
    close(res['est_T_series'], z[prefix + "est_T_series"], 1e-5, what=prefix + "est_T_series")
    if prefix + "transformed_source" in z:
        close(res['transformed_source'], z[prefix + "transformed_source"], 1e-5, what=prefix + "transformed_source")
        if z[prefix + "has_r"]:
            close(res['r'], z[prefix + "r"], 1e-5, rtol=1e-4, what=prefix + "r")
        else:
            assert res['r'] is None
    if with_itr:
        assert res['itr'] == int(z[prefix + "itr"])


def test_pointnetlk_checkpoint_and_forward_on_cpu(golden):
    z = golden("pnlk_trained")
    net = trained_pnlk(golden)
    assert tuple(net.dt.shape) == (1, 6) and not net.dt.requires_grad
    with torch.no_grad():
        res = net(T(z["template"]), T(z["source"]), maxiter=10)
    check_pnlk(res, z, "f32.", with_itr=False)                      # itr at xtol 1e-7 sits in fp32 noise: not compared
    assert isinstance(res['itr'], int) and res['est_T_series'].shape == (11, 8, 4, 4)
    net3 = trained_pnlk(golden, xtol=1e-3)
    with torch.no_grad():
        res3 = net3(T(z["template"]), T(z["source"]), maxiter=10)
    check_pnlk(res3, z, "f32.xtol3.", with_itr=True)
    assert res3['itr'] == int(z["f64.xtol3.itr"])
    assert torch.equal(res3['est_T_series'][res3['itr']:], res3['est_T'].unsqueeze(0).expand(11 - res3['itr'], -1, -1, -1))


def test_pointnetlk_small_cases_on_cpu(golden):
    z = golden("pnlk_cases")
    net = trained_pnlk(golden)
    with torch.no_grad():
        res = net(T(z["ragged.template"]), T(z["ragged.source"]))
        check_pnlk(res, z, "ragged.f32.", with_itr=False)
        res = net(T(z["same.template"]), T(z["same.source"]))
        assert res['itr'] == 1 and net.last_err == 0 and float(res['r'].abs().max()) == 0.0
        check_pnlk(res, z, "same.f32.", with_itr=True)
        close(res['est_T'], np.broadcast_to(np.eye(4), (2, 4, 4)), 1e-6, what="identical clouds est_T")
        res = net(T(z["point.template"]), T(z["point.source"]))
        assert res['r'] is None and res['itr'] == 1 and isinstance(net.last_err, RuntimeError)
        check_pnlk(res, z, "point.f32.", with_itr=True)
        res = trained_pnlk(golden, p0_zero_mean=False, p1_zero_mean=False)(T(z["nomean.template"]), T(z["nomean.source"]))
        check_pnlk(res, z, "nomean.f32.", with_itr=False)


def test_pointnetlk_gradients_on_cpu(golden):
    """Loss and gradients of FrobeniusNormLoss(est_T, igt) + RMSEFeaturesLoss(r) after two iterations, op-sequence route, at the
    training path's 2e-5-of-scale bar: the route run in fp64 against the reference's fp64 gradients (measured here: 8e-15 and
    2e-15 of scale for conv1 / conv5), and run in fp32 against the reference's fp32 gradients (2.8e-6, 5.8e-7).  An fp32 run is
    NOT held to the fp64 fixture: the reference's own fp32 gradients are 5.5e-5 (conv1) and 1.6e-5 (conv5) of scale away from its
    fp64 ones -- the pseudo-inverse amplifies fp32 feature rounding -- and ours sit at the same 5.5e-5 / 1.6e-5 (printed below)."""
    from learning3d_amd.losses import FrobeniusNormLoss, RMSEFeaturesLoss
    z = golden("pnlk_grad")
    for tag, dtype in (("f64.", torch.float64), ("f32.", torch.float32)):
        net = trained_pnlk(golden).to(dtype)
        res = net(T(z["template"]).to(dtype), T(z["source"]).to(dtype), maxiter=2)
        loss = FrobeniusNormLoss()(res['est_T'], T(z["igt"]).to(dtype)) + RMSEFeaturesLoss()(res['r'])
        loss.backward()
        print(tag, "loss", float(loss), "reference", float(z[tag + "loss"]), "reference fp64", float(z["f64.loss"]))
        assert abs(float(loss) - float(z[tag + "loss"])) <= 2e-5 * abs(float(z[tag + "loss"]))
        for name in ("conv1", "conv5"):
            got = getattr(net.feature_model, name).weight.grad.numpy().astype(np.float64)
            want, want64 = z[tag + "grad_" + name].astype(np.float64), z["f64.grad_" + name]
            err = np.abs(got - want).max() / np.abs(want).max()
            print(f"{tag}{name}: max error / scale = {err:.3e} (bar 2e-5); against the fp64 reference {np.abs(got - want64).max() / np.abs(want64).max():.3e}")
            assert err <= 2e-5


def test_ipcrnet_on_cpu(golden):
    z8, z1 = golden("ipcrnet_seeded"), golden("ipcrnet_seeded_it1")
    net = seeded_ipcrnet(golden)
    assert [k for k in net.state_dict() if k.startswith("linear.")][0] == "linear.0.weight" and "linear.10.weight" in net.state_dict()
    for z, iters in ((z8, 8), (z1, 1)):
        with torch.no_grad():
            res = net(T(z8["template"]), T(z8["source"]), max_iteration=iters)
        assert res['est_t'].shape == (8, 1, 3)
        for k in ("est_R", "est_t", "est_T", "transformed_source"):
            close(res[k], z["f32." + k], 1e-5, what=f"iPCRNet[{iters}] {k}")
        close(res['r'], z["f32.r"], 1e-5, rtol=1e-4, what=f"iPCRNet[{iters}] r")


def test_registration_argument_validation_without_gpu():
    import ctypes as C
    from learning3d_amd import _lib
    l = _lib.lib()
    buf = C.create_string_buffer(256)
    p = C.cast(buf, C.c_void_p)
    # null pointers / non-positive sizes -> -1, shapes the kernels do not take -> -2, before any launch
    assert l.l3d_reg_pose_first_layer(None, p, None, 1, 1, 8, p, None, None, 64, 1, p, None, None) == -1
    assert l.l3d_reg_pose_first_layer(p, p, None, 1, 1, 8, p, None, None, 64, 1, None, None, None) == -1       # no output asked for
    assert l.l3d_reg_pose_first_layer(p, p, p, 1, 6, 8, p, None, None, 64, 1, p, None, None) == -1            # transforms AND dt
    assert l.l3d_reg_pose_first_layer(p, None, None, 1, 6, 8, p, None, None, 64, 1, p, None, None) == -1      # neither
    assert l.l3d_reg_pose_first_layer(p, p, None, 1, 1, 8, None, None, None, 64, 1, p, None, None) == -1      # features without weights
    assert l.l3d_reg_pose_first_layer(p, p, None, 0, 1, 8, p, None, None, 64, 1, p, None, None) == -1
    assert l.l3d_reg_pose_first_layer(p, None, p, 1, 5, 8, p, None, None, 64, 1, p, None, None) == -2          # dt wants 6 transforms
    assert l.l3d_reg_pose_first_layer(p, p, None, 1, 1, 8, p, None, None, 60, 1, p, None, None) == -2          # C1 % 16
    assert l.l3d_reg_pose_first_layer(p, p, None, 20000, 6, 8, p, None, None, 64, 1, p, None, None) == -2      # B Tn > 65535
    assert l.l3d_reg_jac_pinv(None, p, p, 1, 8, p, p, None) == -1
    assert l.l3d_reg_jac_pinv(p, p, p, 1, 0, p, p, None) == -1
    assert l.l3d_reg_jac_pinv(p, p, p, 70000, 8, p, p, None) == -2
    assert l.l3d_reg_iclk_step(None, p, p, 1, 8, 0, 10, 1e-7, p, p, p, p, p, p, None) == -1
    assert l.l3d_reg_iclk_step(p, p, p, 1, 8, 10, 10, 1e-7, p, p, p, p, p, p, None) == -1                      # step outside [0, maxiter)
    assert l.l3d_reg_iclk_step(p, p, p, 1, 8, 0, 0, 1e-7, p, p, p, p, p, p, None) == -1
    assert l.l3d_reg_iclk_step(p, p, p, 70000, 8, 0, 10, 1e-7, p, p, p, p, p, p, None) == -2
    assert l.l3d_reg_quat_update(None, 1, 1, p, p, p, None) == -1
    assert l.l3d_reg_quat_update(p, 0, 1, p, p, p, None) == -1
    assert l.l3d_reg_quat_update(p, (1 << 24) + 1, 1, p, p, p, None) == -2


def test_models_are_exported_and_route_switch_exists():
    from learning3d_amd import models, ops
    from learning3d_amd.models import pointnetlk
    assert models.PointNetLK is pointnetlk.PointNetLK and models.iPCRNet.__name__ == "iPCRNet"
    assert pointnetlk.FUSED_LOOP is True
    assert hasattr(ops, "se3") and hasattr(ops, "data_utils")
    a, b = models.PointNetLK(), models.PointNetLK()
    assert a.feature_model is not b.feature_model                # built per instance
