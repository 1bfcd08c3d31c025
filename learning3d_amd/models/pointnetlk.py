"""Drop-in for learning3d/models/pointnetlk.py on MI355X: PointNetLK, the inverse-compositional Lucas-Kanade loop on PointNet
features.  Same constructor arguments, attribute names and state_dict keys (`dt`, `feature_model.*`) as the reference, so its
checkpoints load with strict=True.

Two routes compute the same forward:
  * the FUSED route (device fp32 clouds, BatchNorm on running statistics, nothing to differentiate): every PointNet pass poses
    its cloud inside the first layer's kernel, the Jacobian's pseudo-inverse and the per-iteration update are one launch each
    (registration.hip), the reference's `break` is a word on the device.  The forward is a fixed list of launches followed by ONE
    device-to-host read (for `itr`, a Python int);
  * the OP-SEQUENCE route (CPU tensors, autograd, train-mode BatchNorm): the reference's operations in plain torch on top of
    the package's PointNet; differentiable, one host read per iteration like the reference.
FUSED_LOOP = False sends everything through the op-sequence route (tests compare the two).

Deviations from the reference, both on purpose: `est_T_series` is returned on the inputs' device (the reference builds it on
the CPU), and on the fused route the convergence test runs on the device.  The default feature_model is built per instance,
not once at import."""
import torch

from ..ops import data_utils, se3
from . import _registration as _reg
from .pointnet import PointNet
from .pooling import Pooling

FUSED_LOOP = True


class PointNetLK(torch.nn.Module):
    def __init__(self, feature_model=None, delta=1.0e-2, learn_delta=False, xtol=1.0e-7, p0_zero_mean=True, p1_zero_mean=True,
                 pooling='max'):
        super().__init__()
        self.feature_model = feature_model if feature_model is not None else PointNet()
        self.pooling = Pooling(pooling)
        self.exp = se3.Exp
        self.transform = se3.transform
        self.dt = torch.nn.Parameter(torch.full((1, 6), float(delta), dtype=torch.float32), requires_grad=learn_delta)
        self.last_err = None
        self.prev_r = None
        self.est_T = None
        self.est_T_series = None
        self.itr = 0
        self.xtol = xtol
        self.p0_zero_mean = p0_zero_mean
        self.p1_zero_mean = p1_zero_mean

    def forward(self, template, source, maxiter=10):
        template, source, template_mean, source_mean = data_utils.mean_shift(template, source, self.p0_zero_mean, self.p1_zero_mean)
        if FUSED_LOOP and maxiter >= 1 and _reg.usable(self, self.feature_model, self.pooling, template, source):
            ctx = self.fused_setup(template, source, maxiter)
            self.fused_loop(ctx)
            result = self.fused_result(ctx)
        else:
            result = self.iclk(template, source, maxiter)
        return data_utils.postprocess_data(result, template, source, template_mean, source_mean, self.p0_zero_mean, self.p1_zero_mean)

    # ------------------------------------------------------------------ fused route
    def fused_setup(self, template, source, maxiter):
        """Everything before the loop, on centred clouds: template features, the finite-difference Jacobian (one PointNet pass over
        the 6 B perturbed templates, which are never written) and its pseudo-inverse; allocates the loop's buffers.  Returns the
        context fused_loop and fused_result take."""
        template, source = _reg.prepare(template, source)
        B, N, _ = template.shape
        dev = template.device
        eye = _reg.identity(B, dev)
        eyeT = eye.view(B, 1, 4, 4)
        words = torch.zeros(5 + B, dtype=torch.int32, device=dev)        # {done, itr, stopped at 0, ticket} | singular[1 + B]
        f0, _ = _reg.posed_features(self.feature_model, template, T=eyeT)
        dt = self.dt.detach().to(device=dev, dtype=torch.float32).reshape(6).contiguous()
        f, _ = _reg.posed_features(self.feature_model, template, dt=dt)
        pinv = _reg.jac_pinv(f0, f, dt, words[4:])
        series = torch.zeros((maxiter + 1, B, 4, 4), dtype=torch.float32, device=dev)
        series[0] = eye
        return {"source": source, "f0": f0, "pinv": pinv, "words": words, "eyeT": eyeT, "maxiter": maxiter,
                "est_T": eye.clone(), "series": series, "r": torch.zeros_like(f0),
                "ws": torch.zeros((B, 8), dtype=torch.float32, device=dev),
                "transformed_source": torch.empty_like(source)}

    def fused_loop(self, ctx):
        """The iterations and the final posed source: launches only, the same list whatever the data, so it can be captured in
        one graph and replayed (launch 0 starts from the identity by itself)."""
        words, est_T = ctx["words"], ctx["est_T"]
        B = est_T.shape[0]
        for i in range(ctx["maxiter"]):
            T = ctx["eyeT"] if i == 0 else est_T.view(B, 1, 4, 4)
            f, _ = _reg.posed_features(self.feature_model, ctx["source"], T=T)
            _reg.iclk_step(f, ctx["f0"], ctx["pinv"], i, ctx["maxiter"], self.xtol, words[4:], ctx["ws"], words, est_T,
                           ctx["series"], ctx["r"])
        _, posed = _reg.posed_features(self.feature_model, ctx["source"], T=est_T.view(B, 1, 4, 4), want_features=False, want_cloud=True)
        ctx["transformed_source"].copy_(posed)

    def fused_result(self, ctx):
        """The one device-to-host read of the forward, then the reference's dictionary (before postprocess_data)."""
        done, itr, stopped_at_0, _, singular = ctx["words"][:5].tolist()
        est_T = ctx["est_T"]
        self.est_T, self.est_T_series = est_T, ctx["series"]
        self.last_err = None
        r = ctx["r"]
        if singular:                                     # torch.inverse raises here; the reference returns early with r = None
            self.last_err = RuntimeError("PointNetLK: J^T J is singular for at least one cloud of the batch")
            r, itr = None, 1
        elif stopped_at_0:
            self.last_err = 0
        self.itr = itr
        return {'est_R': est_T[:, 0:3, 0:3], 'est_t': est_T[:, 0:3, 3], 'est_T': est_T, 'r': r,
                'transformed_source': ctx["transformed_source"], 'itr': itr, 'est_T_series': ctx["series"]}

    # ------------------------------------------------------------------ op-sequence route
    def _features(self, cloud):
        return self.pooling(self.feature_model(cloud))

    def iclk(self, template, source, maxiter):
        B = template.size(0)
        est_T = torch.eye(4).to(template).view(1, 4, 4).expand(B, 4, 4).contiguous()
        series = torch.zeros(maxiter + 1, B, 4, 4, dtype=est_T.dtype, device=est_T.device)
        series[0] = est_T
        self.est_T_series = series
        training = self.handle_batchNorm(template, source)

        f0 = self._features(template)
        dt = self.dt.to(template).expand(B, 6)
        J = self.approx_Jic(template, f0, dt)
        self.last_err = None
        pinv = self.compute_inverse_jacobian(J, f0, source)
        if pinv is None:
            self.feature_model.train(training)
            return {'est_R': est_T[:, 0:3, 0:3], 'est_t': est_T[:, 0:3, 3], 'est_T': est_T, 'r': None,
                    'transformed_source': self.transform(est_T.unsqueeze(1), source), 'itr': 1, 'est_T_series': series}

        itr, r = 0, None
        for itr in range(maxiter):
            self.prev_r = r
            r = self._features(self.transform(est_T.unsqueeze(1), source)) - f0
            dx = -pinv.bmm(r.unsqueeze(-1)).view(B, 6)
            if float(dx.norm(p=2, dim=1).max()) < self.xtol:
                if itr == 0:
                    self.last_err = 0                    # converged before any update
                break
            est_T = self.update(est_T, dx)
            series[itr + 1] = est_T
        series[itr + 1:] = est_T.unsqueeze(0)            # the tail repeats the final estimate

        self.feature_model.train(training)
        self.est_T = est_T
        self.itr = itr + 1
        return {'est_R': est_T[:, 0:3, 0:3], 'est_t': est_T[:, 0:3, 3], 'est_T': est_T, 'r': r,
                'transformed_source': self.transform(est_T.unsqueeze(1), source), 'itr': itr + 1, 'est_T_series': series}

    def update(self, g, dx):
        return self.exp(dx).matmul(g)

    def approx_Jic(self, template, template_features, dt):
        """J[:, :, k] = (f(template) - f(exp(-dt_k e_k) template)) / dt_k  -> [B,K,6]"""
        B, N = template.size(0), template.size(1)
        transf = self.exp(-torch.diag_embed(dt)).unsqueeze(2)                       # [B,6,1,4,4]
        p = self.transform(transf, template.unsqueeze(1))                           # [B,6,N,3]
        f = self._features(p.reshape(-1, N, 3)).view(B, 6, -1).transpose(1, 2)       # [B,K,6]
        return (template_features.unsqueeze(-1) - f) / dt.unsqueeze(1)

    def compute_inverse_jacobian(self, J, template_features, source):
        """pinv(J) = (J^T J)^-1 J^T [B,6,K]; None (and last_err set) when J^T J is singular for any cloud"""
        Jt = J.transpose(1, 2)
        H = Jt.bmm(J)
        inv, info = torch.linalg.inv_ex(H)
        if bool((info != 0).any()):
            self.last_err = RuntimeError("PointNetLK: J^T J is singular for at least one cloud of the batch")
            return None
        return inv.bmm(Jt)

    def handle_batchNorm(self, template, source):
        """In train mode one pass over each cloud updates the BatchNorm statistics; the loop itself then runs on fixed ones."""
        training = self.feature_model.training
        if training:
            self._features(template)
            self._features(source)
        self.feature_model.eval()
        return training
