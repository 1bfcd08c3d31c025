"""Drop-in for learning3d/models/deepgmr.py on MI355X: DeepGMR, registration of two clouds as the alignment of two Gaussian mixtures
whose soft assignments a PointNet-style network predicts from rotation-invariant (RRI) features (reference: models/deepgmr.py;
examples/test_deepgmr.py).  gmm_params, gmm_register, Conv1dBNReLU, FCBNReLU, TNet, PointNet and DeepGMR keep the reference's names,
attribute names and state_dict keys (backbone.encoder.{0..3}.{0,1}.*, backbone.decoder.{0..2}.{0,1}.*, backbone.decoder.3.*, and
backbone.tnet.* with use_tnet: 44 entries without), so its checkpoints load with strict=True.

The reference's module cannot run as written; what is changed, and only that:
  * PointNet(use_rri, use_tnet=False, nearest_neighbors=20, d_model=1024, n_clusters=16) and DeepGMR(use_rri=True,
    feature_model=None, nearest_neighbors=20, d_model=1024, n_clusters=16): the two trailing keywords replace the undefined global
    `args` (:111-116); their defaults are the DeepGMR paper's.
  * feature_model=None builds a fresh PointNet.  The reference's `feature_model if not None else ...` (:130) always takes the
    argument, None included.
  * forward reads self.est_T / self.est_T_inverse where the reference reads the undefined names est_T / est_T_inverse (:154-161), and
    does not set self.igt (:152 reads an undefined `igt`).  The key 'est_t_inverese' is kept as spelt.
  * 'transformed_source' transforms self.source, the first three columns.  The reference passes the whole `source`, RRI columns
    included (:154), which cannot be multiplied by a 3x3 rotation.
  * gmm_params / gmm_register build their constants (eye, the bottom row) in the input's dtype and on its device, so `.double()`
    works; the reference builds fp32 ones (:27, :48, :52).  gmm_register runs its SVD on the tensor's own device; the reference
    moves Ms to the host and back (:45-47).  gmm_params squeezes the two matrix dimensions by name; the reference's bare
    `.squeeze()` (:29) also drops a batch of one.
  * with use_rri=True an input [B,N,3] is accepted beside the reference's [B,N,3+4k]: the features are then computed on the fly
    from the centred cloud (data_utils.rri_features), as the reference's dataset computes them on the host.
With use_rri=False the network's input is `x - x.mean(dim=2, keepdim=True)` exactly as the reference writes it (:142-143): a mean
over the COORDINATE axis (x + y + z) / 3 of each point, not the cloud's centroid.

With device fp32 clouds, BatchNorm on running statistics, nothing to differentiate and use_tnet=False (FUSED and _fused.fusable):
  * both clouds as one batch of 2B (two clouds of different sizes raise ValueError on every route: the reference's residual 'r'
    subtracts their feature tensors, :162, and fails there),
  * the encoder's four folded Conv+BN+ReLU layers on the conv kernels (_fused.pointwise_conv), the first reading the features
    channel-last as they arrive; the pooled maximum of the last one,
  * decoder[0] over the local features alone: f_glob is the same for every point, so bn(W [f_loc ; f_glob]) =
    scale (W[:, :d] f_loc) + (scale (W[:, d:] f_glob) + shift), a per-cloud shift from l3d_linear_rows -- no [B,2d,N] tensor,
  * decoder[1..3] folded; the logits stay channel-first [2B,J,N] and go straight into l3d_gmm_params (softmax over J, pi, mu and
    the isotropic variance about the computed mean; no [B,N,J,3] tensor), then l3d_gmm_register twice (the 3x3 SVD on the device),
  * no host read anywhere.
Anything else (CPU tensors, other dtypes, autograd, train-mode BatchNorm, use_tnet) takes the reference's op sequence in torch.
_lib.LAUNCH_LOG shows the route: l3d_gmm_params / l3d_gmm_register appear on the fused one only."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .._lib import call, f32c, on_device_of
from ..data_utils.rri import rri_features
from . import _fused

FUSED = True                 # False: the op sequence for every input (A/B: tools/deepgmr_bench.py)


def gmm_params(gamma, pts):
    """the op-sequence GMM fit (:13-31): soft assignments gamma [B,N,J] and points pts [B,N,3] -> weights pi [B,J], means mu [B,J,3]
    and isotropic covariances sigma [B,J,3,3] = var * eye, var the assignment-weighted mean of |p - mu|^2 about the computed mean.
    Differentiable, any dtype and device; it goes through the [B,N,J,3] differences, which l3d_gmm_params (gmm_fit) never forms."""
    pi = gamma.mean(dim=1)
    Npi = pi * gamma.shape[1]                                      # the assignments' mass per component
    mu = gamma.transpose(1, 2) @ pts / Npi.unsqueeze(2)
    diff = pts.unsqueeze(2) - mu.unsqueeze(1)                      # every point against every mean
    eye = torch.eye(3, dtype=gamma.dtype, device=gamma.device).unsqueeze(0).unsqueeze(1)
    sigma = (
        ((diff.unsqueeze(3) @ diff.unsqueeze(4)).squeeze(4).squeeze(3) * gamma).sum(dim=1) / Npi
    ).unsqueeze(2).unsqueeze(3) * eye
    return pi, mu, sigma


def gmm_fit(logits, pts, want_gamma=True):
    """l3d_gmm_params: logits [B,J,N] channel-first, pts [B,N,3] (device fp32) -> (gamma [B,N,J] or None, pi [B,J], mu [B,J,3],
    var [B,J]) with gamma = softmax over J and var the scalar of the reference's sigma = var * eye"""
    logits, pts = f32c(logits), f32c(pts)
    B, J, N = logits.shape
    dev = logits.device
    gamma = torch.empty((B, N, J), dtype=torch.float32, device=dev) if want_gamma else None
    pi = torch.empty((B, J), dtype=torch.float32, device=dev)
    mu = torch.empty((B, J, 3), dtype=torch.float32, device=dev)
    var = torch.empty((B, J), dtype=torch.float32, device=dev)
    call("l3d_gmm_params", logits, pts, B, J, N, gamma, pi, mu, var)
    return gamma, pi, mu, var


def gmm_register_fused(pi_s, mu_s, mu_t, var_t):
    """l3d_gmm_register: pi_s [B,J], mu_s, mu_t [B,J,3], var_t [B,J] (device fp32) -> T [B,4,4]"""
    pi_s, mu_s, mu_t, var_t = f32c(pi_s), f32c(mu_s), f32c(mu_t), f32c(var_t)
    B, J = pi_s.shape
    T = torch.empty((B, 4, 4), dtype=torch.float32, device=pi_s.device)
    call("l3d_gmm_register", pi_s, mu_s, mu_t, var_t, B, J, T)
    return T


def gmm_register(pi_s, mu_s, mu_t, sigma_t):
    """the op-sequence registration of two mixtures that share the weights pi_s [B,J] (:34-54): means mu_s, mu_t [B,J,3], target
    covariances sigma_t [B,J,3,3] -> T [B,4,4] mapping the s mixture onto the t mixture.  Kabsch on the weighted, covariance-scaled
    cross-covariance Ms, with the sign of det(V U^T) on the last singular direction.  Differentiable through torch.svd."""
    c_s = pi_s.unsqueeze(1) @ mu_s
    c_t = pi_s.unsqueeze(1) @ mu_t
    Ms = torch.sum((pi_s.unsqueeze(2) * (mu_s - c_s)).unsqueeze(3) @
                   (mu_t - c_t).unsqueeze(2) @ sigma_t.inverse(), dim=1)
    U, _, V = torch.svd(Ms)
    S = torch.eye(3, dtype=U.dtype, device=U.device).unsqueeze(0).repeat(U.shape[0], 1, 1)
    S[:, 2, 2] = torch.det(V @ U.transpose(1, 2))
    R = V @ S @ U.transpose(1, 2)
    t = c_t.transpose(1, 2) - R @ c_s.transpose(1, 2)
    bot_row = torch.tensor([[[0, 0, 0, 1]]], dtype=R.dtype, device=R.device).repeat(R.shape[0], 1, 1)
    T = torch.cat([torch.cat([R, t], dim=2), bot_row], dim=1)
    return T


class Conv1dBNReLU(nn.Sequential):
    def __init__(self, in_planes, out_planes):
        super(Conv1dBNReLU, self).__init__(
            nn.Conv1d(in_planes, out_planes, kernel_size=1, bias=False),
            nn.BatchNorm1d(out_planes),
            nn.ReLU(inplace=True))

    def fused(self, x, channel_last=False):
        """the folded Conv+BN+ReLU on the conv kernels: x [B,Cin,N] (or [B,N,Cin]) -> [B,Cout,N]"""
        w, scale, shift = _fused.fold_conv_bn(self[0], self[1])
        return _fused.pointwise_conv(x, w, scale, shift, relu=True, channel_last=channel_last)


class FCBNReLU(nn.Sequential):
    def __init__(self, in_planes, out_planes):
        super(FCBNReLU, self).__init__(
            nn.Linear(in_planes, out_planes, bias=False),
            nn.BatchNorm1d(out_planes),
            nn.ReLU(inplace=True))


class TNet(nn.Module):
    def __init__(self):
        super(TNet, self).__init__()
        self.encoder = nn.Sequential(
            Conv1dBNReLU(3, 64),
            Conv1dBNReLU(64, 128),
            Conv1dBNReLU(128, 256))
        self.decoder = nn.Sequential(
            FCBNReLU(256, 128),
            FCBNReLU(128, 64),
            nn.Linear(64, 6))

    @staticmethod
    def f2R(f):
        r1 = F.normalize(f[:, :3])
        proj = (r1.unsqueeze(1) @ f[:, 3:].unsqueeze(2)).squeeze(2)
        r2 = F.normalize(f[:, 3:] - proj * r1)
        r3 = torch.cross(r1, r2, dim=1)
        return torch.stack([r1, r2, r3], dim=2)

    def forward(self, pts):
        f = self.encoder(pts)
        f, _ = f.max(dim=2)
        f = self.decoder(f)
        R = self.f2R(f)
        return R @ pts


class PointNet(nn.Module):
    def __init__(self, use_rri, use_tnet=False, nearest_neighbors=20, d_model=1024, n_clusters=16):
        super(PointNet, self).__init__()
        self.use_tnet = use_tnet
        self.tnet = TNet() if self.use_tnet else None
        d_input = nearest_neighbors * 4 if use_rri else 3
        self.d_model = d_model
        self.encoder = nn.Sequential(
            Conv1dBNReLU(d_input, 64),
            Conv1dBNReLU(64, 128),
            Conv1dBNReLU(128, 256),
            Conv1dBNReLU(256, d_model))
        self.decoder = nn.Sequential(
            Conv1dBNReLU(d_model * 2, 512),
            Conv1dBNReLU(512, 256),
            Conv1dBNReLU(256, 128),
            nn.Conv1d(128, n_clusters, kernel_size=1))

    def forward(self, pts):
        # channel-first features [B,d_input,N] in, one row of n_clusters logits per point out
        pts = self.tnet(pts) if self.use_tnet else pts
        f_loc = self.encoder(pts)
        f_glob, _ = f_loc.max(dim=2)
        f_glob = f_glob.unsqueeze(2).expand_as(f_loc)
        y = self.decoder(torch.cat([f_loc, f_glob], dim=1))
        return y.transpose(1, 2)

    def fusable(self, *tensors):
        """the fused route's gate: FUSED, no TNet, device fp32 tensors, BatchNorm on running statistics, nothing to differentiate"""
        return FUSED and not self.use_tnet and _fused.fusable(self, *tensors)

    def fused(self, x, channel_last=False):
        """x [R,d_input,N] (or [R,N,d_input]) -> the logits channel-first [R,n_clusters,N]: no transpose, no [R,2d,N] tensor"""
        f = self.encoder[0].fused(f32c(x), channel_last)
        for layer in list(self.encoder)[1:]:
            f = layer.fused(f)
        d0, last = self.decoder[0], self.decoder[3]
        wl, wg, scale, shift = _fused.conv_column_blocks(d0[0], d0[1], f.shape[1], scale_block=1)      # wg carries the BN scale
        y = _fused.pointwise_conv(f, wl, scale, _fused.rows_affine(f.amax(dim=2), wg, shift), relu=True)
        y = self.decoder[2].fused(self.decoder[1].fused(y))
        w, _, bias = _fused.fold_conv_bn(last)
        return _fused.pointwise_conv(y, w, None, bias, relu=False)


def _transform(points, T):
    """ops/transform_functions.py:24-29 with a rotation matrix: points [B,N,3], T [B,4,4] -> R p + t"""
    return (torch.matmul(T[:, :3, :3], points.permute(0, 2, 1)) + T[:, :3, 3].unsqueeze(2)).permute(0, 2, 1)


class DeepGMR(nn.Module):
    def __init__(self, use_rri=True, feature_model=None, nearest_neighbors=20, d_model=1024, n_clusters=16):
        super(DeepGMR, self).__init__()
        self.backbone = feature_model if feature_model is not None else PointNet(
            use_rri=use_rri, nearest_neighbors=nearest_neighbors, d_model=d_model, n_clusters=n_clusters)
        self.use_rri = use_rri
        self.nearest_neighbors = nearest_neighbors

    def _features(self, cloud):
        """the network's input of one cloud, channel-last [B,N,C] (the reference transposes it; so does the op sequence below)"""
        if not self.use_rri:
            return cloud - cloud.mean(dim=2, keepdim=True)         # the reference's mean over the coordinate axis (:142-143)
        if cloud.shape[-1] == 3:
            return rri_features(cloud, self.nearest_neighbors, center=True)      # in the cloud's own dtype
        return cloud[..., 3:]

    def forward(self, template, source):
        if self.use_rri:
            self.template = template[..., :3]
            self.source = source[..., :3]
        else:
            self.template = template
            self.source = source
        template_features = self._features(template)
        source_features = self._features(source)
        if template_features.shape != source_features.shape:
            # the reference fails in the same place, later: its residual 'r' subtracts the two feature tensors (:162)
            raise ValueError(f"DeepGMR takes two clouds of one size (its residual 'r' is their features' difference), got "
                             f"{tuple(template.shape)} and {tuple(source.shape)}")

        fusable = getattr(self.backbone, "fusable", None)
        if fusable is not None and fusable(template, source):
            with on_device_of(template, source):
                self._fit_fused(template_features, source_features)
        else:
            self.template_gamma = F.softmax(self.backbone(template_features.transpose(1, 2)), dim=2)
            self.template_pi, self.template_mu, self.template_sigma = gmm_params(self.template_gamma, self.template)
            self.source_gamma = F.softmax(self.backbone(source_features.transpose(1, 2)), dim=2)
            self.source_pi, self.source_mu, self.source_sigma = gmm_params(self.source_gamma, self.source)

            self.est_T_inverse = gmm_register(self.template_pi, self.template_mu, self.source_mu, self.source_sigma)
            self.est_T = gmm_register(self.source_pi, self.source_mu, self.template_mu, self.template_sigma)      # maps the source onto the template

        est_T, est_T_inverse = self.est_T, self.est_T_inverse
        transformed_source = _transform(self.source, est_T)

        result = {'est_R': est_T[:, :3, :3],
                  'est_t': est_T[:, :3, 3],
                  'est_R_inverse': est_T_inverse[:, :3, :3],
                  'est_t_inverese': est_T_inverse[:, :3, 3],
                  'est_T': est_T,
                  'est_T_inverse': est_T_inverse,
                  'r': template_features.transpose(1, 2) - source_features.transpose(1, 2),
                  'transformed_source': transformed_source}

        return result

    def _fit_fused(self, template_features, source_features):
        net = self.backbone
        B = template_features.shape[0]
        eye = torch.eye(3, dtype=torch.float32, device=template_features.device)
        logits = net.fused(torch.cat([template_features, source_features], dim=0), channel_last=True)         # [2B,J,N]
        gamma, pi, mu, var = gmm_fit(logits, torch.cat([self.template, self.source], dim=0))
        self.template_gamma, self.template_pi, self.template_mu, tvar = gamma[:B], pi[:B], mu[:B], var[:B]
        self.source_gamma, self.source_pi, self.source_mu, svar = gamma[B:], pi[B:], mu[B:], var[B:]
        self.template_sigma = tvar[:, :, None, None] * eye
        self.source_sigma = svar[:, :, None, None] * eye
        self.est_T_inverse = gmm_register_fused(self.template_pi, self.template_mu, self.source_mu, svar)
        self.est_T = gmm_register_fused(self.source_pi, self.source_mu, self.template_mu, tvar)
