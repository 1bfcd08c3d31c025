"""Drop-in for learning3d/models/pcrnet.py on MI355X: iPCRNet, PointNet features of template and source -> a six-layer head -> a
pose (quaternion, translation) per iteration.  Same constructor arguments (`droput` is the reference's spelling), attribute names
and state_dict keys (`feature_model.*`, `linear.0.weight` ... `linear.10.weight`).

The FUSED route (device fp32 clouds, eval-mode BatchNorm / Dropout, nothing to differentiate) keeps one accumulated pose on the
device: each iteration poses the ORIGINAL source by it inside PointNet's first-layer kernel, runs the head on l3d_linear_rows and
folds the new quaternion into the pose in one launch (registration.hip); no host read anywhere.  The OP-SEQUENCE route is the
reference's operations in plain torch (CPU, autograd, train mode).  pointnetlk.FUSED_LOOP = False disables the fused route here
too.  The default feature_model is built per instance, not once at import."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _fused
from . import _registration as _reg
from . import pointnetlk as _switch
from .pointnet import PointNet
from .pooling import Pooling


def _qrot(q, v):
    """v [..,3] rotated by unit quaternions q [..,4] (w x y z): v + 2 (w (u x v) + u x (u x v))"""
    u = q[..., 1:]
    uv = torch.cross(u, v, dim=-1)
    uuv = torch.cross(u, uv, dim=-1)
    return v + 2 * (q[..., :1] * uv + uuv)


class iPCRNet(nn.Module):
    def __init__(self, feature_model=None, droput=0.0, pooling='max'):
        super().__init__()
        self.feature_model = feature_model if feature_model is not None else PointNet()
        self.pooling = Pooling(pooling)
        layers = [nn.Linear(self.feature_model.emb_dims * 2, 1024), nn.ReLU(),
                  nn.Linear(1024, 1024), nn.ReLU(),
                  nn.Linear(1024, 512), nn.ReLU(),
                  nn.Linear(512, 512), nn.ReLU(),
                  nn.Linear(512, 256), nn.ReLU()]
        if droput > 0.0:
            layers.append(nn.Dropout(droput))
        layers.append(nn.Linear(256, 7))
        self.linear = nn.Sequential(*layers)

    # ------------------------------------------------------------------ op-sequence route
    def spam(self, template_features, source, est_R, est_t):
        """one alignment pass: the head's pose from (template, current source) features, folded into est_R / est_t and applied"""
        B, N = source.size(0), source.size(1)
        self.source_features = self.pooling(self.feature_model(source))
        pose = self.linear(torch.cat([template_features, self.source_features], dim=1))
        q = F.normalize(pose[:, 0:4], dim=1)
        t = pose[:, 4:]
        eye = torch.eye(3).to(source).view(1, 3, 3).expand(B, 3, 3).contiguous()
        R = _qrot(q.unsqueeze(1).expand(-1, 3, -1).contiguous(), eye).permute(0, 2, 1)      # rows of qrot(identity) are R's columns
        est_t = torch.bmm(R, est_t.permute(0, 2, 1)).permute(0, 2, 1) + t.view(-1, 1, 3)
        est_R = torch.bmm(R, est_R)
        source = _qrot(q.unsqueeze(1).expand(-1, N, -1).contiguous(), source) + t.view(-1, 1, 3).repeat(1, N, 1)
        return est_R, est_t, source

    def forward(self, template, source, max_iteration=8):
        if _switch.FUSED_LOOP and max_iteration >= 1 and self._head_fusable() and \
                _reg.usable(self, self.feature_model, self.pooling, template, source):
            return self.fused_forward(template, source, max_iteration)
        B = template.size(0)
        est_R = torch.eye(3).to(template).view(1, 3, 3).expand(B, 3, 3).contiguous()
        est_t = torch.zeros(1, 3).to(template).view(1, 1, 3).expand(B, 1, 3).contiguous()
        template_features = self.pooling(self.feature_model(template))
        for _ in range(max_iteration):
            est_R, est_t, source = self.spam(template_features, source, est_R, est_t)
        bottom = torch.tensor([[[0.0, 0.0, 0.0, 1.0]]]).repeat(B, 1, 1).to(est_R)
        est_T = torch.cat([torch.cat([est_R, est_t[:, 0, :].unsqueeze(-1)], dim=2), bottom], dim=1)
        return {'est_R': est_R, 'est_t': est_t, 'est_T': est_T, 'r': template_features - self.source_features,
                'transformed_source': source}

    # ------------------------------------------------------------------ fused route
    def _head_fusable(self):
        return all(isinstance(m, (nn.Linear, nn.ReLU, nn.Dropout)) for m in self.linear) and \
            all(m.in_features % 256 == 0 for m in self.linear if isinstance(m, nn.Linear))

    def _head(self, y):
        mods = list(self.linear)
        for i, m in enumerate(mods):
            if isinstance(m, nn.Linear):
                y = _fused.linear_rows(y, m, relu=i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU))
        return y

    def fused_forward(self, template, source, max_iteration):
        """launches only (capturable in one graph); the accumulated pose est_T poses the original source each iteration"""
        template, source = _reg.prepare(template, source)
        B = template.shape[0]
        dev = template.device
        eyeT = _reg.identity(B, dev).view(B, 1, 4, 4)
        est_R = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
        est_t = torch.empty((B, 1, 3), dtype=torch.float32, device=dev)
        est_T = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
        f_t, _ = _reg.posed_features(self.feature_model, template, T=eyeT)
        for i in range(max_iteration):
            f_s, _ = _reg.posed_features(self.feature_model, source, T=eyeT if i == 0 else est_T.view(B, 1, 4, 4))
            pose7 = self._head(torch.cat([f_t, f_s], dim=1))
            _reg.quat_update(pose7, i == 0, est_R, est_t, est_T)
        self.source_features = f_s
        _, posed = _reg.posed_features(self.feature_model, source, T=est_T.view(B, 1, 4, 4), want_features=False, want_cloud=True)
        return {'est_R': est_R, 'est_t': est_t, 'est_T': est_T, 'r': f_t - f_s, 'transformed_source': posed}
