"""SE(3) helpers the iterative registration models call (reference: ops/se3.py:51-122, ops/sinc.py): Exp / exp, transform, inverse.
Plain torch on any device and dtype -- this is the op-sequence route; on the fused route the same arithmetic runs inside
registration.hip (csrc/se3_exp.h).  `log`, the Lie bracket and the so3 module are not needed by the models and are not here."""
import torch


def _sincs(t):
    """sin(t)/t, (1 - cos t)/t^2, (t - sin t)/t^3 with the Taylor branch of ops/sinc.py below |t| = 0.01"""
    small = t.abs() < 0.01
    t2 = t * t
    ts = torch.where(small, torch.ones_like(t), t)            # a safe denominator where the Taylor branch is taken
    ts2 = ts * ts
    s1 = torch.where(small, 1 - t2 / 6 * (1 - t2 / 20 * (1 - t2 / 42)), torch.sin(ts) / ts)
    s2 = torch.where(small, 1 / 2 * (1 - t2 / 12 * (1 - t2 / 30 * (1 - t2 / 56))), (1 - torch.cos(ts)) / ts2)
    s3 = torch.where(small, 1 / 6 * (1 - t2 / 20 * (1 - t2 / 42 * (1 - t2 / 72))), (ts - torch.sin(ts)) / (ts ** 3))
    return s1, s2, s3


def _hat(w):
    """[M,3] -> the skew matrices [M,3,3]"""
    o = torch.zeros_like(w[:, 0])
    return torch.stack((torch.stack((o, -w[:, 2], w[:, 1]), dim=1),
                        torch.stack((w[:, 2], o, -w[:, 0]), dim=1),
                        torch.stack((-w[:, 1], w[:, 0], o), dim=1)), dim=1)


def exp(x):
    """twists [*,6] = (w, v) -> [*,4,4]: R = I + sinc1 W + sinc2 W^2, p = (I + sinc2 W + sinc3 W^2) v  (Rodrigues)"""
    x_ = x.reshape(-1, 6)
    w, v = x_[:, 0:3], x_[:, 3:6]
    t = w.norm(p=2, dim=1).view(-1, 1, 1)
    W = _hat(w)
    S = W.bmm(W)
    eye = torch.eye(3, dtype=x.dtype, device=x.device)
    s1, s2, s3 = _sincs(t)
    R = eye + s1 * W + s2 * S
    V = eye + s2 * W + s3 * S
    p = V.bmm(v.contiguous().view(-1, 3, 1))
    bottom = torch.tensor([0, 0, 0, 1], dtype=x.dtype, device=x.device).view(1, 1, 4).repeat(x_.size(0), 1, 1)
    g = torch.cat((torch.cat((R, p), dim=2), bottom), dim=1)
    return g.view(*x.shape[:-1], 4, 4)


def _generators(like):
    """the six generators of se(3) as [6,4,4]"""
    return _hat_se3(torch.eye(6, dtype=like.dtype, device=like.device))


def _hat_se3(x):
    x_ = x.reshape(-1, 6)
    X = torch.zeros((x_.size(0), 4, 4), dtype=x.dtype, device=x.device)
    X[:, 0:3, 0:3] = _hat(x_[:, 0:3])
    X[:, 0:3, 3] = x_[:, 3:6]
    return X


class ExpMap(torch.autograd.Function):
    """exp with the reference's gradient (ops/se3.py:135-165): d exp(x) / d x_k is taken as gen_k exp(x), the derivative of the
    left perturbation, which is what the reference's trained models were differentiated with."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return exp(x)

    @staticmethod
    def backward(ctx, grad_output):
        x, = ctx.saved_tensors
        g = exp(x)
        dg = _generators(x).matmul(g.reshape(-1, 1, 4, 4)).to(grad_output)          # [M,6,4,4]
        return (grad_output.contiguous().view(-1, 1, 4, 4) * dg).sum(-1).sum(-1).view_as(x)


Exp = ExpMap.apply


def inverse(g):
    """[*,4,4] rigid transforms -> their inverses [R^T | -R^T p]"""
    g_ = g.reshape(-1, 4, 4)
    Q = g_[:, 0:3, 0:3].transpose(1, 2)
    q = -Q.matmul(g_[:, 0:3, 3].unsqueeze(-1))
    bottom = torch.tensor([0, 0, 0, 1], dtype=g.dtype, device=g.device).view(1, 1, 4).repeat(g_.size(0), 1, 1)
    return torch.cat((torch.cat((Q, q), dim=2), bottom), dim=1).view(*g.shape[:-2], 4, 4)


def transform(g, a):
    """g [*,4,4] applied to a: a [*,3,N] when g and a have the same number of axes, else points a [*,N,3] (g broadcast)"""
    g_ = g.reshape(-1, 4, 4)
    R = g_[:, 0:3, 0:3].contiguous().view(*g.shape[:-2], 3, 3)
    p = g_[:, 0:3, 3].contiguous().view(*g.shape[:-2], 3)
    if g.dim() == a.dim():
        return R.matmul(a) + p.unsqueeze(-1)
    return R.matmul(a.unsqueeze(-1)).squeeze(-1) + p
