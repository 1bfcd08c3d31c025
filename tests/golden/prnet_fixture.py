"""Reader of prnet_seeded.npz (make_golden_prnet.py wrote it from the reference), and what the generator and the tests share: the
case table, the clouds, the models rebuilt from the stored seed, the rescaling applied to their seeded weights and the hooks that
collect a run's quantities.

The reference cannot run its whole forward in fp64, so the fp64 truth has two parts: `temperature`, `disparity` and `emb_k_src` are
the reference's own predict_embedding in fp64; the head and loop quantities come from this package's CPU op sequence in fp64
(`reference64`), which tests/test_prnet_cpu.py first holds to 1e-9 against everything the reference computed in fp64.  Every gap
is max |reference fp32 - fp64|."""
import copy
import functools
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from seeded import seeded_params    # noqa: E402

SAMPLES = 2048
GAP_FACTOR = 4.0
B = 2
#         name  emb_nn      attention      emb  N    K    iters  temp_net.nn[9].bias  ground truth
CASES = (("m1", "dgcnn", "transformer", 64, 64, 32, 3, 5.0, False),
         ("m2", "dgcnn", "transformer", 64, 48, 48, 3, 20.0, False),
         ("m3", "dgcnn", "transformer", 512, 256, 128, 1, 5.0, False),
         ("m4", "pointnet", "identity", 64, 64, 32, 2, 20.0, True))
HEAD0 = ("R_ab0", "t_ab0", "R_ba0", "t_ba0")                       # the head's outputs in iteration 0
EMBED0 = ("temperature", "disparity", "emb_k_src")                 # the reference's predict_embedding, iteration 0
FINAL = ("est_R", "est_t", "transformed_source", "loss")


def case(name):
    return next((i, c) for i, c in enumerate(CASES) if c[0] == name)


def rescale(net, bias):
    """temp_net.nn[9].bias <- bias: with seeded weights the temperature head lands on its lower clamp (0.01), the softmax is nearly
    uniform and H's singular values are 1e-3 .. 1e-5, so a whole-model comparison measures noise.  With the bias at 5 / 20 the
    temperature is about 5 / 20, inside the clamp, and the softmax is peaked.  (BatchNorm statistics and affine parameters are
    already randomised by seeded_params.)"""
    with torch.no_grad():
        net.temp_net.nn[9].bias.fill_(bias)
    return net


def clouds(name, seed):
    """-> src, tgt [B,N,3] fp32, rotation_ab [B,3,3], translation_ab [B,3]: src is the rotated (<= 45 degrees per axis), translated
    and permuted target, and (rotation_ab, translation_ab) takes src back onto tgt"""
    i, (_, _, _, _, N, _, _, _, _) = case(name)
    g = torch.Generator().manual_seed(seed + 1000 + i)
    tgt = torch.rand((B, N, 3), generator=g) - 0.5
    ang = (torch.rand((B, 3), generator=g) * 2 - 1) * (math.pi / 4)
    t = torch.rand((B, 3), generator=g) - 0.5
    c, s = torch.cos(ang).double(), torch.sin(ang).double()
    one, zero = torch.ones(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    Rx = torch.stack([one, zero, zero, zero, c[:, 0], -s[:, 0], zero, s[:, 0], c[:, 0]], 1).view(B, 3, 3)
    Ry = torch.stack([c[:, 1], zero, s[:, 1], zero, one, zero, -s[:, 1], zero, c[:, 1]], 1).view(B, 3, 3)
    Rz = torch.stack([c[:, 2], -s[:, 2], zero, s[:, 2], c[:, 2], zero, zero, zero, one], 1).view(B, 3, 3)
    R = Rz @ Ry @ Rx
    src = torch.stack([(tgt[b].double() @ R[b].T + t[b].double())[torch.randperm(N, generator=g)] for b in range(B)])
    Rab = R.transpose(1, 2)
    tab = -(Rab @ t.double().unsqueeze(2)).squeeze(2)
    return src.float().contiguous(), tgt.contiguous(), Rab.float().contiguous(), tab.float().contiguous()


def build_model(cls, name, seed, **kw):
    """the case's PRNet from class cls (the reference's or this package's: same arguments and keys), seeded and rescaled, eval mode"""
    i, (_, emb_nn, attention, emb, N, K, iters, bias, _) = case(name)
    net = cls(emb_nn=emb_nn, attention=attention, head="svd", emb_dims=emb, num_keypoints=K, num_subsampled_points=N, num_iters=iters, **kw)
    return rescale(seeded_params(net, seed + 50 + 10 * i), bias).eval()


def sampled(v):
    flat = v.reshape(-1)
    return flat[::-(-flat.numel() // SAMPLES)] if flat.numel() > SAMPLES else flat


def matched_indices(before, after):
    """the ascending indices n with before[b,:,n] a column of after [B,C,K] (how the generator reads a KeyPointNet's choice off its
    inputs and outputs, whatever order it gathered in)"""
    hit = (before[:, :, :, None] == after[:, :, None, :]).all(dim=1).any(dim=2)            # [B,N]
    return torch.stack([h.nonzero().view(-1) for h in hit])


class Hooks:
    """collects, while a PRNet (the reference's or this package's op-sequence route) runs: every head call's inputs and outputs,
    every temp_net call's outputs and every KeyPointNet call's inputs and outputs"""

    def __init__(self, net):
        self.net, self.head, self.temp, self.kp, self.handles = net, [], [], [], []

    def __enter__(self):
        n = self.net
        self.handles = [n.head.register_forward_hook(lambda m, a, out: self.head.append((a, out))),
                        n.temp_net.register_forward_hook(lambda m, a, out: self.temp.append(out))]
        if hasattr(n.keypointnet, "num_keypoints"):
            self.handles.append(n.keypointnet.register_forward_hook(lambda m, a, out: self.kp.append((a, out))))
        return self

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()
        return False

    def keypoint_sets(self):
        """per iteration: (src indices, tgt indices) [B,K] ascending"""
        return [(matched_indices(a[2], out[2]), matched_indices(a[3], out[3])) for a, out in self.kp]

    def quantities(self, result=None):
        d = lambda t: t.detach()
        q = {"temperature": d(self.temp[0][0]).reshape(-1), "disparity": d(self.temp[0][1])}
        q["emb_k_src"] = None
        if self.kp:                                            # the chosen columns in ascending index order, whatever order the run gathered in
            before, after = d(self.kp[0][0][2]), d(self.kp[0][1][2])
            q["emb_k_src"] = torch.gather(before, 2, matched_indices(before, after)[:, None, :].expand(-1, before.shape[1], -1))
        if self.head:
            (_, (Rab, tab)), (_, (Rba, tba)) = self.head[0], self.head[1]
            q.update(R_ab0=d(Rab), t_ab0=d(tab), R_ba0=d(Rba), t_ba0=d(tba))
        for it, out in enumerate(self.temp):
            q[f"temperature_it{it}"] = d(out[0]).reshape(-1)
        if result is not None:
            q.update({k: d(result[k]) for k in FINAL if k in result})
        return q


def head_H(src_emb, tgt_emb, src, tgt, temperature):
    """the 3 x 3 matrix whose SVD the head takes, from a head call's inputs (for the generator's singular-value screen)"""
    Bn = src.shape[0]
    scores = torch.softmax(temperature.view(Bn, 1, 1) * (src_emb.transpose(2, 1) @ tgt_emb) / math.sqrt(src_emb.shape[1]), dim=2)
    corr = tgt @ scores.transpose(2, 1)
    return (src - src.mean(dim=2, keepdim=True)) @ (corr - corr.mean(dim=2, keepdim=True)).transpose(2, 1)


def run(net, name, src, tgt, Rab=None, tab=None):
    """one forward under the hooks -> the quantities of the module text"""
    with Hooks(net) as h:
        out = net(src, tgt, Rab, tab) if Rab is not None else net(src, tgt)
    return h.quantities(out), h


# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def load():
    return dict(np.load(os.path.join(HERE, "prnet_seeded.npz")))


def seed():
    return int(load()["seed"])


def stored(key):
    return torch.from_numpy(np.asarray(load()[key]))


def gap(key):
    return float(load()[key + "_gap"])


def inputs(name):
    """src, tgt and, for a case with ground truth, rotation_ab and translation_ab (else None, None)"""
    src, tgt, Rab, tab = clouds(name, seed())
    return (src, tgt, Rab, tab) if case(name)[1][8] else (src, tgt, None, None)


def model(name, **kw):
    """the case's model in fp32 on the CPU, as the generator built the reference's"""
    from learning3d_amd.models.prnet import PRNet
    return build_model(PRNet, name, seed(), **kw)


def quantities(name):
    """the names stored for a case"""
    return [q for q in EMBED0 + HEAD0 + FINAL if f"{name}_{q}_gap" in load()]


@functools.lru_cache(maxsize=None)
def reference64(name):
    """this package's op sequence in fp64 on the CPU -> (quantities, per-iteration keypoint indices, the inputs of the head's first
    call: src_emb_k, tgt_emb_k, src_k, tgt_k, temperature)"""
    net = copy.deepcopy(model(name)).double()
    net.keypoint_log = []
    with torch.no_grad():
        q, h = run(net, name, *[None if t is None else t.double() for t in inputs(name)])
    return q, net.keypoint_log, tuple(t.detach() for t in h.head[0][0])


def truth(name, q):
    """the fp64 truth of a stored quantity: the reference's own where it has one (EMBED0; emb_k_src whole from reference64, whose
    samples test_prnet_cpu.py holds to 1e-9 against the stored ones), reference64 else"""
    if q in ("temperature", "disparity"):
        return stored(f"{name}_{q}_64").reshape(reference64(name)[0][q].shape)         # (stored flat)
    return reference64(name)[0][q]


def err(got, want64):
    return float((got.detach().cpu().double() - want64).abs().max())
