"""Reader of rpmnet_seeded.npz (make_golden_rpmnet.py wrote it from the reference): the cases' inputs, the models rebuilt from
the stored seed, the stored fp64 values and gaps, and the sampling rule of the large tensors.

The large tensors ([B,J,K] matrices, grouped features, layer outputs) are stored as fp64 samples flat[::stride]; `reference64`
rebuilds them whole by running this package's op sequence in fp64 on the CPU.  tests/test_rpmnet_cpu.py holds that run to 1e-9
against everything stored, samples included, before any other test leans on it."""
import functools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from seeded import seeded_params    # noqa: E402

SAMPLES = 2048
GAP_FACTOR = 4.0


@functools.lru_cache(maxsize=None)
def load():
    return dict(np.load(os.path.join(HERE, "rpmnet_seeded.npz")))


def cases():
    fx = load()
    return {str(n): (int(k), int(i), bool(nm)) for n, k, i, nm in zip(fx["cases"], fx["case_K"], fx["case_iters"], fx["case_normals"])}


def sampled(v):
    flat = v.reshape(-1)
    return flat[::-(-flat.numel() // SAMPLES)]


def build(name, **ppf_kw):
    """the case's model in fp32 on the CPU, as the generator built the reference's"""
    from learning3d_amd.models import PPFNet, RPMNet
    fx = load()
    K = cases()[name][0]
    net = seeded_params(RPMNet(feature_model=PPFNet(num_neighbors=K, **ppf_kw)), int(fx["seed"])).eval()
    with torch.no_grad():
        for m in net.feat_extractor.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.mul_(float(fx["gn_factor"]))
        if name == "a":
            net.weights_net.postpool[-1].bias[0] = float(fx["beta_bias"])
    return net


def inputs(name):
    fx = load()
    t, s = torch.from_numpy(fx["template"]), torch.from_numpy(fx["source"])
    if not cases()[name][2]:
        t, s = t[:, :, :3], s[:, :, :3]
    return t.contiguous(), s.contiguous()


@functools.lru_cache(maxsize=None)
def reference64(name):
    """the whole result dict of the case in fp64: this package's op sequence on the CPU (held to the stored values by the CPU tests)"""
    import copy
    t, s = inputs(name)
    with torch.no_grad():
        return copy.deepcopy(build(name)).double()(t.double(), s.double(), cases()[name][1])


def stored(key):
    return torch.from_numpy(np.asarray(load()[key]))


def pooled_gap(suffix, names=None):
    """the largest gap over the fixture's cases of one kind: keys `<case>_<suffix><iteration>_gap`"""
    import re
    names = list(cases()) if names is None else names
    vals = [float(v) for k, v in load().items() if any(re.fullmatch(rf"{n}_{suffix}\d*_gap", k) for n in names)]
    assert vals, suffix
    return max(vals)


def model_errors(result, name):
    """-> {quantity: error of `result` against the fp64 reference}; perm_matrices_init relative"""
    ref = reference64(name)
    err = lambda a, b: float((torch.as_tensor(a).detach().cpu().double() - torch.as_tensor(b)).abs().max())       # noqa: E731
    out = {q: err(result[q], ref[q]) for q in ("est_T", "beta", "alpha")}
    for q in ("transforms", "weighted_template", "perm_matrices"):
        out[q] = max(err(a, b) for a, b in zip(result[q], ref[q]))
    out["perm_matrices_init"] = max(float(((a.detach().cpu().double() - b) / b).abs().max())
                                    for a, b in zip(result["perm_matrices_init"], ref["perm_matrices_init"]))
    return out


QUANTITIES = ("est_T", "beta", "alpha", "transforms", "weighted_template", "perm_matrices", "perm_matrices_init")
