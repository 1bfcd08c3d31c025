"""How deepgmr_seeded.npz stores its large arrays, shared by make_golden_deepgmr.py (pack_*) and the tests (load_case).  Two full
copies (fp32 and fp64) of the RRI features of every cloud do not fit the 1 MiB a committed file may have, so:

  * a source quantity that is the template's up to rounding (features, logits, gamma: the source is a rigid copy and the features are
    rotation invariant) is stored as the int64 difference of the two fp32 bit patterns, `s_<q>32_ulps`; t32 bits + ulps = s32 bits,
    exactly;
  * features are stored kind-major, [4 (rp, rq, theta, phi), B, N, k], so that rp, the same for a point's k neighbours, is a run;
  * the fp64 features are fp32 + d, d quantised to int16 in units of gap_kind / 8192 (`*_feat_q64`): exact to 1/16384 of the gap the
    tests' bars are multiples of, clipped at +-4 gaps (only entries across the 2 pi wrap, which the unstable-phi mask names);
  * the fp64 logits are fp32 + d, d quantised the same way in units of their gap / 8192 (`*_logits_q64`; |d| <= gap by the gap's
    definition, so nothing is clipped): exact to 1/16384 of the gap;
  * gamma is stored in full fp64 (the model in fp64 is held to 1e-12 of it), and the fp32 gamma as the difference of its bit pattern
    from that of the fp64 value rounded to fp32 (`*_gamma32_ulps`, a few units): exact;
  * the source's kNN indices are stored as their difference from the template's.
pi, mu, sigma and both T are small and stored twice in full."""
import math

import numpy as np
import torch

FEAT_UNITS = 8192.0


def rri_restated_fp64(xyz, idx, wrap=1e-5):
    """get_rri's definition in fp64 on the CPU, written from the formulas and independent of the package: xyz [B,N,3], idx [B,N,k]
    -> feat [B,N,k,4] (rp, rq, theta, phi), the mask [B,N,k] of entries with some psi_ab, b != a, within `wrap` of 0 or 2 pi, and
    psi [B,N,k,k]"""
    x = xyz.double().cpu()
    idx = idx.cpu()
    B, N, _ = x.shape
    k = idx.shape[2]
    q = torch.stack([x[b][idx[b]] for b in range(B)])                            # [B,N,k,3]
    p = x[:, :, None, :].expand_as(q)
    rp, rq = p.norm(dim=-1), q.norm(dim=-1)
    pn = p / rp[..., None]
    dot = (pn * q / rq[..., None]).sum(-1)
    theta = torch.acos(dot.clamp(-1, 1))
    t = q - dot[..., None] * p
    ta, tb = t[:, :, :, None, :].expand(B, N, k, k, 3), t[:, :, None, :, :].expand(B, N, k, k, 3)
    sin = (torch.linalg.cross(tb, ta, dim=-1) * pn[:, :, :1, None, :]).sum(-1)
    psi = torch.remainder(torch.atan2(sin, (tb * ta).sum(-1)), 2 * math.pi)
    off = ~torch.eye(k, dtype=torch.bool)
    phi = psi.masked_fill(~off, float("inf")).min(dim=-1)[0]
    near = (((psi < wrap) | (psi > 2 * math.pi - wrap)) & off).any(dim=-1)
    return torch.stack([rp, rq, theta, phi], dim=-1), near, psi


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)


def pack_pair32(out, q, t32, s32):
    t32, s32 = np.asarray(t32, dtype=np.float32), np.asarray(s32, dtype=np.float32)
    out[f"t_{q}32"] = t32
    out[f"s_{q}32_ulps"] = _bits(s32) - _bits(t32)
    assert np.array_equal(unpack_pair32(out, q)[1].view(np.int32), s32.view(np.int32))


def unpack_pair32(c, q):
    t32 = np.asarray(c[f"t_{q}32"], dtype=np.float32)
    s32 = (_bits(t32) + c[f"s_{q}32_ulps"]).astype(np.int32).view(np.float32)
    return t32, s32


def kind_major(feat):
    B, N, k4 = feat.shape
    return np.ascontiguousarray(feat.reshape(B, N, k4 // 4, 4).transpose(3, 0, 1, 2))


def neighbour_major(km):
    _, B, N, k = km.shape
    return np.ascontiguousarray(km.transpose(1, 2, 3, 0)).reshape(B, N, 4 * k)


def pack_feat64(out, cn, f32, f64, gaps):
    d = kind_major(np.asarray(f64, dtype=np.float64) - np.asarray(f32, dtype=np.float64))
    q = np.clip(np.rint(d / (np.asarray(gaps)[:, None, None, None] / FEAT_UNITS)), -32767, 32767).astype(np.int16)
    out[f"{cn}_feat_q64"] = q
    return np.abs(q) < 32767           # kind-major mask of the entries that are stored to 1/16384 of the gap


def pack_q64(out, key, v32, v64, gap):
    d = np.asarray(v64, dtype=np.float64) - np.asarray(v32, dtype=np.float64)
    q = np.rint(d / (gap / FEAT_UNITS))
    assert np.abs(q).max() <= FEAT_UNITS
    out[f"{key}_q64"] = q.astype(np.int16)


def pack_gamma(out, cn, g32, g64):
    out[f"{cn}_gamma64"] = np.asarray(g64, dtype=np.float64)
    out[f"{cn}_gamma32_ulps"] = (_bits(g32) - _bits(out[f"{cn}_gamma64"].astype(np.float32))).astype(np.int32)


def load_case(z, name):
    """-> dict of the case's arrays with the packed ones rebuilt: {t,s}_feat32 / feat64 [B,N,4k], {t,s}_logits32 / 64, gamma32 / 64"""
    c = {k[len(name) + 1:]: v for k, v in z.items() if k.startswith(name + "_")}
    km = dict(zip("ts", unpack_pair32(c, "featkm")))
    for cn in "ts":
        gaps = c[f"{cn}_feat_gap"]
        d = c[f"{cn}_feat_q64"].astype(np.float64) * (gaps[:, None, None, None] / FEAT_UNITS)
        c[f"{cn}_feat32"] = neighbour_major(km[cn])
        c[f"{cn}_feat64"] = neighbour_major(km[cn].astype(np.float64) + d)
    c["t_idx"] = c["t_idx"].astype(np.int64)
    c["s_idx"] = c["t_idx"] + c["s_idx_delta"].astype(np.int64)
    for cn, v32 in zip("ts", unpack_pair32(c, "logits")):
        c[f"{cn}_logits32"] = v32
        c[f"{cn}_logits64"] = v32.astype(np.float64) + c[f"{cn}_logits_q64"].astype(np.float64) * (float(c[f"{cn}_logits_gap"]) / FEAT_UNITS)
        c[f"{cn}_gamma32"] = (_bits(c[f"{cn}_gamma64"].astype(np.float32)) + c[f"{cn}_gamma32_ulps"]).astype(np.int32).view(np.float32)
    return c
