"""What the tests of the partial / noisy pairs share: the fixture tests/golden/partial_seeded.npz (made from the reference by
make_golden_partial.py), the case lists, and an fp64 numpy model of l3d_crop_select's selection as include/ext/l3d_partial.h
states it.  The model is the yardstick of the kernel at shapes the reference was not run at; the fixture holds the model itself to
the reference's own index lists (tests/test_partial_cpu.py)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "partial_seeded.npz")
NEAREST, PLANE = 0, 1

# farthest_subsample_points: (name, N, K, C, sign of the view point's offset)
FARTHEST = (("f1024c3p", 1024, 768, 3, +1), ("f1024c6n", 1024, 768, 6, -1), ("f200c3n", 200, 77, 3, -1), ("f200c6p", 200, 77, 6, +1))
# planar_crop: (name, N)
PLANAR = (("p1024", 1024), ("p101", 101), ("p11", 11))
# whole RegistrationData samples: (name, index into the dataset)
SAMPLES = (("s_prnet", 3), ("s_planar", 5))
NEAREST_GAP, PLANE_GAP = 1e-6, 1e-5     # conditions the generator puts on its seeds (PLANE_GAP: the issue's 1e-9, raised so that an
                                        # ulp of the fp32 centroid -- torch's mean against numpy's -- cannot move the boundary)

_cache = {}


def load():
    if "z" not in _cache:
        _cache["z"] = dict(np.load(PATH))
    return _cache["z"]


def ordered_u64(key):
    """fp64 keys -> uint64 with the same order under l3d_mask_select's rule: a NaN above every number, -0 == +0"""
    key = np.ascontiguousarray(key, dtype=np.float64)
    u = np.where(key == 0.0, 0.0, key).view(np.uint64).copy()
    neg = (u >> np.uint64(63)).astype(bool)
    u = np.where(neg, ~u, u | np.uint64(1 << 63))
    u[np.isnan(key)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return u


def keys(points, vec, centre, mode):
    """the header's fp64 keys of one cloud: points [N,C] fp32, vec [3] fp64, centre [3] fp32 -> [N] fp64; every product and sum is a
    separate numpy operation, so each is rounded on its own"""
    xyz = np.asarray(points, dtype=np.float32)[:, :3]
    vec = np.asarray(vec, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == NEAREST:
            d = xyz.astype(np.float64) - vec[None, :]
            xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]
        else:
            f = (xyz - np.asarray(centre, dtype=np.float32)[None, :]).astype(np.float32)
            xx, yy, zz = f[:, 0].astype(np.float64) * vec[0], f[:, 1].astype(np.float64) * vec[1], f[:, 2].astype(np.float64) * vec[2]
        return (xx + yy) + zz


def select(points, vec, centre, mode, K):
    """-> int64 [K]: the indices l3d_crop_select lists for one cloud"""
    if mode == PLANE and K == len(points):
        return np.arange(K, dtype=np.int64)
    u = ordered_u64(keys(points, vec, centre, mode))
    if mode == NEAREST:
        return np.argsort(u, kind="stable")[:K].astype(np.int64)             # ascending key, equal keys by index
    return np.sort(np.argsort(~u, kind="stable")[:K]).astype(np.int64)         # the K largest, equal keys by index; then index order


def select_batch(points, vec, centre, mode, K):
    """points [B,N,C], vec [B,3], centre [B,3] or None -> (idx int64 [B,K], mask fp32 [B,N])"""
    idx = np.stack([select(points[b], None if vec is None else vec[b], None if centre is None else centre[b], mode, K)
                    for b in range(len(points))])
    mask = np.zeros(points.shape[:2], dtype=np.float32)
    np.put_along_axis(mask, idx, 1.0, axis=1)
    return idx, mask


def jitter(rows, noise, sigma, clip):
    """the header's `out`: rows [..,C] fp32 + clamp(sigma noise, -clip, clip), one fp32 multiplication and one fp32 addition"""
    e = np.asarray(noise, dtype=np.float32)
    if sigma is not None:
        e = (np.asarray(sigma, dtype=np.float32).reshape((-1,) + (1,) * (e.ndim - 1)) * e).astype(np.float32)
    if clip > 0:
        c = np.float32(clip)
        e = np.where(e < -c, -c, np.where(e > c, c, e)).astype(np.float32)
    return (np.asarray(rows, dtype=np.float32) + e).astype(np.float32)
