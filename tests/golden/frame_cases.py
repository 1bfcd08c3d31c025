"""Inputs far from the unit cube for the geometric kernels (numpy only; tests/test_frames_cpu.py holds every claim made here).

A frame maps a base cloud clip(randn, -2, 2) and scales the search radius / bandwidth with it:

  unit     x                        r             control
  offset   x + (1000, -50, 3)       r             a different ulp on every axis
  far      x + 1000                 r             expanded-form noise: ties at every bound
  up       128 x                    128 r         fp32 arithmetic is exactly homogeneous in a power of two: the unit indices
  down     2^-10 x                  2^-10 r       the same, small
  lattice  1024 + 2^-12 x           1.5 * 2^-13   at most 13 fp32 values per axis (5 at and above 1024, 8 below, where the grid is
                                                  twice as fine), about half the points duplicated, exact ties in both forms
  aniso    (100, 1, 0.01) x         r             a flat box 10 000 times longer on one axis than on another

Every frame stays where the reference is defined: 3 (4 s)^2 < 1e10 for the 1e10 start of furthest point sampling, no coordinate
beyond 60 000, nothing near the fp32 subnormals (the smallest squared difference, 2^-28 in `lattice`, is 2^98 above them).

Also here: the feature clouds of the feature-space kNN and the rank-deficient / translated cases of the rotation heads."""
import itertools

import numpy as np

FRAMES = ("unit", "offset", "far", "up", "down", "lattice", "aniso")
R_UNIT = 0.5
OFFSET = (1000.0, -50.0, 3.0)
F32 = np.float32


def base_cloud(B, N, seed):
    return np.clip(np.random.default_rng(seed).standard_normal((B, N, 3)), -2, 2).astype(F32)


def apply(frame, x, r=R_UNIT):
    """(cloud, radius) of `frame`, both fp32: every map is one fp32 operation per coordinate (exact in up, down and lattice)"""
    x = np.asarray(x, F32)
    if frame == "unit":
        return x.copy(), F32(r)
    if frame == "offset":
        return x + np.asarray(OFFSET, F32), F32(r)
    if frame == "far":
        return x + F32(1000.0), F32(r)
    if frame == "up":
        return x * F32(128.0), F32(r) * F32(128.0)
    if frame == "down":
        return x * F32(2.0 ** -10), F32(r) * F32(2.0 ** -10)
    if frame == "lattice":
        return F32(1024.0) + F32(2.0 ** -12) * x, F32(1.5 * 2.0 ** -13)
    if frame == "aniso":
        return x * np.asarray((100.0, 1.0, 0.01), F32), F32(r)
    raise ValueError(frame)


def cloud(frame, B, N, seed, r=R_UNIT):
    return apply(frame, base_cloud(B, N, seed), r)


BALL_N, BALL_S = 2048, 64
BALL_SEED = 6163      # pinned: with this base cloud the aniso frame too has a furthest-point sample whose ball (on the clipped x
#                       face, where 2 % of the points share one x) holds more than 16 points; most seeds give it at most 9


def outside_queries(x, r):
    """8 query points per cloud outside its bounding box [B,8,3]: the extreme point of an axis pushed out by 0.9 r (the
    neighbouring cell; its ball still holds that point), by 1.9 r (two cells out; empty) and by 100 r (far; empty), low and high
    side, each distance on another axis; and the box's two opposite corners pushed out diagonally by 0.9 r and 1.9 r."""
    x = np.asarray(x, F32)
    r = F32(r)
    B = x.shape[0]
    out = np.empty((B, 8, 3), F32)
    for b in range(B):
        lo, hi = x[b].min(0), x[b].max(0)
        for axis, f in enumerate((0.9, 1.9, 100.0)):
            d = F32(f) * r
            q = x[b, x[b, :, axis].argmin()].copy(); q[axis] = q[axis] - d; out[b, 2 * axis] = q
            q = x[b, x[b, :, axis].argmax()].copy(); q[axis] = q[axis] + d; out[b, 2 * axis + 1] = q
        out[b, 6] = lo - F32(0.9) * r
        out[b, 7] = hi + F32(1.9) * r
    return out


# ------------------------------------------------------------------------------------------------------- feature-space kNN
FEATURE_KINDS = ("offset", "relu", "ramp", "onehot")
FEATURE_SHAPES = ((64, 300, 20), (48, 200, 33), (130, 257, 64))        # (C, N, k); (64, 1024, 20) once
FEATKNN_MARGIN = float.fromhex("0x1.1p-9")                             # featknn.hip: margin = 0x1.1p-9 |x_q| max|x_j|


def features(kind, B, C, N, seed):
    """x [B,C,N] fp32.  offset: a common offset far above the spread (every candidate inside the kernel's margin); relu:
    non-negative, mean above spread; ramp: points 128 t .. 128 t + 127 scaled by 10^t (every tile of 128 keys on a scale of
    its own, three tiles 1000-fold apart); onehot: one channel carries 300."""
    g = np.random.default_rng(seed)
    z = g.standard_normal((B, C, N))
    if kind == "offset":
        x = 5.0 + 0.05 * z
    elif kind == "relu":
        x = np.maximum(z, 0.0)
    elif kind == "ramp":
        x = z * (10.0 ** (np.arange(N) // 128))[None, None, :]
    elif kind == "onehot":
        x = z.copy()
        x[:, C // 3, :] += 300.0
    else:
        raise ValueError(kind)
    return x.astype(F32)


def exact_sqdist(x_bcn):
    """fp64 [B,N,N] squared distances by direct differences (no cancellation at any offset) and max|x|^2 summed over channels"""
    x = np.asarray(x_bcn, np.float64)
    d = np.zeros((x.shape[0], x.shape[2], x.shape[2]))
    for c in range(x.shape[1]):
        d += (x[:, c, :, None] - x[:, c, None, :]) ** 2
    return d, float((x ** 2).sum(axis=1).max())


# ------------------------------------------------------------------------------------------------------------ rotation heads
def rotation_from_H64(H):
    """utils/svd.py:38-49 in fp64: R = V U^T, the last column of V negated when det < 0.  Also returns U, S, V."""
    H = np.asarray(H, np.float64)
    u, s, vt = np.linalg.svd(H)
    v = vt.T
    r = v @ u.T
    if np.linalg.det(r) < 0:
        r = (v @ np.diag([1.0, 1.0, -1.0])) @ u.T
    return r, u, s, v


def signed_permutation_H():
    """H = P diag(3, 2, 1) Q [50,3,3] fp32: P runs over the 6 orders times the 8 sign patterns, Q over the same list in
    another order -- exact zeros off the pattern, so a Jacobi sweep never rotates and the sort of three sees every order.  The
    last two are diag(1, 0.5, +-1e-20)."""
    sp = []
    for p in itertools.permutations(range(3)):
        for sg in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3))
            for i in range(3):
                m[i, p[i]] = sg[i]
            sp.append(m)
    H = [sp[i] @ np.diag([3.0, 2.0, 1.0]) @ sp[(7 * i + 5) % 48] for i in range(48)]
    H += [np.diag([1.0, 0.5, 1e-20]), np.diag([1.0, 0.5, -1e-20])]
    return np.stack(H).astype(F32)


def _rot(g):
    q, _ = np.linalg.qr(g.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _rz(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def degenerate_pairs(M=64, seed=7):
    """name -> (src [M,3], corr [M,3], rank) fp32, corr an exact rigid (or mirrored) image of src in fp64, rounded once.
      plane_z0       z = 0 exactly on both sides, a rotation about z: H has an exactly zero row and column
      plane_rot      the plane turned by a random rotation, another random rotation and a shift between the clouds
      plane_mirror   the same with the in-plane y axis mirrored first (a proper rotation fits a plane's mirror image exactly)
      plane_exact    integer points of a tilted plane and their image under a rational rotation: H is exact, of rank exactly 2
      line           points on one line;  line_exact: the same in integers;  point: every point the same
    In-plane axes are scaled (3, 2): s2/s1 = 4/9 and (s1 - s2)/s1 = 5/9 up to the sample's variances."""
    g = np.random.default_rng(seed)
    p = np.zeros((M, 3))
    p[:, 0] = 3.0 * g.standard_normal(M)
    p[:, 1] = 2.0 * g.standard_normal(M)
    q1, q2 = _rot(g), _rot(g)
    shift = np.array([0.5, -1.0, 2.0])
    out = {}
    z0 = p.astype(F32).astype(np.float64)
    rz = _rz(0.7).astype(F32).astype(np.float64)
    c = z0 @ rz.T
    c[:, :2] += shift[:2]
    out["plane_z0"] = (z0, c, 2)
    s = p @ q1.T
    out["plane_rot"] = (s, s @ q2.T + shift, 2)
    out["plane_mirror"] = (s, (p * np.array([1.0, -1.0, 1.0])) @ q1.T @ q2.T + shift, 2)
    line = (g.standard_normal(M)[:, None] * np.array([[2.0, -1.0, 0.5]]))
    out["line"] = (line + 0.25, line @ q2.T + shift, 1)
    # integer coordinates, a rational rotation, M a power of two: means, centred points and H are exact in fp32 and in fp64, so H
    # has rank exactly 2 (1) in a general orientation and its last singular value(s) fall below every "is it zero" threshold
    ea, eb = np.array([1.0, 2.0, 2.0]), np.array([2.0, 1.0, -2.0])            # orthogonal, both of length 3
    qe = np.array([[2.0, -1.0, 2.0], [2.0, 2.0, -1.0], [-1.0, 2.0, 2.0]]) / 3.0   # a proper rotation with entries in thirds
    ishift = np.array([4.0, -7.0, 2.0])
    i, j = g.integers(-9, 10, M // 2).astype(np.float64), g.integers(-6, 7, M // 2).astype(np.float64)
    i, j = np.concatenate([i, -i]), np.concatenate([j, -j])                    # every point with its opposite: the mean is exactly 0
    pe = 3.0 * (i[:, None] * ea + j[:, None] * eb)
    out["plane_exact"] = (pe, np.rint(pe @ qe.T) + ishift, 2)
    le = 3.0 * i[:, None] * ea
    out["line_exact"] = (le, np.rint(le @ qe.T) + ishift, 1)
    pt = np.broadcast_to(np.array([[0.3, -0.2, 0.9]]), (M, 3))
    out["point"] = (pt.copy(), pt @ q2.T + shift, 0)
    return {k: (a.astype(F32), b.astype(F32), rk) for k, (a, b, rk) in out.items()}


def weighted_H64(src, corr, w_centre, w_H):
    """fp64: centroids c = sum w_centre x (w_centre sums to 1), H = sum w_H (src - c_s)(corr - c_c)^T -> (H, c_s, c_c).
    kabsch: both 1/M;  rigid_transform_weighted: both w / (sum w + eps);  gmm_register: w_centre = pi, w_H = pi / var."""
    s, c = np.asarray(src, np.float64), np.asarray(corr, np.float64)
    wc, wh = np.asarray(w_centre, np.float64), np.asarray(w_H, np.float64)
    cs, cc = (wc[:, None] * s).sum(0), (wc[:, None] * c).sum(0)
    H = ((s - cs) * wh[:, None]).T @ (c - cc)
    return H, cs, cc


TRANSLATIONS = {"both_offset": (OFFSET, OFFSET), "apart": ((1000.0, 1000.0, 1000.0), (-500.0, -500.0, -500.0))}
TRANSLATED_M = (3, 128, 1000)


def translated_pair(kind, M, seed):
    """src, corr [M,3] fp32: a unit-scale cloud, its rotated and slightly noisy image, then each side shifted"""
    g = np.random.default_rng(seed)
    a = g.uniform(-1, 1, (M, 3))
    b = a @ _rot(g).T + 0.01 * g.standard_normal((M, 3)) + np.array([0.2, -0.1, 0.3])
    ta, tb = TRANSLATIONS[kind]
    return (a + np.asarray(ta)).astype(F32), (b + np.asarray(tb)).astype(F32)
