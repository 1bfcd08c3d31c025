"""The geometric kernels on clouds far from the unit cube (tests/golden/frame_cases.py; tests/test_frames_cpu.py holds what the
cases claim): metres away from the origin, scaled by powers of two, collapsed onto the fp32 grid at 1024, a box 10 000 times
longer on one axis than on another.  The search kernels are held index for index to the CPU oracle, which restates the
reference's fp32 rounding sequences and so follows it into every one of these frames; feature-space kNN to exact fp64 distances at
the bar its header grants; the rotation heads to an fp64 value on rank-deficient input and, on translated clouds, to GAP_FACTOR
times the fp32-to-fp64 gap of the reference's own op sequence (torch on the CPU).  Every rotation test prints error, gap, ratio."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import frame_cases as fc      # noqa: E402

import oracle                 # noqa: E402

pytestmark = pytest.mark.gpu
B = 2
GAP_FACTOR = 4.0
DEV = "cuda"


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))                         # a copy: the cached clouds stay as they are
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def call(name, *args):
    from learning3d_amd._lib import call as c
    c(name, *args)


@functools.lru_cache(maxsize=None)
def cloud(frame, N, seed=None):
    x, r = fc.cloud(frame, B, N, 4100 + N if seed is None else seed)
    x.setflags(write=False)
    return x, r


# ----------------------------------------------------------------------------------------------------------- point kNN graph
def knn_graph(x, k, variant):
    Bq, N, _ = x.shape
    idx = torch.full((Bq, N, k), -7, dtype=torch.int64, device=DEV)
    call("l3d_knn_graph_variant", dev(x), Bq, N, k, idx, variant)
    return idx.cpu().numpy()


@functools.lru_cache(maxsize=None)
def oracle_knn24(frame, N):
    """the oracle's 24 best per query, best first, lowest index first among equals: its first k are its answer for k"""
    return oracle.knn(cloud(frame, N)[0], min(24, N))


@pytest.mark.parametrize("N", [100, 256, 1000, 2048])
@pytest.mark.parametrize("frame", fc.FRAMES)
def test_knn_graph_every_frame_equals_oracle(frame, N):
    x, _ = cloud(frame, N)
    want = oracle_knn24(frame, N)
    for k in (1, 20, 24):
        one = knn_graph(x, k, 1)
        assert np.array_equal(one, want[:, :, :k]), (frame, N, k, np.argwhere(one != want[:, :, :k])[:4])
        assert np.array_equal(knn_graph(x, k, 0), one), (frame, N, k, "variant 0")
        if N >= 256:
            two = knn_graph(x, k, 2)
            assert np.array_equal(two, one), (frame, N, k, "variant 2", np.argwhere(two != one)[:4])
        if frame in ("up", "down"):                                      # a power-of-two scale: the unit frame's indices, no oracle asked
            assert np.array_equal(one, knn_graph(cloud("unit", N)[0], k, 1)), (frame, N, k, "scale")


# ------------------------------------------------------------------------------------------ kNN between two clouds, three_nn
def knn_pair(q, c, k, variant):
    Bq, n, _ = q.shape
    m = c.shape[1]
    d2 = torch.full((Bq, n, k), -1.0, dtype=torch.float32, device=DEV)
    idx = torch.full((Bq, n, k), -7, dtype=torch.int32, device=DEV)
    call("l3d_knn_variant", Bq, n, m, k, dev(q), dev(c), d2, idx, variant)
    return d2.cpu().numpy(), idx.cpu().numpy()


def oracle_knn_pair(q, c, k):
    q, c = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(c, np.float32)
    Bq, n, _ = q.shape
    d2 = np.empty((Bq, n, k), np.float32)
    idx = np.empty((Bq, n, k), np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    oracle.lib().orc_knn_pair(Bq, n, c.shape[1], k, vp(q), vp(c), vp(d2), vp(idx))
    return d2, idx


def within_ulps(a, b, n):
    return np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= n * np.spacing(np.maximum(np.abs(a), np.abs(b))))


@pytest.mark.parametrize("m", [64, 1100])
@pytest.mark.parametrize("frame", fc.FRAMES)
def test_knn_pair_every_frame_equals_oracle(frame, m):
    q, _ = cloud(frame, 300, 4400)
    c, _ = cloud(frame, m)
    want_d64, want_i64 = oracle_knn_pair(q, c, 64)                      # insertion in scan order: a prefix answers every smaller k
    for k in (3, 4, 16, 64):
        wd, wi = want_d64[:, :, :k], want_i64[:, :, :k]
        d1, i1 = knn_pair(q, c, k, 1)
        assert np.array_equal(i1, wi), (frame, m, k, np.argwhere(i1 != wi)[:4])
        assert within_ulps(d1, wd, 2), (frame, m, k)
        if frame == "lattice":                                           # differences and their squares are exact there
            assert np.array_equal(d1, wd), (frame, m, k)
        for variant in (2, 3) if k <= 4 else (2,):
            dv, iv = knn_pair(q, c, k, variant)
            assert np.array_equal(iv, i1) and np.array_equal(dv, d1), (frame, m, k, variant)
    d3 = torch.full((B, 300, 3), -1.0, dtype=torch.float32, device=DEV)
    i3 = torch.full((B, 300, 3), -7, dtype=torch.int32, device=DEV)
    call("l3d_three_nn", B, 300, m, dev(q), dev(c), d3, i3)
    od, oi = oracle.three_nn(q, c)                                       # (sqrt d2, idx)
    assert np.array_equal(i3.cpu().numpy(), oi), (frame, m)
    assert np.array_equal(i3.cpu().numpy(), want_i64[:, :, :3])
    assert within_ulps(d3.cpu().numpy(), want_d64[:, :, :3], 2), (frame, m)


# ------------------------------------------------------------------------------------------------ furthest point sampling
def fps32(x, S, temp=False):
    Bq, n, _ = x.shape
    idx = torch.full((Bq, S), -7, dtype=torch.int32, device=DEV)
    t = torch.empty((Bq, n), dtype=torch.float32, device=DEV) if temp else None
    call("l3d_furthest_point_sampling", Bq, n, S, dev(x), t, idx)
    return idx.cpu().numpy()


@pytest.mark.parametrize("n", [300, 2048])
@pytest.mark.parametrize("frame", fc.FRAMES)
def test_fps_every_frame_equals_oracle(frame, n):
    x, _ = cloud(frame, n)
    got = fps32(x, 64)
    assert np.array_equal(got, oracle.furthest_point_sampling(x, 64)), (frame, n)       # bit-reversed tie rule (lattice: duplicates)
    assert np.array_equal(fps32(x, 64, temp=True), got)
    idx = torch.full((B, 64), -7, dtype=torch.int64, device=DEV)
    call("l3d_farthest_point_sample", dev(x), B, n, 64, None, None, idx)
    assert np.array_equal(idx.cpu().numpy(), oracle.farthest_point_sample(x, 64)), (frame, n)   # first maximal index


# ------------------------------------------------------------------------------------------------------------- ball query
def ball_query(x, cen, r, K, cells):
    Bq, n, _ = x.shape
    m = cen.shape[1]
    idx = torch.full((Bq, m, K), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(Bq * (16 * n + 16448), dtype=torch.uint8, device=DEV) if cells else None
    call("l3d_ball_query", Bq, n, m, float(r), K, dev(cen), dev(x), idx, ws)
    return idx.cpu().numpy()


def ball_case(frame, n, r):
    x, r0 = cloud(frame, n, fc.BALL_SEED if n == fc.BALL_N else None)
    r = r0 if r is None else np.float32(r)
    fps = oracle.furthest_point_sampling(x, fc.BALL_S)
    cen = np.concatenate([np.stack([x[b][fps[b]] for b in range(B)]), fc.outside_queries(x, r)], axis=1)
    return x, cen, r


BALL_CASES = [(f, None) for f in fc.FRAMES] + [("aniso", 0.005), ("lattice", 2.0 ** -13)]


@pytest.mark.parametrize("frame,r", BALL_CASES)
def test_ball_query_both_routes_every_frame_equal_oracle(frame, r):
    for n in (300, 2048):
        x, cen, rr = ball_case(frame, n, r)
        for K in (16, 64):
            want = oracle.ball_query(rr, K, x, cen)
            scan = ball_query(x, cen, rr, K, False)
            assert np.array_equal(scan, want), (frame, n, K, "scan", np.argwhere(scan != want)[:4])
            if n >= 2048:
                cells = ball_query(x, cen, rr, K, True)
                assert np.array_equal(cells, want), (frame, n, K, "cells", np.argwhere(cells != want)[:4])
                assert np.array_equal(cells, scan)


# ----------------------------------------------------- the torch-level primitives: expanded and direct forms, N = 300 and 1500
@pytest.mark.parametrize("N", [300, 1500])
@pytest.mark.parametrize("frame", fc.FRAMES)
def test_torch_level_primitives_every_frame(frame, N):
    x, r = cloud(frame, N)
    S = 128
    fps = oracle.farthest_point_sample(x, S)
    new = np.stack([x[b][fps[b]] for b in range(B)])
    xd, nd = dev(x), dev(new)
    # square_distance: the reference's expanded form, bit for bit
    dist = torch.empty((B, S, N), dtype=torch.float32, device=DEV)
    call("l3d_square_distance", nd, xd, B, S, N, 3, dist)
    want_d = oracle.square_distance(new, x)
    assert np.array_equal(dist.cpu().numpy(), want_d), (frame, N)
    # query_ball_point, without and with itself_indices
    for K in (16, 64):
        idx = torch.full((B, S, K), -7, dtype=torch.int64, device=DEV)
        cnt = torch.full((B, S), -7, dtype=torch.int64, device=DEV)
        call("l3d_query_ball_point", float(r), K, xd, nd, B, N, S, None, idx, cnt)
        oi, oc = oracle.query_ball_point(float(r), K, x, new, get_cnt=True)
        assert np.array_equal(idx.cpu().numpy(), oi) and np.array_equal(cnt.cpu().numpy(), oc), (frame, N, K)
        call("l3d_query_ball_point", float(r), K, xd, nd, B, N, S, dev(fps), idx, None)
        assert np.array_equal(idx.cpu().numpy(), oracle.query_ball_point_itself(float(r), K, x, new, fps)), (frame, N, K, "itself")
    # knn_point: direct differences
    val = torch.empty((B, S, 16), dtype=torch.float32, device=DEV)
    idx = torch.full((B, S, 16), -7, dtype=torch.int64, device=DEV)
    call("l3d_knn_point", 16, xd, nd, B, N, S, val, idx)
    ov, oi = oracle.knn_point(16, x, new)
    assert np.array_equal(idx.cpu().numpy(), oi), (frame, N)
    assert within_ulps(val.cpu().numpy(), ov, 1), (frame, N)             # sqrt of the same fp32 sum: at most its last bit
    # knn_point_expanded: nearest first on the expanded form; only exact ties of the ranked value may be ordered differently
    idx = torch.full((B, S, 32), -7, dtype=torch.int64, device=DEV)
    call("l3d_knn_point_expanded", 32, xd, nd, B, N, S, idx)
    got, want = idx.cpu().numpy(), oracle.knn_point_expanded(32, x, new)
    if not np.array_equal(got, want):
        assert got.min() >= 0 and got.max() < N
        assert np.array_equal(np.take_along_axis(want_d, got, -1), np.take_along_axis(want_d, want, -1)), (frame, N)
        srt = np.sort(got, -1)
        assert (srt[..., 1:] != srt[..., :-1]).all()


@pytest.mark.parametrize("frame", ["unit", "up", "down", "offset"])
def test_gaussian_density_scaled_bandwidth(frame):
    for N in (300, 1500):
        x, r = cloud(frame, N)
        bw = float(r) * 0.2                                              # 0.1 in the unit frame, scaled like the radius
        out = torch.empty((B, N), dtype=torch.float32, device=DEV)
        call("l3d_gaussian_density", dev(x), B, N, bw, out)
        np.testing.assert_allclose(out.cpu().numpy(), oracle.gaussian_density(x, bw), rtol=1e-5, atol=0, err_msg=f"{frame} {N}")


# ------------------------------------------------------------------------------------------------------ feature-space kNN
def knn_feature(x, k):
    from learning3d_amd._lib import lib
    Bq, C, N = x.shape
    ws = torch.empty(lib().l3d_knn_feature_workspace_bytes(Bq, C, N), dtype=torch.uint8, device=DEV)
    idx = torch.full((Bq, N, k), -7, dtype=torch.int64, device=DEV)
    call("l3d_knn_feature", dev(x), Bq, C, N, k, ws, idx)
    return idx.cpu().numpy()


def check_feature_lists(x, k, idx, what):
    N = x.shape[2]
    d, sqmax = fc.exact_sqdist(x)
    tol = 4e-6 * sqmax
    assert idx.min() >= 0 and idx.max() < N, what
    kth = np.sort(d, axis=-1)[:, :, k - 1]
    got = np.take_along_axis(d, idx, axis=-1)
    assert np.all(got.max(axis=-1) <= kth + tol), (what, float((got.max(axis=-1) - kth).max()), tol)
    assert np.all(np.diff(got, axis=-1) >= -tol), what
    srt = np.sort(idx, axis=-1)
    assert np.all(srt[:, :, 1:] != srt[:, :, :-1]), what
    nearest = np.sort(d, axis=-1)[:, :, 1]                               # the nearest OTHER point (d[i][i] = 0 exactly)
    sure = nearest > tol
    assert np.all(idx[:, :, 0][sure] == np.broadcast_to(np.arange(N), idx.shape[:2])[sure]), what
    return float(sure.mean())


@pytest.mark.parametrize("C,N,k", fc.FEATURE_SHAPES)
@pytest.mark.parametrize("kind", fc.FEATURE_KINDS)
def test_knn_feature_kinds_vs_exact_distances(kind, C, N, k):
    x = fc.features(kind, B, C, N, 900 + N)
    idx = knn_feature(x, k)
    sure = check_feature_lists(x, k, idx, (kind, C, N, k))
    print(f"knn_feature {kind} C {C} N {N} k {k}: self-first asked of {sure:.2f} of the queries")
    up = knn_feature(x * np.float32(128.0), k)                           # 2^7: every product, sum and comparison scales exactly
    assert np.array_equal(up, idx), (kind, C, N, k, "scale", int((up != idx).sum()))


def test_knn_feature_kinds_more_than_one_block():
    C, N, k = 64, 1024, 20
    for kind in fc.FEATURE_KINDS:
        x = fc.features(kind, B, C, N, 900 + N)
        idx = knn_feature(x, k)
        check_feature_lists(x, k, idx, (kind, C, N, k))
        assert np.array_equal(knn_feature(x * np.float32(128.0), k), idx), (kind, "scale")


# ---------------------------------------------------------------------------------------------------------- rotation heads
def svd_rotation(H):
    H = dev(H)
    R = torch.empty_like(H)
    call("l3d_svd3x3_rotation", H, H.shape[0], R)
    return R.cpu().numpy().astype(np.float64)


def kabsch(src, corr):
    """src, corr [Bq,M,3] numpy -> R [Bq,3,3], t [Bq,3] (the entry point takes [Bq,3,M])"""
    s, c = dev(np.transpose(src, (0, 2, 1))), dev(np.transpose(corr, (0, 2, 1)))
    Bq, _, M = s.shape
    R = torch.empty((Bq, 3, 3), dtype=torch.float32, device=DEV)
    t = torch.empty((Bq, 3), dtype=torch.float32, device=DEV)
    call("l3d_kabsch", s, c, Bq, M, R, t, None)
    return R.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64)


RIGID_EPS = 1e-5      # models/rpmnet.py _EPS


def rigid(src, corr, w):
    Bq, M, _ = src.shape
    T = torch.empty((Bq, 3, 4), dtype=torch.float32, device=DEV)
    call("l3d_rigid_transform_weighted", dev(src), dev(corr), dev(w), Bq, M, RIGID_EPS, T)
    T = T.cpu().numpy().astype(np.float64)
    return T[:, :, :3], T[:, :, 3]


def gmm(pi, mu_s, mu_t, var):
    Bq, J = pi.shape
    T = torch.empty((Bq, 4, 4), dtype=torch.float32, device=DEV)
    call("l3d_gmm_register", dev(pi), dev(mu_s), dev(mu_t), dev(var), Bq, J, T)
    T = T.cpu().numpy().astype(np.float64)
    assert np.array_equal(T[:, 3], np.broadcast_to([0.0, 0.0, 0.0, 1.0], (Bq, 4)))
    return T[:, :3, :3], T[:, :3, 3]


def weights(M, seed):
    """(w for rigid_transform_weighted, pi and var for gmm_register), fp32, the same for every cloud of a case"""
    g = np.random.default_rng(seed)
    w = (g.uniform(0.5, 1.5, M)).astype(np.float32)
    pi = g.uniform(0.2, 1.2, M)
    pi = (pi / pi.sum()).astype(np.float32)
    var = g.uniform(0.5, 1.5, M).astype(np.float32)
    return w, pi, var


def heads(src, corr, seed):
    """name -> (R, t, H64, c_s, c_c) of one pair [M,3] through the three cloud heads, with each head's own fp64 H and centroids"""
    M = src.shape[0]
    w, pi, var = weights(M, seed)
    s1, c1 = src[None], corr[None]
    out = {}
    u = np.full(M, 1.0 / M)
    out["kabsch"] = kabsch(s1, c1) + fc.weighted_H64(src, corr, u, u)
    wn = w.astype(np.float64) / (w.astype(np.float64).sum() + RIGID_EPS)
    out["rigid"] = rigid(s1, c1, w[None]) + fc.weighted_H64(src, corr, wn, wn)
    if M <= 64:
        p64 = pi.astype(np.float64)
        out["gmm"] = gmm(pi[None], s1, c1, var[None]) + fc.weighted_H64(src, corr, p64, p64 / var.astype(np.float64))
    return {k: (v[0][0], v[1][0], v[2], v[3], v[4]) for k, v in out.items()}


def proper(R, what, tol=1e-6):
    assert np.isfinite(R).all(), what
    assert np.abs(R.T @ R - np.eye(3)).max() <= tol, (what, "R^T R", float(np.abs(R.T @ R - np.eye(3)).max()))
    assert abs(np.linalg.det(R) - 1.0) <= tol, (what, "det", float(np.linalg.det(R)))


def test_svd3x3_signed_permutations():
    H = fc.signed_permutation_H()
    R = svd_rotation(H)
    worst = 0.0
    for i in range(H.shape[0]):
        want = fc.rotation_from_H64(H[i])[0]
        worst = max(worst, float(np.abs(R[i] - want).max()))
        proper(R[i], ("signed permutation", i))
    print(f"svd3x3 signed permutations and diag(1, 0.5, +-1e-20): |R - fp64| {worst:.2e}")
    assert worst <= 1e-6


@pytest.mark.parametrize("name", ["plane_z0", "plane_rot", "plane_mirror", "plane_exact"])
def test_planar_clouds_rank_two_every_head(name):
    src, corr, rank = fc.degenerate_pairs()[name]
    assert rank == 2
    res = heads(src, corr, 31)
    u = np.full(src.shape[0], 1.0 / src.shape[0])
    H32 = fc.weighted_H64(src, corr, u, u)[0].astype(np.float32)
    res["svd3x3"] = (svd_rotation(H32[None])[0], None, H32.astype(np.float64), None, None)
    if name == "plane_z0":
        assert not H32[2].any() and not H32[:, 2].any()
    for head, (R, t, H, cs, cc) in res.items():
        want = fc.rotation_from_H64(H)[0]
        err = float(np.abs(R - want).max())
        print(f"{name} {head}: |R - fp64| {err:.2e}")
        proper(R, (name, head))
        assert err <= 1e-5, (name, head, err)
        assert t is None or np.isfinite(t).all()


def test_collinear_and_coincident_clouds_every_head():
    cases = fc.degenerate_pairs()
    for name in ("line", "line_exact"):
        src, corr, _ = cases[name]
        res = heads(src, corr, 32)
        u = np.full(src.shape[0], 1.0 / src.shape[0])
        H32 = fc.weighted_H64(src, corr, u, u)[0].astype(np.float32)
        res["svd3x3"] = (svd_rotation(H32[None])[0], None, H32.astype(np.float64), None, None)
        for head, (R, t, H, cs, cc) in res.items():
            _, uu, s, vv = fc.rotation_from_H64(H)
            err = float(np.abs(R @ uu[:, 0] - vv[:, 0]).max())
            print(f"{name} {head}: |R u1 - v1| {err:.2e}")
            proper(R, (name, head))
            assert err <= 1e-5, (name, head, err)
            assert t is None or np.isfinite(t).all()
    src, corr, _ = cases["point"]
    res = heads(src, corr, 33)
    res["svd3x3"] = (svd_rotation(np.zeros((1, 3, 3), np.float32))[0], None, None, None, None)
    for head, (R, t, H, cs, cc) in res.items():
        proper(R, ("point", head))
        if t is not None:
            assert np.isfinite(t).all()
            assert np.abs(t - (cc - R @ cs)).max() <= 1e-5 * max(1.0, np.abs(cc).max()), ("point", head)   # t = mean_c - R mean_s


# translated clouds: the reference's op sequences with torch on the CPU, in fp32 and in fp64 on the same operands
def ref_kabsch(src, corr):
    """utils/svd.py:29-58 on [3,M] tensors of either precision"""
    s, c = src.t(), corr.t()
    sm, cm = s.mean(dim=1, keepdim=True), c.mean(dim=1, keepdim=True)
    H = (s - sm) @ (c - cm).t()
    u, _, v = torch.svd(H)
    r = v @ u.t()
    if torch.det(r) < 0:
        r = (v @ torch.diag(torch.tensor([1.0, 1.0, -1.0], dtype=H.dtype))) @ u.t()
    return r, (-r @ sm + cm).view(3)


def ref_rigid(src, corr, w):
    from learning3d_amd.models.rpmnet import compute_rigid_transform          # the op sequence, in the operands' precision
    T = compute_rigid_transform(src[None], corr[None], w[None])[0]
    return T[:, :3], T[:, 3]


def ref_gmm(pi, mu_s, mu_t, var):
    from learning3d_amd.models.deepgmr import gmm_register                     # the op sequence, in the operands' precision
    sigma = var[None, :, None, None] * torch.eye(3, dtype=var.dtype)[None, None]
    T = gmm_register(pi[None], mu_s[None], mu_t[None], sigma)[0]
    return T[:3, :3], T[:3, 3]


def held(pairs, what):
    gap, worst = max(g for _, g in pairs), max(e for e, _ in pairs)
    print(f"{what}: error {worst:.2e}, gap {gap:.2e}, ratio {worst / gap if gap else float('inf'):.2f}")
    assert gap > 0 and worst <= GAP_FACTOR * gap, (what, worst, gap)


@pytest.mark.parametrize("kind", list(fc.TRANSLATIONS))
def test_translated_clouds_within_the_reference_gap(kind):
    """gmm_register takes at most 64 components: its cases are J = 3 and the first 64 points of the larger clouds"""
    pairs = {(h, q): [] for h in ("kabsch", "rigid", "gmm") for q in ("R", "t")}
    e = lambda got, want: float(np.abs(got - want.numpy()).max())
    g = lambda a, b: float((a.double() - b).abs().max())
    for M in fc.TRANSLATED_M:
        src, corr = fc.translated_pair(kind, M, 70 + M)
        w, _, _ = weights(M, 40 + M)
        s32, c32, w32 = torch.from_numpy(src), torch.from_numpy(corr), torch.from_numpy(w)
        R, t = kabsch(src[None], corr[None])
        r32, t32 = ref_kabsch(s32, c32)
        r64, t64 = ref_kabsch(s32.double(), c32.double())
        pairs["kabsch", "R"].append((e(R[0], r64), g(r32, r64)))
        pairs["kabsch", "t"].append((e(t[0], t64), g(t32, t64)))
        R, t = rigid(src[None], corr[None], w[None])
        r32, t32 = ref_rigid(s32, c32, w32)
        r64, t64 = ref_rigid(s32.double(), c32.double(), w32.double())
        pairs["rigid", "R"].append((e(R[0], r64), g(r32, r64)))
        pairs["rigid", "t"].append((e(t[0], t64), g(t32, t64)))
        J = min(M, 64)
        _, pi, var = weights(J, 50 + M)
        p32, v32 = torch.from_numpy(pi), torch.from_numpy(var)
        R, t = gmm(pi[None], src[None, :J], corr[None, :J], var[None])
        r32, t32 = ref_gmm(p32, s32[:J], c32[:J], v32)
        r64, t64 = ref_gmm(p32.double(), s32[:J].double(), c32[:J].double(), v32.double())
        pairs["gmm", "R"].append((e(R[0], r64), g(r32, r64)))
        pairs["gmm", "t"].append((e(t[0], t64), g(t32, t64)))
    failed = []
    for (h, q), p in pairs.items():
        try:
            held(p, f"{h} {kind} {q}")
        except AssertionError as ex:
            failed.append(str(ex))
    assert not failed, failed
