"""The cases of tests/golden/frame_cases.py are what they claim to be (no GPU): the tie masses that push the kNN kernels into
their overflow phases, the feature clouds that force featknn's exact fallback, ball queries with short, full and empty balls in
every frame, rotation cases with the stated rank and separations and an expected rotation that does not hang on the sign of a
null vector, and power-of-two frames that leave the oracle's indices unchanged.  Conditions with pinned seeds, not measurements;
the figures they print are in LABLOG.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import frame_cases as fc      # noqa: E402

import oracle                 # noqa: E402

B = 2


def _ties_at_kth(rank, k):
    """per row of `rank` (larger is better): how many candidates carry exactly the k-th best value"""
    kth = -np.partition(-rank, k - 1, axis=-1)[..., k - 1]
    return (rank == kth[..., None]).sum(-1)


def _direct_d2(q, x):
    """[B,S,N] fp32 (dx*dx + dy*dy) + dz*dz, the direct form of ball_query / knn_pair / FPS"""
    d = q[:, :, None, :] - x[:, None, :, :]
    d = d * d
    return (d[..., 0] + d[..., 1]) + d[..., 2]


@pytest.mark.parametrize("N", [1000, 2048])
def test_lattice_overflows_the_knn_candidate_lists(N):
    x, _ = fc.cloud("lattice", B, N, 4100 + N)
    ties = _ties_at_kth(oracle.knn_pd(x), 20)
    over, phase = float((ties > 64).mean()), float((ties >= 45).mean())
    print(f"lattice N {N}: ties at the 20th value median {int(np.median(ties))}, max {int(ties.max())}; > 64 for {over:.2f}, >= 45 for {phase:.2f}")
    assert over > 0.5 and phase > 0.7


def test_far_ties_at_the_bound():
    x, _ = fc.cloud("far", B, 2048, 4100 + 2048)
    pd = oracle.knn_pd(x)
    ties = _ties_at_kth(pd, 20)
    print(f"far N 2048: ties at the 20th value median {int(np.median(ties))}, max {int(ties.max())}; "
          f"{np.mean([len(np.unique(r)) for r in pd[0, ::64]]):.0f} distinct ranking values per row")
    assert np.median(ties) >= 10


def test_lattice_is_a_lattice():
    N = 2048
    x, r = fc.cloud("lattice", B, N, 4100 + N)
    for b in range(B):
        levels = [len(np.unique(x[b, :, a])) for a in range(3)]
        distinct = len(np.unique(x[b], axis=0))
        print(f"lattice cloud {b}: levels per axis {levels}, {distinct} distinct points of {N}")
        assert max(levels) <= 13 and distinct < N / 1.5
    q, _ = fc.cloud("lattice", B, 300, 4400)
    m, _ = fc.cloud("lattice", B, 1100, 5200)
    ties = _ties_at_kth(-_direct_d2(q, m), 16)
    print(f"lattice direct form, 300 queries on 1100: ties at the 16th value median {int(np.median(ties))}, max {int(ties.max())}")
    assert ties.max() >= 8


@pytest.mark.parametrize("frame", fc.FRAMES)
def test_ball_queries_have_short_full_and_empty_balls(frame):
    N, S, K = fc.BALL_N, fc.BALL_S, 16
    x, r = fc.cloud(frame, B, N, fc.BALL_SEED)
    fps = oracle.furthest_point_sampling(x, S)
    cen = np.concatenate([np.stack([x[b][fps[b]] for b in range(B)]), fc.outside_queries(x, r)], axis=1)
    hits = (_direct_d2(cen, x) < r * r).sum(-1)
    print(f"{frame}: hits per ball min {hits[:, :S].min()}, median {int(np.median(hits[:, :S]))}, max {hits[:, :S].max()}; outside {hits[0, S:].tolist()}")
    assert (hits[:, :S] < K).any() and (hits[:, :S] > K).any()
    assert (hits[:, S:] == 0).any(axis=1).all() and (hits[:, S:] > 0).any(axis=1).all()
    lo, hi = x.min(1)[:, None], x.max(1)[:, None]
    assert ((cen[:, S:] < lo) | (cen[:, S:] > hi)).any(-1).all()               # outside the box, every one
    assert np.abs(x).max() < 60000 and 3 * (2 * np.abs(x - x.mean(1, keepdims=True)).max()) ** 2 < 1e10


@pytest.mark.parametrize("C,N,k", fc.FEATURE_SHAPES + ((64, 1024, 20),))
def test_offset_features_force_the_exact_fallback(C, N, k):
    x = fc.features("offset", B, C, N, 900 + N)
    d, _ = fc.exact_sqdist(x)
    norm = np.sqrt((x.astype(np.float64) ** 2).sum(1))                          # [B,N]
    margin = fc.FEATKNN_MARGIN * norm * norm.max(1, keepdims=True)
    print(f"offset C {C} N {N}: margin min {margin.min():.2f}, largest squared distance {d.max():.2f}")
    assert (margin >= d.max(-1)).all()


def test_feature_kinds_are_what_they_say():
    relu = fc.features("relu", B, 64, 300, 1200)
    assert relu.min() == 0 and relu.mean() > 0.5 * relu.std()
    ramp = fc.features("ramp", 1, 64, 300, 1200)[0]
    sc = [np.abs(ramp[:, 128 * t:128 * (t + 1)]).max() for t in range(3)]
    assert sc[1] > 5 * sc[0] and sc[2] > 5 * sc[1]
    one = fc.features("onehot", 1, 64, 300, 1200)[0]
    assert (np.abs(one).argmax(0) == 64 // 3).all()


def test_signed_permutations_cover_every_order_and_sign():
    H = fc.signed_permutation_H()
    assert H.shape == (50, 3, 3)
    pats = set()
    for h in H[:48]:
        assert (h != 0).sum() == 3 and sorted(np.abs(h[h != 0])) == [1, 2, 3]
        pats.add(tuple(h.ravel()))
    col_orders = {tuple(np.abs(h).argmax(0)) for h in H[:48]}
    signs = {tuple(np.sign(h[h != 0])) for h in H[:48]}
    row_of_largest = {int(np.abs(h).max(1).argmax()) for h in H[:48]}
    assert len(pats) == 48 and len(col_orders) == 6 and len(signs) == 8 and row_of_largest == {0, 1, 2}
    for h in H:                                                                 # distinct singular values: R is unique
        s = np.linalg.svd(h.astype(np.float64), compute_uv=False)
        assert (s[0] - s[1]) / s[0] >= 0.1 and s[1] / s[0] >= 0.1


def _flip_null(H, rank):
    """the reference's rotation with the null vectors of U (and so the pairing) flipped: columns rank.. of U negated"""
    R, u, s, v = fc.rotation_from_H64(H)
    u2 = u.copy()
    u2[:, 2] = -u2[:, 2]
    r2 = v @ u2.T
    if np.linalg.det(r2) < 0:
        r2 = (v @ np.diag([1.0, 1.0, -1.0])) @ u2.T
    return R, r2, s


def test_degenerate_pairs_have_the_stated_rank_and_a_unique_rotation():
    cases = fc.degenerate_pairs()
    M = 64
    w = np.full(M, 1.0 / M)
    for name, (src, corr, rank) in cases.items():
        H, _, _ = fc.weighted_H64(src, corr, w, w)
        R, R2, s = _flip_null(H, rank)
        print(f"{name}: singular values {s / max(s[0], 1e-300)}")
        assert (s > 1e-5 * max(s[0], 1e-30)).sum() == rank or rank == 0
        if rank == 2:
            assert (s[0] - s[1]) / s[0] >= 0.1 and s[1] / s[0] >= 0.1 and s[2] / s[0] < 1e-6
            assert np.abs(R - R2).max() < 1e-12                                # the null vector's sign does not matter
            assert np.abs(corr - corr.mean(0) - (src - src.mean(0)) @ R.T).max() < 1e-5   # and R is the rotation that fits
        if rank == 0:
            assert s[0] == 0
    for name in ("plane_exact", "line_exact"):                                 # exact in fp32 too: the same H from fp32 arithmetic
        src, corr, rank = cases[name]
        sc, cc = src - src.mean(0, dtype=np.float32), corr - corr.mean(0, dtype=np.float32)
        H32 = sc.T @ cc
        assert np.array_equal(H32.astype(np.float64), M * fc.weighted_H64(src, corr, w, w)[0])
        s = np.linalg.svd(H32.astype(np.float64), compute_uv=False)
        assert s[rank] <= 1e-14 * s[0]                                         # below svd3x3.h's threshold: its completion branches
    H0 = fc.weighted_H64(*cases["plane_z0"][:2], w, w)[0].astype(np.float32)
    assert not H0[2].any() and not H0[:, 2].any() and H0[:2, :2].all()         # an exactly zero row and column
    # the mirrored plane: the in-plane 2x2 block of the fitted map, seen from the two planes' own axes, is a reflection, so the
    # rotation that fits differs from the unmirrored one by a half turn about an in-plane axis
    Rr = fc.rotation_from_H64(fc.weighted_H64(*cases["plane_rot"][:2], w, w)[0])[0]
    Rm = fc.rotation_from_H64(fc.weighted_H64(*cases["plane_mirror"][:2], w, w)[0])[0]
    assert abs(np.trace(Rr.T @ Rm) + 1) < 1e-6                                  # a rotation by pi: trace = 1 + 2 cos(pi)


@pytest.mark.parametrize("kind", list(fc.TRANSLATIONS))
def test_translated_pairs_are_well_conditioned(kind):
    for M in fc.TRANSLATED_M:
        src, corr = fc.translated_pair(kind, M, 70 + M)
        w = np.full(M, 1.0 / M)
        H, cs, cc = fc.weighted_H64(src, corr, w, w)
        s = np.linalg.svd(H, compute_uv=False)
        assert np.abs(cs).max() > 2 and s[1] / s[0] > 1e-2 and (M == 3 or s[2] / s[0] > 1e-2)


@pytest.mark.parametrize("frame", ["up", "down"])
def test_power_of_two_frames_leave_the_oracle_unchanged(frame):
    N = 1000
    base = fc.base_cloud(B, N, 4100 + N)
    x, r = fc.apply(frame, base)
    assert np.array_equal(oracle.knn(x, 20), oracle.knn(base, 20))
    fps = oracle.furthest_point_sampling(base, 64)
    assert np.array_equal(oracle.furthest_point_sampling(x, 64), fps)
    cen = np.stack([base[b][fps[b]] for b in range(B)])
    cx, _ = fc.apply(frame, cen)
    assert np.array_equal(oracle.ball_query(r, 16, x, cx), oracle.ball_query(fc.R_UNIT, 16, base, cen))
