"""chamfer_grid.hip's search restated in numpy float32, held against the oracle: the cell function, the nine runs of the sorted
image, the acceptance threshold and the fallback scan (steps 2-5 of the kernel's header comment).  Two things are checked:
(a) the bound -- no candidate outside a query's 27 cells has a computed distance below thr, on coordinates snapped to cell
edges +- 1 ulp, at offsets up to 10^2, scales 10^-3 .. 10^3 and G from 1 to 16; (b) the emulated search returns
oracle.chamfer_forward's distances and indices bit for bit, however the candidates are ordered inside a cell.  No GPU needed."""
import numpy as np
import pytest

import oracle

F = np.float32
ONE_M = F(1.0) - F(2.0) ** F(-12)


def grid_size(nc):
    g = 1
    for t in range(2, 13):
        if 2 * t * t * t <= nc:
            g = t
    return g


def cells(v, lo, s, G):
    """cell(v) = clamp((int)fl(fl(v - lo) * s), 0, G - 1) along every axis; v [n, 3]"""
    t = (v - lo).astype(F) * s
    return np.clip(np.trunc(np.clip(t.astype(F), F(-1e9), F(1e9))), 0, G - 1).astype(np.int64)


def dist(c, q):
    d = (c - q).astype(F)
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + d[:, 2] * d[:, 2]).astype(F)


def lexmin(d, idx):
    """(d, idx) of the lexicographic minimum; NaN never wins; no finite distance -> (inf, 0)"""
    ok = d < np.inf
    if not ok.any():
        return F(np.inf), 0
    d, idx = d[ok], idx[ok]
    m = d.min()
    return m, int(idx[d == m].min())


def grid_search(q, c, rng):
    """one direction of one cloud -> (dist [n], idx [n], accepted, listed, whole)"""
    n, m = len(q), len(c)
    dout, iout = np.empty(n, F), np.empty(n, np.int32)
    order = np.arange(m)
    with np.errstate(all="ignore"):
        lo = c.min(0)
        ext = F(np.max((c.max(0) - lo).astype(F)))
        G = grid_size(m)
        s, rinv = F(G) / ext, ext / F(G)
        r2 = F(rinv * rinv)
        thr = F(r2 * ONE_M)
        whole = not (np.isfinite(c).all() and np.isfinite(q).all()) or not (r2 >= F(1e-30) and r2 <= F(1e30))
        if whole:
            for i in range(n):
                dout[i], iout[i] = lexmin(dist(c, q[i]), order)
            return dout, iout, 0, 0, True
        cc = cells(c, lo, s, G)
        cid = (cc[:, 2] * G + cc[:, 1]) * G + cc[:, 0]
        perm = rng.permutation(m)                                  # the order inside a cell is whatever the atomics give
        perm = perm[np.argsort(cid[perm], kind="stable")]
        start = np.searchsorted(cid[perm], np.arange(G ** 3 + 1))
        img, imgi = c[perm], order[perm]
        qc = cells(q, lo, s, G)
        listed = 0
        for i in range(n):
            cx, cy, cz = qc[i]
            x0, x1 = max(cx - 1, 0), min(cx + 1, G - 1)
            sel = []
            for zz in range(cz - 1, cz + 2):
                for yy in range(cy - 1, cy + 2):
                    if 0 <= zz < G and 0 <= yy < G:
                        row = (zz * G + yy) * G
                        sel.append(np.arange(start[row + x0], start[row + x1 + 1]))
            sel = np.concatenate(sel)
            best, bi = lexmin(dist(img[sel], q[i]), imgi[sel]) if len(sel) else (F(np.inf), 0)
            if not best < thr:
                listed += 1
                best, bi = lexmin(dist(img, q[i]), imgi)
            dout[i], iout[i] = best, bi
    return dout, iout, n - listed, listed, False


def check_against_oracle(a, b, seed=0):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    rng = np.random.default_rng(seed)
    o1, o2, oi1, oi2 = oracle.chamfer_forward(a[None], b[None])
    d1, i1, acc1, lst1, w1 = grid_search(a, b, rng)
    d2, i2, acc2, lst2, w2 = grid_search(b, a, rng)
    assert np.array_equal(d1, o1[0], equal_nan=True) and np.array_equal(d2, o2[0], equal_nan=True)
    assert np.array_equal(i1, oi1[0]) and np.array_equal(i2, oi2[0])
    return (acc1, lst1, w1), (acc2, lst2, w2)


def snapped(rng, n, G, lo, ext):
    """coordinates on cell edges of a G-grid over [lo, lo + ext], half of them moved by one ulp either way"""
    v = (F(lo) + rng.integers(0, G + 1, (n, 3)).astype(F) * (F(ext) / F(G))).astype(F)
    up = np.nextafter(v, F(np.inf)); dn = np.nextafter(v, F(-np.inf))
    k = rng.integers(0, 4, (n, 3))
    return np.where(k == 0, up, np.where(k == 1, dn, v)).astype(F)


@pytest.mark.parametrize("G", [1, 2, 3, 5, 8, 12, 16])
def test_no_candidate_outside_the_block_is_below_the_threshold(G):
    rng = np.random.default_rng(100 + G)
    worst = np.inf
    for scale in (1e-3, 1.0, 1e3):
        for offset in (0.0, -3.0, 100.0):
            lo0, ext0 = offset * scale, scale
            for kind in ("snapped", "uniform"):
                if kind == "snapped":
                    c, q = snapped(rng, 160, G, lo0, ext0), snapped(rng, 160, G, lo0, ext0)
                else:
                    c = (F(lo0) + rng.random((160, 3)).astype(F) * F(ext0)).astype(F)
                    q = (F(lo0) + (rng.random((160, 3)).astype(F) * F(1.6) - F(0.3)) * F(ext0)).astype(F)     # some outside the box
                lo = c.min(0)
                ext = F(np.max((c.max(0) - lo).astype(F)))
                s, rinv = F(G) / ext, ext / F(G)
                thr = F(F(rinv * rinv) * ONE_M)
                cc, qc = cells(c, lo, s, G), cells(q, lo, s, G)
                outside = (np.abs(cc[None, :, :] - qc[:, None, :]) >= 2).any(-1)              # [q, c]
                d = (c[None, :, :] - q[:, None, :]).astype(F)
                dd = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(F) + d[..., 2] * d[..., 2]).astype(F)
                if outside.any():
                    assert (dd[outside] >= thr).all(), (G, scale, offset, kind)
                    worst = min(worst, float((dd[outside].astype(np.float64) / np.float64(thr)).min()))
    if G > 2:
        assert worst < 1.5          # the cases do reach the bound's neighbourhood: the check above is not vacuous


def test_grid_size_rule():
    assert [grid_size(n) for n in (1, 15, 16, 53, 54, 1023, 1024, 1457, 1458, 2000, 2048, 3455, 3456, 100000)] == \
        [1, 1, 2, 2, 3, 7, 8, 8, 9, 10, 10, 11, 12, 12]


@pytest.mark.parametrize("n,m", [(1, 5), (77, 130), (1024, 1000), (300, 2048)])
def test_uniform_clouds_equal_the_oracle(n, m):
    rng = np.random.default_rng(n + m)
    (acc1, lst1, w1), _ = check_against_oracle(rng.random((n, 3)), rng.random((m, 3)))
    if m >= 1000:
        assert not w1 and acc1 >= 0.9 * n               # the pruning is real on a uniform cloud


def test_cell_edge_coordinates_equal_the_oracle():
    rng = np.random.default_rng(5)
    a, b = snapped(rng, 600, 8, 0.0, 1.0), snapped(rng, 640, 8, 0.0, 1.0)
    a[0], a[1], b[0], b[1] = 0.0, 1.0, 0.0, 1.0
    check_against_oracle(a, b)


def test_far_offsets_small_extents_equal_the_oracle():
    rng = np.random.default_rng(6)
    a = (rng.random((500, 3)) * 1e-3 + 1000.0).astype(F)
    b = (rng.random((700, 3)) * 1e-3 + 1000.0).astype(F)
    check_against_oracle(a, b)


def test_duplicated_points_lowest_index_wins():
    rng = np.random.default_rng(7)
    dup = rng.random((300, 3))
    (_, _, _), (_, _, _) = check_against_oracle(rng.random((200, 3)), np.concatenate([dup, dup, dup]))
    check_against_oracle(np.concatenate([dup, dup, dup]), np.concatenate([dup, dup]))


def test_degenerate_extents_equal_the_oracle():
    rng = np.random.default_rng(8)
    (_, _, w), _ = check_against_oracle(rng.random((200, 3)), np.full((300, 3), 0.25))
    assert w                                            # ext == 0: the exact scan for the whole block
    flat = rng.random((400, 3)); flat[:, 2] = 0.125
    check_against_oracle(rng.random((200, 3)), flat)
    line = np.outer(rng.random(400), [1.0, 2.0, -0.5]) + 0.1
    check_against_oracle(rng.random((200, 3)), line)


def test_two_clusters_send_some_queries_to_the_fallback():
    rng = np.random.default_rng(9)
    b = np.concatenate([rng.random((512, 3)) * 0.01, 1.0 - rng.random((512, 3)) * 0.01])
    (acc, lst, w), _ = check_against_oracle(rng.random((512, 3)), b)
    assert not w and lst > 0 and acc + lst == 512


def test_queries_away_from_the_candidates_all_fall_back():
    rng = np.random.default_rng(10)
    (acc, lst, w), _ = check_against_oracle(rng.random((300, 3)) + 2.0, rng.random((1024, 3)))
    assert not w and acc == 0 and lst == 300


def test_non_finite_coordinates_take_the_exact_scan():
    """the kernels' convention for a query without a finite distance is (inf, 0) (chamfer_fwd_kernel); the oracle seeds its scan
    with candidate 0 and returns that NaN, so the non-finite query's own row is held to the convention and every other row to
    the oracle"""
    rng = np.random.default_rng(11)
    a, b = rng.random((200, 3)).astype(F), rng.random((300, 3)).astype(F)
    b[17, 1] = np.nan
    a[5, 0] = np.inf
    o1, o2, oi1, oi2 = oracle.chamfer_forward(a[None], b[None])
    d1, i1, _, _, w1 = grid_search(a, b, rng)
    d2, i2, _, _, w2 = grid_search(b, a, rng)
    assert w1 and w2
    k1, k2 = np.arange(200) != 5, np.arange(300) != 17
    assert np.array_equal(d1[k1], o1[0][k1]) and np.array_equal(i1[k1], oi1[0][k1])
    assert np.array_equal(d2[k2], o2[0][k2]) and np.array_equal(i2[k2], oi2[0][k2])
    assert d1[5] == np.inf and i1[5] == 0 and d2[17] == np.inf and i2[17] == 0
