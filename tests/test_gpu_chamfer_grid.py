"""Chamfer search with exact grid pruning (chamfer_grid.hip: l3d_chamfer_forward_variant 4, and what auto = variant 1 picks inside
its size window) against the per-candidate kernels (variant 0) and, for the first cloud of a batch, oracle.chamfer_forward:
distances AND indices must be identical.  The inputs go after the cell function's rounding (coordinates on cell edges +- 1 ulp,
far offsets), the grid's degenerate shapes (zero extents, one-point clouds), exact ties, and both ways out of the pruning: the
fallback list (some queries, every query) and the whole-workgroup exact scan (non-finite coordinates).  The counters of
l3d_chamfer_forward_grid_stats say which way a case went."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _outputs(B, N, M, fill=None):
    d1, d2 = torch.empty((B, N), device="cuda"), torch.empty((B, M), device="cuda")
    i1, i2 = torch.empty((B, N), dtype=torch.int32, device="cuda"), torch.empty((B, M), dtype=torch.int32, device="cuda")
    if fill is not None:
        d1.fill_(fill); d2.fill_(fill); i1.fill_(-1); i2.fill_(-1)
    return d1, d2, i1, i2


def run(ta, tb, variant, expect=0):
    from learning3d_amd._lib import check, lib, ptr, stream_ptr
    B, N, M = ta.shape[0], ta.shape[1], tb.shape[1]
    out = _outputs(B, N, M)
    rc = lib().l3d_chamfer_forward_variant(ptr(ta), ptr(tb), B, N, M, *[ptr(o) for o in out], variant, stream_ptr())
    if expect != 0:
        assert rc == expect
        return None
    check(rc, "chamfer")
    return [o.cpu().numpy() for o in out]


def run_stats(ta, tb, fill=None):
    """l3d_chamfer_forward_grid_stats, bound here by name (l3d_hip_testing.h describes it without declaring it)"""
    import ctypes as C
    from learning3d_amd._lib import check, lib, ptr, stream_ptr
    fn = lib().l3d_chamfer_forward_grid_stats
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
    B, N, M = ta.shape[0], ta.shape[1], tb.shape[1]
    out = _outputs(B, N, M, fill)
    stats = torch.zeros(3, dtype=torch.int32, device="cuda")
    check(fn(ptr(ta), ptr(tb), B, N, M, *[ptr(o) for o in out], ptr(stats), stream_ptr()), "chamfer_grid_stats")
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out], [int(v) for v in stats.cpu()]


def same(got, want, what):
    for g, w, name in zip(got, want, ("dist1", "dist2", "idx1", "idx2")):
        assert np.array_equal(g, w, equal_nan=g.dtype == F), (what, name, int((g != w).sum()))


def check_case(a, b, with_oracle=True):
    """variant 4, variant 1 and the counting instantiation against variant 0 (and the oracle on the first cloud) -> the counters"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    want = run(ta, tb, 0)
    same(run(ta, tb, 4), want, "variant 4")
    same(run(ta, tb, 1), want, "variant 1")
    got, stats = run_stats(ta, tb)
    same(got, want, "stats instantiation")
    if with_oracle:
        same([w[:1] for w in want], oracle.chamfer_forward(a[:1], b[:1]), "oracle")
    return stats


def snapped(rng, shape):
    """multiples of 1/8 in [0, 1], half of them one ulp up or down"""
    v = (rng.integers(0, 9, shape) / 8.0).astype(F)
    k = rng.integers(0, 4, shape)
    return np.where(k == 0, np.nextafter(v, F(2)), np.where(k == 1, np.nextafter(v, F(-1)), v)).astype(F)


@pytest.mark.parametrize("B,N,M", [(1, 1, 5), (2, 77, 130), (3, 1024, 1000), (1, 2048, 300), (32, 1024, 1024), (8, 1100, 2048)])
def test_grid_chamfer_sizes(B, N, M):
    """B = 1 and 3, G from 1 to 10; the last two shapes are inside the window where variant 1 picks this kernel by itself (the first of
    them is the bench step's)"""
    rng = np.random.default_rng(N + M)
    stats = check_case(rng.random((B, N, 3)), rng.random((B, M, 3)))
    if N > 1:
        assert stats[0] + stats[1] == B * (N + M) and stats[2] == 0
    else:                                                         # a one-point candidate cloud has no extent: the whole-workgroup scan
        assert stats[0] + stats[1] == B * N and stats[2] == B


def test_grid_chamfer_size_limit():
    rng = np.random.default_rng(1)
    a, b = rng.random((1, 2049, 3)).astype(F), rng.random((1, 700, 3)).astype(F)
    from learning3d_amd import _lib
    for x, y in ((a, b), (b, a)):
        tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        run(tx, ty, 4, expect=_lib.L3D_ERR_UNSUPPORTED)
        want = run(tx, ty, 0)
        same(run(tx, ty, 1), want, "variant 1")
        same(want, oracle.chamfer_forward(x, y), "oracle")


def test_grid_chamfer_ties_lowest_index_wins():
    rng = np.random.default_rng(2)
    dup = rng.random((1, 300, 3))
    check_case(rng.random((1, 200, 3)), np.concatenate([dup, dup, dup], 1))
    check_case(np.concatenate([dup, dup, dup], 1), np.concatenate([dup, dup], 1))


def test_grid_chamfer_degenerate_extents():
    rng = np.random.default_rng(3)
    stats = check_case(rng.random((2, 500, 3)), np.full((2, 700, 3), 0.25))
    assert stats[2] > 0                                           # ext == 0 in one direction: the whole-workgroup exact scan
    flat = rng.random((2, 600, 3)); flat[..., 2] = 0.125
    check_case(rng.random((2, 500, 3)), flat)
    check_case(flat, flat[:, ::-1].copy())
    line = rng.random((2, 600, 1)) * np.array([1.0, 2.0, -0.5]) + 0.1
    check_case(rng.random((2, 500, 3)), line)
    check_case(line, line[:, ::-1].copy())


def test_grid_chamfer_cell_edges():
    rng = np.random.default_rng(4)
    a, b = snapped(rng, (2, 1024, 3)), snapped(rng, (2, 1024, 3))
    a[:, 0], a[:, 1], b[:, 0], b[:, 1] = 0.0, 1.0, 0.0, 1.0
    check_case(a, b)


def test_grid_chamfer_fallback_partial():
    rng = np.random.default_rng(5)
    b = np.concatenate([rng.random((2, 512, 3)) * 0.01, 1.0 - rng.random((2, 512, 3)) * 0.01], 1)
    stats = check_case(rng.random((2, 1024, 3)), b)
    assert stats[1] > 0 and stats[2] == 0


def test_grid_chamfer_fallback_all_queries():
    """queries in [2, 3]^3, candidates in [0, 1]^3, and the reverse in the launch's other direction: every query's 27 cells hold
    nothing nearer than the clouds' gap, so every query goes to the list -- the bounded all-pairs pass"""
    rng = np.random.default_rng(6)
    stats = check_case(rng.random((2, 600, 3)) + 2.0, rng.random((2, 1024, 3)))
    assert stats == [0, 2 * (600 + 1024), 0]


def test_grid_chamfer_far_offsets():
    rng = np.random.default_rng(7)
    check_case(rng.random((2, 900, 3)) * 1e-3 + 1000.0, rng.random((2, 1100, 3)) * 1e-3 + 1000.0)


def test_grid_chamfer_non_finite_inputs():
    rng = np.random.default_rng(8)
    a, b = rng.random((2, 900, 3)).astype(F), rng.random((2, 1100, 3)).astype(F)
    b[0, 17, 1] = np.nan
    a[1, 5, 0] = np.inf
    stats = check_case(a, b, with_oracle=False)                   # the oracle seeds its scan with candidate 0: another NaN convention
    assert stats[2] > 0


def test_grid_chamfer_pruning_is_real():
    rng = np.random.default_rng(9)
    stats = check_case(rng.random((3, 1024, 3)), rng.random((3, 1024, 3)))
    assert stats[0] >= 0.9 * (2 * 3 * 1024) and stats[2] == 0


def test_grid_chamfer_is_stateless():
    rng = np.random.default_rng(10)
    ta = torch.from_numpy(rng.random((2, 1000, 3)).astype(F)).cuda()
    tb = torch.from_numpy(rng.random((2, 1024, 3)).astype(F)).cuda()
    first, s1 = run_stats(ta, tb, fill=float("nan"))
    second, s2 = run_stats(ta, tb, fill=float("nan"))
    same(first, second, "second call")
    same(first, run(ta, tb, 0), "variant 0")
    assert s1 == s2


def test_grid_chamfer_residency_beside_knn():
    """both instantiations beside two knn_mfma_kernel<8> workgroups on a CU at N = 1024 (tests/test_knn_mfma_residency.py's budget):
    static LDS <= 160 KB - 2 x kNN's, <= 128 VGPRs, no scratch"""
    import ctypes
    from learning3d_amd import _lib
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    meta = km.kernel_metadata(_lib.LIB_PATH)
    f = getattr(_lib.lib(), "_Z22l3d_knn_mfma_lds_bytesi")
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int]
    knn_lds = int(f(1024))
    ks = [k for n, k in meta.items() if n.startswith("_Z23chamfer_fwd_grid_kernel")]
    assert len(ks) == 4                                           # product and counting instantiation, for up to 1024 and up to 2048 candidates
    for k in ks:
        assert k[".group_segment_fixed_size"] <= 163840 - 2 * knn_lds, k[".name"]
        assert k[".group_segment_fixed_size"] <= 44512, k[".name"]
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 128, k[".name"]
        assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0, k[".name"]
