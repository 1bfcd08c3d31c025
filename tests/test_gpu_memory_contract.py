"""Every entry point of the C ABI held to the memory contract its header states (tests/golden/memory_contract.py): each case
launches one entry point with every writable tensor a guarded, exactly sized slice under two fills and asserts that the guards
are intact, the `const` operands unchanged and the outputs the same bits under both fills -- at the smallest shapes at which the
kernel has a partial tile, a padded tail or a second tile.  The entry points that take a workspace are also held to their value
bar at these shapes (a reference in fp64 torch or the oracle; each names the test its bar comes from).

Not marked gpu: the accounting test (every prototype has a case or is a stream-less EXEMPT) and the harness self-test (a fake
launch in torch that breaks one rule at a time; check() must name the parameter)."""
import ctypes as C
import math
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, ROOT)
import layout_audit                                                                     # noqa: E402
import memory_contract as mc                                                            # noqa: E402
from memory_contract import ContractError, Spec, check                                  # noqa: E402
from view_cases import assert_identical                                                 # noqa: E402

gpu = pytest.mark.gpu
F32, I32, I64, U8, F64 = torch.float32, torch.int32, torch.int64, torch.uint8, torch.float64
TINY = 2.0 ** -24


def rnd(*shape, seed=0, scale=1.0):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(3000 + seed)) * 2 - 1).mul_(scale).cuda()


def randn(*shape, seed=0, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(3500 + seed)).mul_(scale).cuda()


def rint(hi, *shape, seed=0, dtype=I64):
    return torch.randint(0, hi, shape, generator=torch.Generator().manual_seed(4000 + seed)).to(dtype).cuda()


def lib():
    from learning3d_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------------------
# the cases: id -> (entry points it launches through check(), function)
CASES = {}


def case(*entries):
    def register(f):
        assert f.__name__ not in CASES
        CASES[f.__name__] = (entries, f)
        return f
    return register


def simple(name, build, ident=None):
    """a case that is one check() with nothing to compare afterwards"""
    ident = ident or name[4:]
    assert ident not in CASES, ident
    CASES[ident] = ((name,), lambda: check(name, build()))


# --- kNN graph, scatter, EdgeConv gather, feature kNN ---------------------------------------------------------------------------
def _knn_graph(variant):
    def make():
        xyz = rnd(2, 257, 3, seed=1)
        if variant is None:
            return lambda a: (xyz, 2, 257, 5, a.out(I64, 2, 257, 5))
        return lambda a: (xyz, 2, 257, 5, a.out(I64, 2, 257, 5), variant)
    return make


simple("l3d_knn_graph", _knn_graph(None))
for _v in (0, 1, 2):
    simple("l3d_knn_graph_variant", _knn_graph(_v), f"knn_graph_variant_{_v}")


def _scatter_case(B, Cc, T, E, div, weighted, seed):
    """bar: tests/test_gpu_vector_scalar_routes.py::test_scatter_add_det_source_row_alignment -- every target's entries summed in
    ascending entry order in fp32: the same bits as the sequential sum"""
    src = randn(B, Cc, E // div, seed=seed)
    idx = rint(T, B, E, seed=seed, dtype=I32)
    w = (rnd(B, E, seed=seed + 1).abs_() + 0.5) if weighted else None
    n = lib().l3d_scatter_add_det_workspace_bytes(B, T, E)
    out = check("l3d_scatter_add_det", lambda a: (src, idx, w, B, Cc, T, E, div, a.bytes(n), a.f32(B, Cc, T)))["dst"]
    s, ix = src.cpu(), idx.cpu().long()
    wc = w.cpu() if weighted else None
    want = torch.zeros(B, Cc, T)
    for e in range(E):                                        # ascending entry order, fp32 adds
        v = s[:, :, e // div]
        if weighted:
            v = v * wc[:, e:e + 1]
        for b in range(B):
            want[b, :, ix[b, e]] += v[b]
    err = float((out.cpu().double() - want.double()).abs().max())
    print(f"scatter_add_det B={B} C={Cc} T={T} E={E} div={div} weighted={weighted}: max error against the sequential fp32 sum {err:g} (bar 0)")
    assert torch.equal(out.cpu(), want)


for _E in (1024, 1025, 3072, 3073):
    CASES[f"scatter_add_det_E{_E}"] = (("l3d_scatter_add_det",), (lambda E: lambda: _scatter_case(2, 3, 37, E, 1, False, E))(_E))
CASES["scatter_add_det_weighted_div3"] = (("l3d_scatter_add_det",), lambda: _scatter_case(2, 2, 41, 3 * 343, 3, True, 7))
CASES["scatter_add_det_E7169"] = (("l3d_scatter_add_det",), lambda: _scatter_case(1, 1, 19, 7169, 1, False, 8))


def _edge_gather_max():
    pq, idx = randn(2, 128, 130, seed=10), rint(130, 2, 130, 7, seed=10)
    return lambda a: (pq, idx, 2, 64, 130, 7, 1, a.f32(2, 64, 130), 64 * 130)


simple("l3d_edge_gather_max", _edge_gather_max)


def _knn_feature_case(k):
    """bar: tests/test_gpu_f16x2_per_output.py::test_feature_knn_per_query_tolerance -- each query's k-th returned distance within
    16 fp32 ulps of its own |x_i|^2 + |x_j|^2 of the exact k-th distance"""
    B, Cc, N = 2, 40, 130
    x = randn(B, Cc, N, seed=11)
    n = lib().l3d_knn_feature_workspace_bytes(B, Cc, N)
    idx = check("l3d_knn_feature", lambda a: (x, B, Cc, N, k, a.bytes(n), a.out(I64, B, N, k)))["idx"]
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    xd = x.double()
    sq = (xd ** 2).sum(1)
    d = sq[:, :, None] + sq[:, None, :] - 2 * torch.einsum("bci,bcj->bij", xd, xd)
    order = d.argsort(dim=-1, stable=True)
    kth = d.gather(-1, order[:, :, k - 1:k])[..., 0]
    sq_all = sq[:, None, :].expand(B, N, N)
    sq_kth = sq_all.gather(-1, order[:, :, k - 1:k])[..., 0]
    got = d.gather(-1, idx)
    sq_got = sq_all.gather(-1, idx).max(-1)[0]
    tol = 16 * TINY * (sq + torch.maximum(sq_kth, sq_got))
    excess = float(((got.max(-1)[0] - kth) / tol).max())
    print(f"knn_feature B={B} C={Cc} N={N} k={k}: worst k-th distance excess {excess:.3f} of the per-query tolerance (bar 1)")
    assert excess <= 1.0
    assert bool((got[..., 1:] - got[..., :-1] >= -tol[..., None]).all())
    assert all(len(set(row.tolist())) == k for row in idx.reshape(-1, k)[:64].cpu())


CASES["knn_feature_k20"] = (("l3d_knn_feature",), lambda: _knn_feature_case(20))
CASES["knn_feature_k21"] = (("l3d_knn_feature",), lambda: _knn_feature_case(21))


def _graph_feature():
    x, idx = rnd(2, 33, 5, seed=12), rint(33, 2, 33, 3, seed=12)
    return lambda a: (x, idx, 2, 33, 5, 3, a.f32(2, 33, 3, 10))


simple("l3d_graph_feature", _graph_feature)


# --- Chamfer ------------------------------------------------------------------------------------------------------------------
def _chamfer_outputs(a, B, N, M):
    return a.f32(B, N), a.f32(B, M), a.out(I32, B, N), a.out(I32, B, M)


def _chamfer_forward(variant, B=2, N=130, M=77):
    def make():
        x1, x2 = rnd(B, N, 3, seed=20), rnd(B, M, 3, seed=21)
        tail = () if variant is None else (variant,)
        return lambda a: (x1, x2, B, N, M, *_chamfer_outputs(a, B, N, M), *tail)
    return make


simple("l3d_chamfer_forward", _chamfer_forward(None))
for _v in (0, 1, 2, 3, 4):
    simple("l3d_chamfer_forward_variant", _chamfer_forward(_v), f"chamfer_forward_variant_{_v}")
simple("l3d_chamfer_forward_variant", _chamfer_forward(4, 1, 1025, 1030), "chamfer_forward_variant_4_n1025")


@case(mc.GRID_STATS)
def chamfer_forward_grid_stats():
    B, N, M = 2, 130, 77
    x1, x2 = rnd(B, N, 3, seed=20), rnd(B, M, 3, seed=21)
    out = check(mc.GRID_STATS, lambda a: (x1, x2, B, N, M, *_chamfer_outputs(a, B, N, M), a.inout(torch.zeros(3, dtype=I32, device="cuda"))),
                launch=mc.launch_grid_stats)
    assert int(out["stats"].sum()) > 0, "the counters the caller zeroed were not added to"


def _chamfer_backward(variant):
    def make():
        B, N, M = 2, 130, 77
        x1, x2 = rnd(B, N, 3, seed=22), rnd(B, M, 3, seed=23)
        g1, g2 = rnd(B, N, seed=24), rnd(B, M, seed=25)
        i1, i2 = rint(M, B, N, seed=26, dtype=I32), rint(N, B, M, seed=27, dtype=I32)
        tail = () if variant is None else (variant,)
        return lambda a: (x1, x2, B, N, M, g1, g2, i1, i2, a.f32(B, N, 3), a.f32(B, M, 3), *tail)
    return make


simple("l3d_chamfer_backward", _chamfer_backward(None))
for _v in (0, 1, 2):
    simple("l3d_chamfer_backward_variant", _chamfer_backward(_v), f"chamfer_backward_variant_{_v}")


def _dists(B, N, M, seed):
    return rnd(B, N, seed=seed).abs_(), rnd(B, M, seed=seed + 1).abs_()


def _chamfer_partials():
    d1, d2 = _dists(3, 77, 130, 30)
    return lambda a: (d1, d2, 3, 77, 130, a.out(F64, 4))


def _chamfer_combine():
    p = torch.tensor([[3.0, 4.0, 10.0, 20.0], [1.0, 2.0, 5.0, 7.0], [0.5, 0.25, 1.0, 3.0]], dtype=F64).cuda()
    return lambda a: (p, 3, a.f32(1))


simple("l3d_chamfer_partials", _chamfer_partials)
simple("l3d_chamfer_combine", _chamfer_combine)


def _loss_fp64(d1, d2):
    return float((d1.double().sqrt().mean() + d2.double().sqrt().mean()) / 2)


@case("l3d_chamfer_loss_local_mb")
def chamfer_loss_local_mb():
    """bar: tests/test_gpu_parity.py::test_chamfer_loss_local_equals_partials_plus_combine -- |loss - fp64| < 1e-6"""
    for (B, N, M) in ((3, 77, 130), (1, 5, 2)):
        d1, d2 = _dists(B, N, M, 32)
        n = lib().l3d_chamfer_loss_local_ws_bytes()
        out = check("l3d_chamfer_loss_local_mb", lambda a: (d1, d2, B, N, M, a.bytes(n, zero_first=8, key="ws"), a.out(F64, 4), a.f32(1)))
        want = _loss_fp64(d1, d2)
        err = abs(float(out["loss"][0]) - want)
        print(f"chamfer_loss_local_mb B={B} N={N} M={M}: |loss - fp64| = {err:g} (bar 1e-6)")
        assert err < 1e-6
        assert out["partial"][2] == B * N and out["partial"][3] == B * M


def _chamfer_exact(x1, x2):
    """d = (dx*dx + dy*dy) + dz*dz in fp32 without contraction, the nearest candidate of every query (lowest index on ties)"""
    d1, i1 = [], []
    for b in range(x1.shape[0]):
        diff = x1[b][:, None, :] - x2[b][None, :, :]
        sq = diff * diff
        d = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
        m = d.min(dim=1, keepdim=True)[0]
        first = (d == m).float().argmax(dim=1)
        d1.append(m[:, 0])
        i1.append(first.to(I32))
    return torch.stack(d1), torch.stack(i1)


def _forward_loss_case(B, N, M):
    """bar: tests/test_gpu_parity.py::test_chamfer_forward_loss_one_launch_equals_search_plus_tail -- distances and indices bit for
    bit, |loss - fp64 of the distances| < 1e-6"""
    x1, x2 = rnd(B, N, 3, seed=34), rnd(B, M, 3, seed=35)
    n = lib().l3d_chamfer_forward_loss_ws_bytes(B, N, M)
    out = check("l3d_chamfer_forward_loss", lambda a: (x1, x2, B, N, M, *_chamfer_outputs(a, B, N, M), a.bytes(n, zero_first=16, key="ws"),
                                                       a.out(F64, 4), a.f32(1)))
    wd1, wi1 = _chamfer_exact(x1, x2)
    wd2, wi2 = _chamfer_exact(x2, x1)
    assert torch.equal(out["dist1"], wd1) and torch.equal(out["dist2"], wd2)
    assert torch.equal(out["idx1"], wi1) and torch.equal(out["idx2"], wi2)
    err = abs(float(out["loss"][0]) - _loss_fp64(wd1, wd2))
    print(f"chamfer_forward_loss B={B} N={N} M={M}: distances and indices exact, |loss - fp64| = {err:g} (bar 1e-6)")
    assert err < 1e-6
    assert out["partial"][2] == B * N and out["partial"][3] == B * M


CASES["chamfer_forward_loss_two_launch"] = (("l3d_chamfer_forward_loss",), lambda: _forward_loss_case(2, 77, 130))
CASES["chamfer_forward_loss_one_launch"] = (("l3d_chamfer_forward_loss",), lambda: _forward_loss_case(32, 1024, 700))


# --- PointNet++ ops -----------------------------------------------------------------------------------------------------------
def _ball_query_case(b, n, m, r, ns, with_ws):
    """bar: tests/test_gpu_parity.py::test_ball_query_cell_list_equals_scanning_kernels -- the same indices in the same order; here
    against the fp64 statement of the op, on data with no pair within 1e-5 r^2 of the radius"""
    xyz, new = rnd(b, n, 3, seed=40), rnd(b, m, 3, seed=41)
    nbytes = b * (16 * n + 16448)
    idx = check("l3d_ball_query", lambda a: (b, n, m, r, ns, new, xyz, a.out(I32, b, m, ns), a.bytes(nbytes) if with_ws else None))["idx"]
    d = ((new.double()[:, :, None, :] - xyz.double()[:, None, :, :]) ** 2).sum(-1)
    r2 = float(np.float32(r)) ** 2
    assert not bool(((d - r2).abs() < 1e-5 * r2).any()), "a pair on the boundary: choose another seed"
    hit = d < r2
    rank = hit.cumsum(-1) - 1
    want = torch.zeros(b, m, ns, dtype=torch.int64, device="cuda")
    ar = torch.arange(n, device="cuda").expand(b, m, n)
    first = torch.where(hit.any(-1), hit.float().argmax(-1), torch.zeros((), dtype=torch.int64, device="cuda"))
    want[:] = first[..., None]
    sel = hit & (rank < ns)
    bb, mm, nn = sel.nonzero(as_tuple=True)
    want[bb, mm, rank[bb, mm, nn]] = ar[bb, mm, nn]
    wrong = int((idx.long() != want).sum())
    print(f"ball_query b={b} n={n} m={m} nsample={ns} workspace={with_ws}: {wrong} indices differ from the fp64 statement (bar 0)")
    assert wrong == 0


CASES["ball_query_scan"] = (("l3d_ball_query",), lambda: _ball_query_case(2, 130, 33, 0.4, 8, False))
CASES["ball_query_scan_n2049"] = (("l3d_ball_query",), lambda: _ball_query_case(2, 2049, 65, 0.2, 16, False))
CASES["ball_query_cell_list"] = (("l3d_ball_query",), lambda: _ball_query_case(2, 2049, 65, 0.2, 16, True))


def _pn2():
    b, c, n, npt, ns = 2, 5, 133, 17, 6
    pts = rnd(b, c, n, seed=42)
    idx2, idx1 = rint(n, b, npt, ns, seed=43, dtype=I32), rint(n, b, npt, seed=44, dtype=I32)
    go2, go1 = rnd(b, c, npt, ns, seed=45), rnd(b, c, npt, seed=46)
    return {
        "l3d_group_points": lambda a: (b, c, n, npt, ns, pts, idx2, a.f32(b, c, npt, ns)),
        "l3d_group_points_grad": lambda a: (b, c, n, npt, ns, go2, idx2, a.f32(b, c, n)),
        "l3d_gather_points": lambda a: (b, c, n, npt, pts, idx1, a.f32(b, c, npt)),
        "l3d_gather_points_grad": lambda a: (b, c, n, npt, go1, idx1, a.f32(b, c, n)),
    }


for _n in ("l3d_group_points", "l3d_group_points_grad", "l3d_gather_points", "l3d_gather_points_grad"):
    simple(_n, (lambda n: lambda: _pn2()[n])(_n))


def _fps(with_temp, n=300):
    def make():
        pts = rnd(2, n, 3, seed=47)
        return lambda a: (2, n, 17, pts, a.f32(2, n) if with_temp else None, a.out(I32, 2, 17))
    return make


simple("l3d_furthest_point_sampling", _fps(True), "furthest_point_sampling_temp")
simple("l3d_furthest_point_sampling", _fps(False), "furthest_point_sampling_no_temp")
simple("l3d_furthest_point_sampling", _fps(True, 16385), "furthest_point_sampling_n16385")


def _knn(variant, n=70, m=130, k=4):
    def make():
        q, c = rnd(2, n, 3, seed=48), rnd(2, m, 3, seed=49)
        tail = () if variant is None else (variant,)
        return lambda a: (2, n, m, k, q, c, a.f32(2, n, k), a.out(I32, 2, n, k), *tail)
    return make


simple("l3d_knn", _knn(None))
simple("l3d_knn", _knn(None, 70, 1030, 33), "knn_selection_route")
for _v in (0, 1, 2, 3):
    simple("l3d_knn_variant", _knn(_v), f"knn_variant_{_v}")
simple("l3d_knn_variant", _knn(1, 9, 3, 5), "knn_variant_1_k_past_m")


def _three():
    b, c, m, n = 2, 5, 33, 131
    q, kn, pts = rnd(b, n, 3, seed=50), rnd(b, m, 3, seed=51), rnd(b, c, m, seed=52)
    idx, w = rint(m, b, n, 3, seed=53, dtype=I32), rnd(b, n, 3, seed=54).abs_()
    skip, go = rnd(b, 4, n, seed=55), rnd(b, c, n, seed=56)
    return {
        "l3d_three_nn": lambda a: (b, n, m, q, kn, a.f32(b, n, 3), a.out(I32, b, n, 3)),
        "l3d_three_interpolate": lambda a: (b, c, m, n, pts, idx, w, a.f32(b, c, n)),
        "l3d_three_interpolate_concat": lambda a: (b, c, m, n, pts, idx, w, skip, 4, a.f32(b, c + 4, n)),
        "l3d_three_interpolate_grad": lambda a: (b, c, n, m, go, idx, w, a.f32(b, c, m)),
    }


for _n in ("l3d_three_nn", "l3d_three_interpolate", "l3d_three_interpolate_concat", "l3d_three_interpolate_grad"):
    simple(_n, (lambda n: lambda: _three()[n])(_n))


def _three_interpolate_concat_no_skip():
    b, c, m, n = 2, 5, 33, 131
    pts, idx, w = rnd(b, c, m, seed=52), rint(m, b, n, 3, seed=53, dtype=I32), rnd(b, n, 3, seed=54).abs_()
    return lambda a: (b, c, m, n, pts, idx, w, None, 0, a.f32(b, c, n))


simple("l3d_three_interpolate_concat", _three_interpolate_concat_no_skip, "three_interpolate_concat_no_skip")


# --- torch-level primitives ---------------------------------------------------------------------------------------------------
def _common():
    B, N, M, K = 2, 131, 67, 6
    x, q = rnd(B, N, 3, seed=60), rnd(B, M, 3, seed=61)
    it = rint(N, B, M, seed=62)
    pts, ix = rnd(B, N, 7, seed=63), rint(N, B, 40, seed=64)
    start = rint(N, B, seed=65)
    return {
        "square_distance": ("l3d_square_distance", lambda a: (x, q, B, N, M, 3, a.f32(B, N, M))),
        "gaussian_density": ("l3d_gaussian_density", lambda a: (x, B, N, 0.2, a.f32(B, N))),
        "query_ball_point_cnt": ("l3d_query_ball_point", lambda a: (0.5, K, x, q, B, N, M, None, a.out(I64, B, M, K), a.out(I64, B, M))),
        "query_ball_point_itself": ("l3d_query_ball_point", lambda a: (0.5, K, x, q, B, N, M, it, a.out(I64, B, M, K), None)),
        "index_points": ("l3d_index_points", lambda a: (pts, ix, B, N, 7, 40, a.f32(B, 40, 7))),
        "farthest_point_sample": ("l3d_farthest_point_sample", lambda a: (x, B, N, 17, None, a.f32(B, N), a.out(I64, B, 17))),
        "farthest_point_sample_start_no_temp": ("l3d_farthest_point_sample", lambda a: (x, B, N, 17, start, None, a.out(I64, B, 17))),
        "knn_point": ("l3d_knn_point", lambda a: (K, x, q, B, N, M, a.f32(B, M, K), a.out(I64, B, M, K))),
        "knn_point_expanded": ("l3d_knn_point_expanded", lambda a: (K, x, q, B, N, M, a.out(I64, B, M, K))),
    }


def _register_common():
    names = {"square_distance": "l3d_square_distance", "gaussian_density": "l3d_gaussian_density", "query_ball_point_cnt": "l3d_query_ball_point",
             "query_ball_point_itself": "l3d_query_ball_point", "index_points": "l3d_index_points",
             "farthest_point_sample": "l3d_farthest_point_sample", "farthest_point_sample_start_no_temp": "l3d_farthest_point_sample",
             "knn_point": "l3d_knn_point", "knn_point_expanded": "l3d_knn_point_expanded"}
    for ident, name in names.items():
        CASES[ident] = ((name,), (lambda i: lambda: check(*_common()[i]))(ident))


_register_common()


def _grouping():
    B, N, S, K, Cc, C1 = 2, 131, 9, 7, 5, 12
    xyz, new = rnd(B, N, 3, seed=70), rnd(B, S, 3, seed=71)
    feat, cen = rnd(B, Cc, N, seed=72), rnd(B, 4, S, seed=73)
    idx = rint(N, B, S, K, seed=74, dtype=I32)
    U, V = rnd(B, N, C1, seed=75), rnd(B, S, C1, seed=76)
    shift, wx = rnd(C1, seed=77), rnd(C1, 3, seed=78)
    return {
        "group_concat": ("l3d_group_concat", lambda a: (xyz, new, feat, idx, B, N, S, K, Cc, 1, a.f32(B, 3 + Cc, S, K))),
        "group_concat_no_xyz": ("l3d_group_concat", lambda a: (xyz, new, feat, idx, B, N, S, K, Cc, 0, a.f32(B, Cc, S, K))),
        "group_concat_xyz_only": ("l3d_group_concat", lambda a: (xyz, new, None, idx, B, N, S, K, 0, 1, a.f32(B, 3, S, K))),
        "group_concat2_order0": ("l3d_group_concat2", lambda a: (xyz, new, feat, cen, idx, B, N, S, K, Cc, 4, 0, a.f32(B, 3 + Cc + 4, S, K))),
        "group_concat2_order1": ("l3d_group_concat2", lambda a: (xyz, new, feat, None, idx, B, N, S, K, Cc, 0, 1, a.f32(B, 3 + Cc, S, K))),
        "group_first_layer": ("l3d_group_first_layer", lambda a: (U, V, None, wx, xyz, new, idx, B, N, S, K, C1, 1, a.f32(B, S * K, C1))),
        "group_first_layer_shift": ("l3d_group_first_layer", lambda a: (U, None, shift, wx, xyz, new, idx, B, N, S, K, C1, 0, a.f32(B, S * K, C1))),
        "absmax4_partials": ("l3d_absmax4_partials", lambda a: (U, U.numel(), V, V.numel(), xyz, xyz.numel(), new, new.numel(), a.f32(256))),
        "absmax4_partials_absent": ("l3d_absmax4_partials", lambda a: (U, U.numel(), None, 0, xyz, xyz.numel(), new, new.numel(), a.f32(256))),
    }


for _id, _name in (("group_concat", "l3d_group_concat"), ("group_concat_no_xyz", "l3d_group_concat"), ("group_concat_xyz_only", "l3d_group_concat"),
                   ("group_concat2_order0", "l3d_group_concat2"), ("group_concat2_order1", "l3d_group_concat2"),
                   ("group_first_layer", "l3d_group_first_layer"), ("group_first_layer_shift", "l3d_group_first_layer"),
                   ("absmax4_partials", "l3d_absmax4_partials"), ("absmax4_partials_absent", "l3d_absmax4_partials")):
    CASES[_id] = ((_name,), (lambda i: lambda: check(*_grouping()[i]))(_id))


def _planes_auto_case(with_v):
    B, N, S, K, C1 = 2, 131, 5, 7, 64                         # 70 image rows: one block of 64 and a ragged one
    xyz, new = rnd(B, N, 3, seed=80), rnd(B, S, 3, seed=81)
    idx = rint(N, B, S, K, seed=82, dtype=I32)
    U, V = rnd(B, N, C1, seed=83), (rnd(B, S, C1, seed=84) if with_v else None)
    shift, wx = rnd(C1, seed=85), rnd(C1, 3, seed=86)
    part = torch.zeros(256, device="cuda")
    from learning3d_amd import _lib
    _lib.call("l3d_absmax4_partials", U, U.numel(), V, V.numel() if with_v else 0, xyz, xyz.numel(), new, new.numel(), part)
    wxr, shmax = float(wx.abs().sum(1).max()), float(shift.abs().max())
    n = lib().l3d_f16_image_bytes(1, B * S * K, C1)
    out = check("l3d_group_first_layer_planes_auto",
                lambda a: (U, V, None if with_v else shift, wx, xyz, new, idx, B, N, S, K, C1, 1, part, wxr, 0.0 if with_v else shmax,
                           a.bytes(n), a.inout(torch.zeros(1, dtype=I32, device="cuda"))))
    assert int(out["range_flag"][0]) == 0


CASES["group_first_layer_planes_auto"] = (("l3d_group_first_layer_planes_auto",), lambda: _planes_auto_case(True))
CASES["group_first_layer_planes_auto_shift"] = (("l3d_group_first_layer_planes_auto",), lambda: _planes_auto_case(False))


def _kabsch(with_h):
    def make():
        s, c = rnd(3, 3, 131, seed=90), rnd(3, 3, 131, seed=91)
        return lambda a: (s, c, 3, 131, a.f32(3, 3, 3), a.f32(3, 3), a.f32(3, 3, 3) if with_h else None)
    return make


simple("l3d_kabsch", _kabsch(True))
simple("l3d_kabsch", _kabsch(False), "kabsch_no_h")
simple("l3d_svd3x3_rotation", lambda: (lambda H: lambda a: (H, 5, a.f32(5, 3, 3)))(rnd(5, 3, 3, seed=92)))


def _softcorr_case(B, Cc, N, M):
    """bar: tests/test_gpu_parity.py::test_soft_correspondence_flash_vs_fp64 -- rtol 1e-5, atol 2e-6 against fp64"""
    q, k, v = randn(B, Cc, N, seed=93), randn(B, Cc, M, seed=94), rnd(B, 3, M, seed=95)
    n = lib().l3d_soft_correspondence_workspace_floats(B, N, M)
    scale = 1.0 / math.sqrt(Cc)
    got = check("l3d_soft_correspondence", lambda a: (q, k, v, B, Cc, N, M, scale, a.f32(n), a.f32(B, 3, N)))["src_corr"]
    s = torch.softmax(torch.einsum("bcn,bcm->bnm", q.double(), k.double()) * scale, dim=2)
    want = torch.einsum("bdm,bnm->bdn", v.double(), s)
    excess = float(((got.double() - want).abs() / (2e-6 + 1e-5 * want.abs())).max())
    print(f"soft_correspondence B={B} C={Cc} N={N} M={M}: worst error {excess:.3f} of (2e-6 + 1e-5 |want|) (bar 1)")
    assert excess <= 1.0


for _M in (511, 512, 513, 77):
    CASES[f"soft_correspondence_M{_M}"] = (("l3d_soft_correspondence",), (lambda M: lambda: _softcorr_case(2, 32, 129, M))(_M))


def _attention_reference(q, k, v, B, H, D, N, M, scale):
    q4, k4, v4 = q.double().view(B, H, D, N), k.double().view(B, H, D, M), v.double().view(B, H, D, M)
    s = torch.einsum("bhdn,bhdm->bhnm", q4, k4) * scale
    p = torch.softmax(s, dim=-1)
    want = torch.einsum("bhdm,bhnm->bhdn", v4, p)
    mag = torch.einsum("bhdm,bhnm->bhdn", v4.abs(), p)
    smag = torch.einsum("bhdn,bhdm->bhnm", q4.abs(), k4.abs()) * scale
    spread = torch.einsum("bhnm,bhnm,bhdm->bhdn", smag, p, v4.abs())
    return want.reshape(B, H * D, N), (mag + 2 * spread).reshape(B, H * D, N)


def _attention_strided():
    B, H, D, N, M = 2, 2, 64, 130, 77
    q, k, v = randn(B, H * D, N, seed=96), randn(B, H * D, M, seed=97), randn(B, H * D, M, seed=98)
    return lambda a: (q, k, v, B, H, D, N, M, H * D * N, H * D * M, H * D * M, 0.125, a.f32(B, H * D, N))


simple("l3d_attention_forward_strided", _attention_strided)


def _attention_f16b_case(N, M, mode):
    """bar: tests/test_gpu_f16x2_per_output.py::test_attention_f16b_per_query -- per query, max error <= 2 x the bf16x3 kernel's
    (l3d_attention_forward_strided) + 2^-24 (sum p |v| + 2 sum |s| p |v|)"""
    from learning3d_amd import _lib
    B, H, D = 2, 2, 64
    q, k, v = randn(B, H * D, N, seed=96), randn(B, H * D, M, seed=97), randn(B, H * D, M, seed=98)
    sc = 1.0 / math.sqrt(D)
    st = (H * D * N, H * D * M, H * D * M)
    maxima = torch.stack([q.abs().max(), k.abs().max(), v.abs().max(), torch.zeros((), device="cuda")]).view(I32)

    def ws(a):
        return a.inout(maxima) if mode == "maxima_ready" else a.bytes(16)
    if mode == "image":
        n = lib().l3d_f16_image_bytes(1, B * N, H * D)
        check("l3d_attention_forward_f16b", lambda a: (q, k, v, B, H, D, N, M, *st, sc, ws(a), 0, None, a.bytes(n)))
        check("l3d_attention_forward_f16b", lambda a: (q, k, v, B, H, D, N, M, *st, sc, ws(a), 2, None, a.bytes(n)))
        return
    contract = None
    if mode == "maxima_ready":
        contract = {"l3d_attention_forward_f16b": {"workspace": Spec("inout", "maxima_ready bit 0: workspace already holds the three maxima")}}
    got = check("l3d_attention_forward_f16b", lambda a: (q, k, v, B, H, D, N, M, *st, sc, ws(a), int(mode == "maxima_ready"), a.f32(B, H * D, N), None),
                contract=contract)["ctx"]
    ref = torch.empty_like(got)
    _lib.call("l3d_attention_forward_strided", q, k, v, B, H, D, N, M, *st, sc, ref)
    want, floor = _attention_reference(q, k, v, B, H, D, N, M, sc)
    g = lambda t: t.view(B, H, D, N).permute(0, 1, 3, 2).reshape(-1, D)                            # one group per (b, h, query)
    e, e32 = (g(got.double()) - g(want)).abs().max(1)[0], (g(ref.double()) - g(want)).abs().max(1)[0]
    ratio = float((e / (2.0 * e32 + TINY * g(floor).max(1)[0] + 2.0 ** -149)).max())
    print(f"attention_forward_f16b N={N} M={M} {mode}: worst per-query error {ratio:.3f} of the bar (2 x bf16x3's + the fp32 floor)")
    assert ratio <= 1.0


for _N, _M in ((256, 96), (130, 77), (257, 33)):
    CASES[f"attention_f16b_N{_N}_M{_M}"] = (("l3d_attention_forward_f16b",), (lambda N, M: lambda: _attention_f16b_case(N, M, "ctx"))(_N, _M))
CASES["attention_f16b_maxima_ready"] = (("l3d_attention_forward_f16b",), lambda: _attention_f16b_case(130, 77, "maxima_ready"))
CASES["attention_f16b_image"] = (("l3d_attention_forward_f16b",), lambda: _attention_f16b_case(130, 77, "image"))


def _layernorm(which):
    def make():
        rows, Cc = 17, 64
        x, sa, sb = randn(rows, Cc, seed=100), rnd(Cc, seed=101) + 1.5, rnd(Cc, seed=102)
        n = lib().l3d_f16_image_bytes(1, rows, Cc)
        return lambda a: (x, sa, sb, 1e-6, rows, Cc, a.f32(rows, Cc) if "y" in which else None, a.bytes(n) if "img" in which else None)
    return make


for _w in ("y", "y_img", "img"):
    simple("l3d_layernorm_planes", _layernorm(_w), f"layernorm_planes_{_w}")


def _layernorm_cf(which, flags):
    def make():
        B, Cc, N = 2, 128, 130
        x, sa, sb = randn(B, Cc, N, seed=103), rnd(Cc, seed=104) + 1.5, rnd(Cc, seed=105)
        n = lib().l3d_f16_image_bytes(1, B * N, Cc)
        return lambda a: (x, sa, sb, 1e-6, B, Cc, N, a.f32(B, Cc, N) if "y" in which else None, a.bytes(n) if "img" in which else None, flags)
    return make


simple("l3d_layernorm_planes_cf", _layernorm_cf("y", 0), "layernorm_planes_cf_y")
simple("l3d_layernorm_planes_cf", _layernorm_cf("y_img", 0), "layernorm_planes_cf_y_img")
simple("l3d_layernorm_planes_cf", _layernorm_cf("img", 1), "layernorm_planes_cf_img_unscaled")
simple("l3d_add_transposed", lambda: (lambda x, y: lambda a: (x, y, 2, 33, 35, a.f32(2, 33, 35)))(rnd(2, 33, 35, seed=106), rnd(2, 35, 33, seed=107)))


# --- EdgeConv and the 1x1 convs -----------------------------------------------------------------------------------------------
_EDGE = {}
EDGE_WIDTHS = (6, 64, 64, 128, 256)


def _edge_pack_build():
    """build(arena) of l3d_edgeconv_pack (a host function: CPU pointers, no launch) for seeded weights"""
    g = torch.Generator().manual_seed(5000)
    ws = [(torch.randn(EDGE_WIDTHS[i + 1], EDGE_WIDTHS[i], generator=g) / math.sqrt(EDGE_WIDTHS[i])).contiguous() for i in range(4)]
    scs = [torch.rand(EDGE_WIDTHS[i + 1], generator=g) + 0.5 for i in range(4)]
    shs = [torch.randn(EDGE_WIDTHS[i + 1], generator=g) * 0.1 for i in range(4)]
    nfl = lib().l3d_edgeconv_packed_floats(*EDGE_WIDTHS[1:])
    arr = lambda ts: (C.c_void_p * 4)(*[t.data_ptr() for t in ts])
    keep = (ws, scs, shs)                                # (the pointer arrays do not own the tensors)
    return lambda a, keep=keep: (arr(ws), arr(scs), arr(shs), (C.c_float * 4)(1.0, 1.0, 1.0, 1.0), *EDGE_WIDTHS[1:], a.f32(nfl))


def _edge_packed():
    if not _EDGE:
        from learning3d_amd import _lib
        arena = mc.Arena(mc.FILL_B, "cpu")
        build = _edge_pack_build()                       # (held until the call returns: it owns the tensors behind the pointer arrays)
        args = build(arena)
        _lib.call("l3d_edgeconv_pack", *args)
        del build
        _EDGE["packed"] = args[-1].cuda()
        _EDGE["v2"] = bool(args[-1][lib().l3d_edgeconv_packed_v2_flag_index()] == 1.0)
    return _EDGE["packed"], _EDGE["v2"]


# host entry points that write through a pointer: checked on the CPU, not marked gpu
HOST_CASES = {"edgeconv_pack": (("l3d_edgeconv_pack",), lambda: check("l3d_edgeconv_pack", _edge_pack_build(), device="cpu"))}


@pytest.mark.parametrize("ident", sorted(HOST_CASES))
def test_host_entry_point_keeps_its_memory_contract(ident):
    HOST_CASES[ident][1]()


def _edgeconv(name, mode=None):
    def make():
        B, N, k = 2, 70, 20
        xyz, idx = rnd(B, N, 3, seed=110), rint(N, B, N, k, seed=111)
        packed, v2 = _edge_packed()
        if name == "l3d_edgeconv_forward":
            return lambda a: (xyz, idx, B, N, k, packed, 64, 64, 128, 256, a.f32(B, N, 512))
        if name == "l3d_edgeconv_forward_split":
            return lambda a: (xyz, idx, B, N, k, packed, a.f32(B, N, 512))
        assert v2, "the packer could not place the seeded weights for the two-plane kernel"
        n = lib().l3d_f16_image_bytes(1, B * N, 512)
        flag = torch.zeros(1, dtype=I32, device="cuda")
        return lambda a: (xyz, idx, B, N, k, packed, a.f32(B, N, 512) if mode == 0 else a.bytes(n), mode, a.inout(flag))
    return make


simple("l3d_edgeconv_forward", _edgeconv("l3d_edgeconv_forward"))
simple("l3d_edgeconv_forward_split", _edgeconv("l3d_edgeconv_forward_split"))
_IMAGE_OUT = {"l3d_edgeconv_forward_f16b": {"range_flag": mc.RANGE_FLAG,
                                            "out": Spec("written", "out_mode 1, 2: an fp16 activation image of the pooled values", open=mc._image_tail)}}
CASES["edgeconv_forward_f16b_mode0"] = (("l3d_edgeconv_forward_f16b",), lambda: check("l3d_edgeconv_forward_f16b", _edgeconv("l3d_edgeconv_forward_f16b", 0)()))
for _m in (1, 2):
    CASES[f"edgeconv_forward_f16b_mode{_m}"] = (("l3d_edgeconv_forward_f16b",), (lambda m: lambda: check(
        "l3d_edgeconv_forward_f16b", _edgeconv("l3d_edgeconv_forward_f16b", m)(), contract=_IMAGE_OUT))(_m))


def _pointwise_conv(channel_last, pool, per_cloud):
    def make():
        B, Cin, Cout, N = 2, 5, 37, 136
        x = rnd(B, N, Cin, seed=120) if channel_last else rnd(B, Cin, N, seed=120)
        w, sc = rnd(Cout, Cin, seed=121), rnd(Cout, seed=122).abs_() + 0.5
        sh = rnd(B, Cout, seed=123) if per_cloud else rnd(Cout, seed=123)
        return lambda a: (x, int(channel_last), w, sc, sh, Cout if per_cloud else 0, B, Cin, Cout, N, 1, pool, a.f32(B, Cout, N // (pool or 1)))
    return make


simple("l3d_pointwise_conv", _pointwise_conv(False, 0, False), "pointwise_conv_channel_first")
simple("l3d_pointwise_conv", _pointwise_conv(True, 0, True), "pointwise_conv_channel_last_per_cloud_shift")
simple("l3d_pointwise_conv", _pointwise_conv(False, 8, False), "pointwise_conv_pool8")


def _pointwise_conv_narrow():
    B, Cin, Cout, N = 2, 32, 64, 131
    x, w = rnd(B, Cin, N, seed=124), rnd(Cout, Cin, seed=125)
    return lambda a: (x, 0, w, None, None, 0, B, Cin, Cout, N, 0, 0, a.f32(B, Cout, N))


simple("l3d_pointwise_conv", _pointwise_conv_narrow, "pointwise_conv_no_affine_c64")
simple("l3d_split_rows", lambda: (lambda s, n: lambda a: (s, 37, 21, a.bytes(n)))(rnd(37, 21, seed=126), lib().l3d_split_bytes(37, 21)))


def _conv_split(x_mode, pool):
    def make():
        from learning3d_amd import _lib
        B, Cin, Cout, N = 2, 16, 256, 256 if pool else 128           # (the pooled epilogue lives in the 256-point tile)
        w = rnd(Cout, Cin, seed=127)
        wimg = torch.empty(lib().l3d_split_bytes(Cout, Cin), dtype=U8, device="cuda")
        _lib.call("l3d_split_rows", w, Cout, Cin, wimg)
        x = rnd(B, Cin, N, seed=128) if x_mode == 0 else rnd(B, N, Cin, seed=128)
        if x_mode == 2:
            ximg = torch.empty(lib().l3d_split_bytes(B * N, Cin), dtype=U8, device="cuda")
            _lib.call("l3d_split_rows", x.view(B * N, Cin), B * N, Cin, ximg)
            x = ximg
        sc, sh = rnd(Cout, seed=129).abs_() + 0.5, rnd(Cout, seed=130)
        return lambda a: (x, x_mode, wimg, sc, sh, 0, B, Cin, Cout, N, 1, pool, a.f32(B, Cout, N // (pool or 1)))
    return make


for _xm in (0, 1, 2):
    simple("l3d_pointwise_conv_split", _conv_split(_xm, 0), f"pointwise_conv_split_x_mode{_xm}")
simple("l3d_pointwise_conv_split", _conv_split(0, 64), "pointwise_conv_split_pool64")
simple("l3d_conv_f16_split_weights", lambda: (lambda w, n: lambda a: (w, 128, 48, a.bytes(n)))(rnd(128, 48, seed=131), lib().l3d_f16_image_bytes(2, 128, 48)))
simple("l3d_conv_f16_split_weights", lambda: (lambda w, n: lambda a: (w, 130, 20, a.bytes(n)))(rnd(130, 20, seed=131), lib().l3d_f16_image_bytes(2, 130, 20)),
       "conv_f16_split_weights_padded_rows")
simple("l3d_linear_rows", lambda: (lambda x, w, b: lambda a: (x, w, b, 3, 256, 17, 1, a.f32(3, 17)))(rnd(3, 256, seed=132), rnd(17, 256, seed=133),
                                                                                                      rnd(17, seed=134)))


def _flag(a):
    return a.inout(torch.zeros(1, dtype=I32, device="cuda"))


def _split_f16_rows(channel_first):
    def make():
        B, N, Cc = 2, 65, 40
        x = rnd(B, Cc, N, seed=135) if channel_first else rnd(B, N, Cc, seed=135)
        n = lib().l3d_f16_image_bytes(1, B * N, Cc)
        return lambda a: (x, B * N, Cc, int(channel_first), N, a.bytes(n), _flag(a))
    return make


simple("l3d_split_f16_rows", _split_f16_rows(False), "split_f16_rows_channel_last")
simple("l3d_split_f16_rows", _split_f16_rows(True), "split_f16_rows_channel_first")


def _split_f16_operand(kind):
    def make():
        rows, Cc = 65, 40
        wide = rnd(rows, Cc + 8, seed=136)
        n = lib().l3d_f16_image_bytes(1 + kind, rows, Cc)
        return lambda a: (wide[:, :Cc], rows, Cc, Cc + 8, kind, a.bytes(n), _flag(a))
    return make


simple("l3d_split_f16_operand", _split_f16_operand(0), "split_f16_operand_kind0")
simple("l3d_split_f16_operand", _split_f16_operand(1), "split_f16_operand_kind1")


def _first_layer_planes(channel_last):
    def make():
        B, Cin, Cout, N = 2, 3, 128, 130
        x = rnd(B, N, Cin, seed=137) if channel_last else rnd(B, Cin, N, seed=137)
        w, sh, xmax = rnd(Cout, Cin, seed=138), rnd(Cout, seed=139), torch.ones(1, device="cuda")
        n = lib().l3d_f16_image_bytes(1, B * N, Cout)
        return lambda a: (x, int(channel_last), w, sh, xmax, B, Cin, Cout, N, 1, a.bytes(n), _flag(a))
    return make


simple("l3d_first_layer_f16_planes", _first_layer_planes(True), "first_layer_f16_planes_channel_last")
simple("l3d_first_layer_f16_planes", _first_layer_planes(False), "first_layer_f16_planes_channel_first")


def _conv_f16(what, two_plane=False, Cout=256, N=256, B=2, per_cloud=False):
    """one output combination of l3d_pointwise_conv_f16's comment; the operand images are made by the library's own split kernels"""
    def make():
        from learning3d_amd import _lib
        Cin = 32
        x, w = rnd(B * N, Cin, seed=140), rnd(Cout, Cin, seed=141, scale=0.3)
        ximg = torch.empty(lib().l3d_f16_image_bytes(1, B * N, Cin), dtype=U8, device="cuda")
        if two_plane:
            _lib.call("l3d_split_f16_operand", x, B * N, Cin, Cin, 0, ximg, None)
        else:
            _lib.call("l3d_split_f16_rows", x, B * N, Cin, 0, N, ximg, None)
        wimg = torch.empty(lib().l3d_f16_image_bytes(2, Cout, Cin), dtype=U8, device="cuda")
        _lib.call("l3d_conv_f16_split_weights", w, Cout, Cin, wimg)
        sc = rnd(Cout, seed=142).abs_() + 0.5
        sh = rnd(B, Cout, seed=143) if per_cloud else rnd(Cout, seed=143)
        obs = torch.stack([sh.abs().max(), sc.abs().max()])
        res = rnd(B, Cout, N, seed=144)
        nimg = lib().l3d_f16_image_bytes(1, B * N, Cout)
        flags = 1 if two_plane else 0
        head = (ximg, wimg, sc, sh, Cout if per_cloud else 0, B, Cin, Cout, N, 1)
        if what == "y":
            return lambda a: (*head, flags, a.f32(B, Cout, N), None, None, None, None, 0, None, 0)
        if what == "residual":
            return lambda a: (*head, flags, a.f32(B, Cout, N), res, None, None, None, 0, None, 0)
        if what == "out_img":
            return lambda a: (*head, flags | (2 if two_plane else 0), None, None, a.bytes(nimg), obs, None, 0, None, 0)
        if what == "ypool":
            return lambda a: (*head, flags, None, None, None, None, a.f32(B, Cout, N // 8), 8, None, 0)
        if what == "ypool128":
            return lambda a: (*head, flags, None, None, None, None, a.f32(B, Cout, N // 128), 128, None, 0)
        if what == "out_img_ypool":
            return lambda a: (*head, flags, None, None, a.bytes(nimg), obs, a.f32(B, Cout, N // 128), 128, None, 0)
        assert what == "amax"
        return lambda a: (*head, flags, a.f32(B, Cout, N), None, None, None, None, 0, a.inout(torch.zeros(Cout // 256, dtype=I32, device="cuda")), 256)
    return make


for _what in ("y", "residual", "out_img", "ypool", "ypool128", "out_img_ypool", "amax"):
    simple("l3d_pointwise_conv_f16", _conv_f16(_what), f"pointwise_conv_f16_{_what}")
for _what in ("y", "residual", "out_img", "amax"):
    simple("l3d_pointwise_conv_f16", _conv_f16(_what, two_plane=True), f"pointwise_conv_f16_two_plane_{_what}")
simple("l3d_pointwise_conv_f16", _conv_f16("y", Cout=128, N=512, B=1), "pointwise_conv_f16_narrow_y")
simple("l3d_pointwise_conv_f16", _conv_f16("ypool", Cout=128, N=512, B=1), "pointwise_conv_f16_narrow_ypool")
simple("l3d_pointwise_conv_f16", _conv_f16("y", Cout=512, per_cloud=True), "pointwise_conv_f16_per_cloud_shift")


def _conv_f16_shift_n():
    """the rows-as-weights product of l3d_split_f16_operand's comment: y [rows][Cout] = x W^T + b"""
    from learning3d_amd import _lib
    rows, Cin, Cout = 256, 32, 256
    x, w, b = rnd(rows, Cin, seed=145), rnd(Cout, Cin, seed=146), rnd(Cout, seed=147)
    aimg = torch.empty(lib().l3d_f16_image_bytes(2, rows, Cin), dtype=U8, device="cuda")
    _lib.call("l3d_split_f16_operand", x, rows, Cin, Cin, 1, aimg, None)
    wimg = torch.empty(lib().l3d_f16_image_bytes(1, Cout, Cin), dtype=U8, device="cuda")
    _lib.call("l3d_split_f16_operand", w, Cout, Cin, Cin, 0, wimg, None)
    return lambda a: (wimg, aimg, None, b, 0, 1, Cin, rows, Cout, 0, 1 | 4, a.f32(rows, Cout), None, None, None, None, 0, None, 0)


simple("l3d_pointwise_conv_f16", _conv_f16_shift_n, "pointwise_conv_f16_shift_n")


def _fold_mlp(f16):
    def make():
        from learning3d_amd import _lib
        B, N = 2, 130
        g, w5g, s5 = rnd(B, N, 5, seed=150), rnd(512, 5, seed=151), rnd(B, 512, seed=152)
        w6 = rnd(512, 512, seed=153, scale=0.05)
        if f16:
            img = torch.empty(lib().l3d_f16_image_bytes(2, 512, 512), dtype=U8, device="cuda")
            _lib.call("l3d_conv_f16_split_weights", w6, 512, 512, img)
        else:
            img = torch.empty(lib().l3d_split_bytes(512, 512), dtype=U8, device="cuda")
            _lib.call("l3d_split_rows", w6, 512, 512, img)
        b6, w7, b7, ce = rnd(512, seed=154), rnd(3, 512, seed=155, scale=0.05), rnd(3, seed=156), rnd(B, N, 3, seed=157)
        return lambda a: (g, 5, w5g, s5, img, b6, w7, b7, ce, B, N, a.f32(B, N, 3))
    return make


simple("l3d_fold_mlp", _fold_mlp(False))
simple("l3d_fold_mlp_f16", _fold_mlp(True))


# --- EMD ----------------------------------------------------------------------------------------------------------------------
_EMD = {}


def _emd_case(B, n, m, split):
    """bar: tests/test_gpu_parity.py::test_emd_vs_oracle -- cost within rtol 1e-3 of the oracle's; the header: "The result's bits do
    not depend on" split"""
    from oracle import oracle
    x1, x2 = rnd(B, n, 3, seed=160), rnd(B, m, 3, seed=161)
    nbytes = lib().l3d_emd_workspace_bytes(B, n, m)
    out = check("l3d_emd_forward", lambda a: (x1, x2, B, n, m, a.f32(B, n, m), a.f32(B), a.bytes(nbytes), split))
    key = (B, n, m)
    if key not in _EMD:
        _EMD[key] = (oracle.emd_forward(x1.cpu().numpy(), x2.cpu().numpy())[0], out["match"].clone(), out["cost"].clone(), split)
    want, match0, cost0, split0 = _EMD[key]
    rel = float(np.abs(out["cost"].cpu().numpy() - want).max() / np.abs(want).max())
    print(f"emd_forward B={B} n={n} m={m} split={split}: cost within {rel:g} of the oracle's (bar 1e-3)")
    np.testing.assert_allclose(out["cost"].cpu().numpy(), want, rtol=1e-3)
    assert torch.equal(out["match"], match0) and torch.equal(out["cost"], cost0), f"split {split} and split {split0} give different bits"


for _s in (0, 1, 2, 4):
    CASES[f"emd_forward_split{_s}"] = (("l3d_emd_forward",), (lambda s: lambda: _emd_case(2, 33, 1025, s))(_s))
CASES["emd_forward_n1025_m33"] = (("l3d_emd_forward",), lambda: _emd_case(1, 1025, 33, 0))


def _emd_backward():
    B, n, m = 2, 33, 1025
    x1, x2, match = rnd(B, n, 3, seed=160), rnd(B, m, 3, seed=161), rnd(B, n, m, seed=162).abs_()
    return lambda a: (x1, x2, match, B, n, m, a.f32(B, n, 3), a.f32(B, m, 3))


simple("l3d_emd_backward", _emd_backward)


def _lpfa(with_x):
    def make():
        B, N, Cc, k = 2, 67, 5, 6
        xyz, x, idx = rnd(B, N, 3, seed=163), rnd(B, Cc, N, seed=164), rint(N, B, N, k, seed=165)
        return lambda a: (xyz, x if with_x else None, idx, B, N, Cc if with_x else 0, k, a.f32(B, 9, N, k), a.f32(B, Cc, N, k) if with_x else None)
    return make


simple("l3d_lpfa_group", _lpfa(True))
simple("l3d_lpfa_group", _lpfa(False), "lpfa_group_geo_only")


# --- data feed ----------------------------------------------------------------------------------------------------------------
simple("l3d_uniform_clouds", lambda: lambda a: (12345, 2, 131, -1.0, 1.0, a.f32(2, 131, 3)))
simple("l3d_probe_mfma_sustained", lambda: lambda a: (4, a.f32(131072), a.out(I64, 2)))


def _transforms():
    B, N = 3, 131
    t = rnd(B, N, 3, seed=170)
    e, tr, tw, p7 = rnd(B, 3, seed=171), rnd(B, 3, seed=172), rnd(B, 6, seed=173), rnd(B, 7, seed=174)
    return {"l3d_euler_transform": lambda a: (t, e, tr, B, N, a.f32(B, N, 3), a.f32(B, 4, 4)),
            "l3d_twist_transform": lambda a: (t, tw, B, N, a.f32(B, N, 3), a.f32(B, 4, 4), a.f32(B, 4, 4)),
            "l3d_quat_transform": lambda a: (t, p7, B, N, a.f32(B, N, 3))}


for _n in ("l3d_euler_transform", "l3d_twist_transform", "l3d_quat_transform"):
    simple(_n, (lambda n: lambda: _transforms()[n])(_n))


def _sceneflow(sampled):
    def make():
        F, n1, n2, S, B = 3, 50, 60, 17, 2
        p1, c1, fl = rnd(F, n1, 3, seed=175), rnd(F, n1, 3, seed=176), rnd(F, n1, 3, seed=177)
        p2, c2 = rnd(F, n2, 3, seed=178), rnd(F, n2, 3, seed=179)
        mask = rint(2, F, n1, seed=180, dtype=U8)
        scene = torch.tensor([2, 0], dtype=I64).cuda()
        g = torch.Generator().manual_seed(181)
        s1 = torch.stack([torch.randperm(n1, generator=g)[:S] for _ in range(B)]).to(I32).cuda() if sampled else None
        s2 = torch.stack([torch.randperm(n2, generator=g)[:S] for _ in range(B)]).to(I32).cuda() if sampled else None
        return lambda a: (p1, p2, c1, c2, fl, mask, scene, s1, s2, B, n1, n2, S, a.f32(B, S, 3), a.f32(B, S, 3), a.f32(B, S, 3), a.f32(B, S, 3),
                          a.f32(B, S, 3), a.out(U8, B, S))
    return make


simple("l3d_sceneflow_batch", _sceneflow(True), "sceneflow_batch_sampled")
simple("l3d_sceneflow_batch", _sceneflow(False), "sceneflow_batch_first_rows")


# --- training path ------------------------------------------------------------------------------------------------------------
def _train():
    B, Cc, P, K = 2, 5, 264, 8
    z, dy = randn(B, Cc, P, seed=190), randn(B, Cc, P, seed=191)
    sc, sh = rnd(Cc, seed=192).abs_() + 0.5, rnd(Cc, seed=193)
    mean, rstd = rnd(Cc, seed=194).double(), (rnd(Cc, seed=195).abs_() + 0.5).double()
    gr, m1, m2 = rnd(Cc, seed=196).double(), rnd(Cc, seed=197).double() * 0.1, rnd(Cc, seed=198).double() * 0.1
    dpool, pidx = randn(B, Cc, P // K, seed=199), rint(K, B, Cc, P // K, seed=200, dtype=U8)
    part = randn(3, Cc, 2, seed=201).double()
    x2, g1, i1 = randn(131, 7, seed=202), randn(131, seed=203), rint(7, 131, seed=204, dtype=U8)
    return {
        "channel_stats": ("l3d_channel_stats", lambda a: (z, B, Cc, P, a.out(F64, B, Cc, 2))),
        "bn_act_forward": ("l3d_bn_act_forward", lambda a: (z, sc, sh, B, Cc, P, 1, a.f32(B, Cc, P))),
        "bn_backward_stats": ("l3d_bn_backward_stats", lambda a: (dy, z, sc, sh, mean, rstd, B, Cc, P, 1, a.out(F64, B, Cc, 2), None, None, 0)),
        "bn_backward_stats_pooled": ("l3d_bn_backward_stats", lambda a: (None, z, sc, sh, mean, rstd, B, Cc, P, 1, a.out(F64, B, Cc, 2), dpool, pidx, K)),
        "bn_act_backward": ("l3d_bn_act_backward", lambda a: (dy, z, sc, sh, mean, rstd, gr, m1, m2, B, Cc, P, 1, a.f32(B, Cc, P), None, None, 0)),
        "bn_act_backward_pooled": ("l3d_bn_act_backward", lambda a: (dy, z, sc, sh, mean, rstd, gr, m1, m2, B, Cc, P, 1, a.f32(B, Cc, P), dpool, pidx, K)),
        "sum_clouds_f64": ("l3d_sum_clouds_f64", lambda a: (part, 3, Cc * 2, a.out(F64, Cc, 2))),
        "max_last": ("l3d_max_last", lambda a: (x2, 131, 7, a.f32(131), a.out(U8, 131))),
        "max_last_backward": ("l3d_max_last_backward", lambda a: (g1, i1, 131, 7, a.f32(131, 7))),
    }


for _id in ("channel_stats", "bn_act_forward", "bn_backward_stats", "bn_backward_stats_pooled", "bn_act_backward", "bn_act_backward_pooled",
            "sum_clouds_f64", "max_last", "max_last_backward"):
    CASES[_id] = (("l3d_" + _id.replace("_pooled", ""),), (lambda i: lambda: check(*_train()[i]))(_id))


def _bn_finalize(mode):
    def make():
        B, Cc = 3, 37
        part = torch.stack([randn(B, Cc, seed=210) * 100, randn(B, Cc, seed=211).abs_() * 1000 + 500], dim=2).double().contiguous()
        bias, gamma, beta = rnd(Cc, seed=212), rnd(Cc, seed=213) + 1.5, rnd(Cc, seed=214)
        rm, rv = rnd(Cc, seed=215), rnd(Cc, seed=216).abs_() + 0.5
        outs = lambda a: (a.out(F64, Cc), a.out(F64, Cc), a.out(F64, Cc), a.f32(Cc), a.f32(Cc))
        if mode == 2:
            return lambda a: (part, B, Cc, 300.0, bias, None, None, 1e-5, 2, 0.1, None, None, *outs(a))
        return lambda a: (part, B, Cc, 300.0, bias, gamma, beta, 1e-5, mode, 0.1, a.inout(rm), a.inout(rv), *outs(a))
    return make


for _m in (0, 1, 2):
    simple("l3d_bn_finalize", _bn_finalize(_m), f"bn_finalize_mode{_m}")


def _bn_backward_finalize(batch_stats):
    def make():
        Bl, Ba, Cc = 2, 3, 37
        pl, pa, gr = randn(Bl, Cc, 2, seed=217).double(), randn(Ba, Cc, 2, seed=218).double(), rnd(Cc, seed=219).double()
        return lambda a: (pl, Bl, pa if batch_stats else None, Ba if batch_stats else Bl, Cc, 300.0, int(batch_stats), gr, a.out(F64, Cc),
                          a.out(F64, Cc), a.f32(Cc), a.f32(Cc), a.f32(Cc))
    return make


simple("l3d_bn_backward_finalize", _bn_backward_finalize(True))
simple("l3d_bn_backward_finalize", _bn_backward_finalize(False), "bn_backward_finalize_no_batch_stats")


def _layernorm_backward_case(rows, Cc):
    """bar: tests/test_gpu_grad_routes.py::test_layernorm_hip_forward_backward_vs_fp64 -- dx, da, db within 1e-5 of their scale of the
    reference's op sequence differentiated in fp64"""
    x, sa, g = randn(rows, Cc, seed=220, scale=2.0) + 0.7, randn(Cc, seed=221, scale=0.5) + 1.0, randn(rows, Cc, seed=222)
    n = lib().l3d_layernorm_backward_workspace_floats(rows, Cc)
    out = check("l3d_layernorm_ref_backward", lambda a: (x, sa, g, 1e-6, rows, Cc, a.f32(rows, Cc), a.f32(n), a.f32(Cc), a.f32(Cc)))
    x64, a64, b64 = x.double().requires_grad_(), sa.double().requires_grad_(), torch.zeros(Cc, dtype=F64, device="cuda", requires_grad=True)
    y = a64 * (x64 - x64.mean(-1, keepdim=True)) / (x64.std(-1, keepdim=True) + 1e-6) + b64
    (y * g.double()).sum().backward()
    for name, want in (("dx", x64.grad), ("da", a64.grad), ("db", b64.grad)):
        err = float((out[name].double() - want).abs().max()) / float(want.abs().max())
        print(f"layernorm_ref_backward rows={rows} C={Cc}: {name} within {err:g} of its scale (bar 1e-5)")
        assert err <= 1e-5


CASES["layernorm_ref_backward_rows17"] = (("l3d_layernorm_ref_backward",), lambda: _layernorm_backward_case(17, 64))
CASES["layernorm_ref_backward_rows1000"] = (("l3d_layernorm_ref_backward",), lambda: _layernorm_backward_case(1000, 12))


def _sa_fused():
    B, N, S, K, D = 2, 100, 65, 8, 3
    xyz, new, feat = rnd(B, N, 3, seed=230), rnd(B, S, 3, seed=231), rnd(B, D, N, seed=232)
    idx = rint(N, B, S, K, seed=233, dtype=I32)
    # layer 1: 8 padded inputs (run 2: 16 zero rows per run), layers 2 and 3: run 4; each followed by scale and shift
    params = rnd(4 * (32 + 16) * 2 + 64 + 32 * 32 + 64 + 32 * 64 + 128, seed=234, scale=0.3)
    return lambda a: (xyz, new, feat, idx, params, B, N, S, K, D, 32, 32, 64, a.f32(B, 64, S))


simple("l3d_sa_mlp3_fused", _sa_fused)


def _strides(t):
    return (C.c_long * 4)(*t.stride())


def _bmm_case(flags, parts):
    nb1, nb2, M, N, K = 2, 1, 130, 70, 19
    A, Bm = rnd(nb1, nb2, M, K, seed=240), rnd(nb1, nb2, K, N, seed=241)
    bias, c0 = rnd(N, seed=242), rnd(nb1, nb2, M, N, seed=243)

    def build(a):
        c = a.inout(c0) if flags & 1 else a.f32(nb1, nb2, M, N)
        ws = a.f32(nb1 * nb2 * parts * M * N) if parts > 1 else None
        return (A, _strides(A), Bm, _strides(Bm), c, _strides(c), nb1, nb2, M, N, K, 0.5, flags, bias if flags & 4 else None, parts, ws)
    got = check("l3d_bmm_f32", build)["C"]
    want = 0.5 * (A.double() @ Bm.double()) + (bias.double() if flags & 4 else 0)
    if flags & 2:
        want = want.clamp_min(0)
    if flags & 1:
        want = want + c0.double()
    assert float((got.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


CASES["bmm_f32_plain"] = (("l3d_bmm_f32",), lambda: _bmm_case(0, 1))
CASES["bmm_f32_bias_relu"] = (("l3d_bmm_f32",), lambda: _bmm_case(2 | 4, 1))
CASES["bmm_f32_accumulate"] = (("l3d_bmm_f32",), lambda: _bmm_case(1, 1))
CASES["bmm_f32_parts3"] = (("l3d_bmm_f32",), lambda: _bmm_case(0, 3))
simple("l3d_softmax_rows", lambda: (lambda x: lambda a: (x, None, 67, 131, 0.5, a.f32(67, 131)))(rnd(67, 131, seed=244, scale=4.0)), "softmax_rows_forward")
simple("l3d_softmax_rows", lambda: (lambda p, dp: lambda a: (p, dp, 67, 131, 0.5, a.f32(67, 131)))(torch.softmax(rnd(67, 131, seed=245), 1).contiguous(),
                                                                                                   rnd(67, 131, seed=246)), "softmax_rows_backward")


def _colsum_case(R, Cn):
    """bar: tests/test_gpu_grad_routes.py::test_colsum_rows_vs_fp64_and_repeatable -- |got - fp64| <= sum|x| R 2^-24 per column"""
    wide = randn(R, Cn + 7, seed=247)
    v = wide[:, 3:3 + Cn]
    n = lib().l3d_colsum_rows_workspace_bytes(R, Cn)
    got = check("l3d_colsum_rows", lambda a: (v, R, Cn, Cn + 7, a.bytes(n), a.f32(Cn)))["out"]
    want = v.double().sum(0)
    bound = v.double().abs().sum(0) * (R * 2.0 ** -24) + 1e-30
    ratio = float(((got.double() - want).abs() / bound).max())
    print(f"colsum_rows rows={R} cols={Cn}: worst error {ratio:.3g} of the fp32 summation bound (bar 1)")
    assert ratio <= 1.0


for _R, _Cn in ((129, 257), (128, 5), (1, 1), (300, 256)):
    CASES[f"colsum_rows_{_R}x{_Cn}"] = (("l3d_colsum_rows",), (lambda R, Cn: lambda: _colsum_case(R, Cn))(_R, _Cn))


def _wgrad_case(B, Cout, Cin, P, pc):
    """bar: tests/test_gpu_grad_routes.py::test_wgrad_kernel_vs_fp64_and_deterministic -- 2e-6 of max |dW|"""
    dz, x = randn(B, Cout, P, seed=248), randn(B, Cin, P, seed=249) + 0.5
    n = lib().l3d_wgrad_workspace_bytes(B, Cout, Cin, P, pc)
    assert n % 4 == 0
    got = check("l3d_wgrad", lambda a: (dz, x, B, Cout, Cin, P, pc, a.f32(n // 4), a.f32(Cout, Cin)))["dw"]
    want = torch.einsum("bop,bip->oi", dz.double(), x.double())
    rel = float((got.double() - want).abs().max() / want.abs().max())
    print(f"wgrad B={B} Cout={Cout} Cin={Cin} P={P} pc={pc}: {rel:g} of max |dW| (bar 2e-6)")
    assert rel <= 2e-6


CASES["wgrad_ragged_chunk"] = (("l3d_wgrad",), lambda: _wgrad_case(2, 65, 37, 300, 256))
CASES["wgrad_default_chunk"] = (("l3d_wgrad",), lambda: _wgrad_case(3, 3, 70, 2049, 0))
CASES["wgrad_one_chunk"] = (("l3d_wgrad",), lambda: _wgrad_case(1, 64, 64, 31, 256))


# --- per-model headers --------------------------------------------------------------------------------------------------------
simple("l3d_curve_prepare", lambda: (lambda x, w: lambda a: (x, w, 2, 16, 65, a.f32(2, 65, 16), a.f32(2, 65)))(rnd(2, 16, 65, seed=250), rnd(16, seed=251)))


def _curve_walk():
    B, N, Cc, k, cn, cl = 2, 67, 16, 8, 9, 5
    x, adj, start = rnd(B, N, Cc, seed=252), rint(N, B, N, k, seed=253), rint(N, B, cn, seed=254)
    wa, wm = rnd(2 * Cc, seed=255), rnd(2, 2 * Cc, seed=256)
    one, zero, one2, zero2 = torch.ones(1).cuda(), torch.zeros(1).cuda(), torch.ones(2).cuda(), torch.zeros(2).cuda()
    return lambda a: (x, adj, start, B, N, Cc, k, cn, cl, wa, one, zero, wm, one2, zero2, a.f32(B, Cc, cn, cl), a.out(I32, B, cn, cl))


simple("l3d_curve_walk", _curve_walk)


def _mask_tail(N):
    def make():
        B, Cc, H = 2, 16, 32
        x, w4, b4, w5, b5 = rnd(B, Cc, N, seed=257), rnd(H, Cc, seed=258), rnd(H, seed=259), rnd(H, seed=260), rnd(1, seed=261)
        return lambda a: (x, w4, b4, w5, b5, B, Cc, H, N, a.f32(B, N))
    return make


simple("l3d_mask_tail", _mask_tail(257), "mask_tail_scalar_route")
simple("l3d_mask_tail", _mask_tail(260), "mask_tail_vector_route")


def _mask_select(k):
    def make():
        B, N = (2, 131) if k else (1, 131)
        m, p = rnd(B, N, seed=262), rnd(B, N, 3, seed=263)
        S = k if k else N
        return lambda a: (m, p, B, N, k, 0.1, a.out(I64, B, S), a.f32(B, S, 3), a.out(I32, B))
    return make


simple("l3d_mask_select", _mask_select(17), "mask_select_topk")
simple("l3d_mask_select", _mask_select(0), "mask_select_threshold")
simple("l3d_mish", lambda: (lambda x: lambda a: (x, 1027, a.f32(1027)))(rnd(1027, seed=264, scale=30.0)))
simple("l3d_self_attention_shared", lambda: (lambda q, b: lambda a: (q, b, 2, 32, 129, a.f32(2, 32, 129)))(rnd(2, 32, 129, seed=265), torch.full((1,), 0.3).cuda()))
simple("l3d_outer_softmax_mix", lambda: (lambda x, y, b: lambda a: (x, y, b, 3, 65, a.f32(3, 65), a.f32(3, 65)))(rnd(3, 65, seed=266), rnd(3, 65, seed=267),
                                                                                                                 torch.full((1,), 0.3).cuda()))


def _reg_pose(with_T, which):
    def make():
        B, Tn, N, C1 = 2, 3 if with_T else 6, 131, 16
        cloud = rnd(B, N, 3, seed=270)
        T = torch.eye(4).repeat(B, Tn, 1, 1).cuda() + rnd(B, Tn, 4, 4, seed=271, scale=0.1) if with_T else None
        dt = None if with_T else torch.full((6,), 0.01).cuda()
        w1, sc, sh = rnd(C1, 3, seed=272), rnd(C1, seed=273).abs_() + 0.5, rnd(C1, seed=274)
        return lambda a: (cloud, T, dt, B, Tn, N, w1, sc, sh, C1, 1, a.f32(B * Tn, C1, N) if "y" in which else None,
                          a.f32(B * Tn, N, 3) if "posed" in which else None)
    return make


simple("l3d_reg_pose_first_layer", _reg_pose(True, "y_posed"), "reg_pose_first_layer_T")
simple("l3d_reg_pose_first_layer", _reg_pose(False, "y"), "reg_pose_first_layer_dt")
simple("l3d_reg_pose_first_layer", _reg_pose(True, "posed"), "reg_pose_first_layer_posed_only")


def _reg_jac_pinv():
    B, K = 3, 67
    f0, f, dt = rnd(B, K, seed=275), rnd(B, 6, K, seed=276), torch.full((6,), 0.01).cuda()
    return lambda a: (f0, f, dt, B, K, a.f32(B, 6, K), a.inout(torch.zeros(1 + B, dtype=I32, device="cuda")))


simple("l3d_reg_jac_pinv", _reg_jac_pinv)


def _reg_iclk(step):
    def make():
        B, K, maxiter = 3, 67, 4
        f, f0, pinv = rnd(B, K, seed=277), rnd(B, K, seed=278), rnd(B, 6, K, seed=279, scale=0.01)
        singular = torch.zeros(1 + B, dtype=I32, device="cuda")
        state = torch.tensor([0, step, 0, 0], dtype=I32).cuda()
        est = (torch.eye(4).repeat(B, 1, 1) + (0.01 * step)).cuda()
        series = rnd(maxiter + 1, B, 4, 4, seed=280)
        r0 = rnd(B, K, seed=281)
        return lambda a: (f, f0, pinv, B, K, step, maxiter, 1e-7, singular, a.f32(B, 8), a.inout(state), a.inout(est), a.inout(series), a.inout(r0))
    return make


simple("l3d_reg_iclk_step", _reg_iclk(0), "reg_iclk_step_0")
simple("l3d_reg_iclk_step", _reg_iclk(1), "reg_iclk_step_1")


def _reg_quat(first):
    def make():
        B = 5
        p7, R, t = rnd(B, 7, seed=282), torch.eye(3).repeat(B, 1, 1).cuda(), rnd(B, 3, seed=283)
        if first:
            return lambda a: (p7, B, 1, a.f32(B, 3, 3), a.f32(B, 3), a.f32(B, 4, 4))
        return lambda a: (p7, B, 0, a.inout(R), a.inout(t), a.f32(B, 4, 4))
    return make


CASES["reg_quat_update_first"] = (("l3d_reg_quat_update",), lambda: check("l3d_reg_quat_update", _reg_quat(True)(), contract={}))
simple("l3d_reg_quat_update", _reg_quat(False), "reg_quat_update_next")


def _rri(channel_first):
    def make():
        B, N, k = 2, 67, 5
        xyz, idx = rnd(B, N, 3, seed=284), rint(N, B, N, k, seed=285)
        return lambda a: (xyz, idx, B, N, k, int(channel_first), a.f32(B, 4 * k, N) if channel_first else a.f32(B, N, 4 * k))
    return make


simple("l3d_rri_features", _rri(False))
simple("l3d_rri_features", _rri(True), "rri_features_channel_first")


def _gmm_params(J, N, with_gamma):
    def make():
        B = 2
        lg, pts = randn(B, J, N, seed=286), rnd(B, N, 3, seed=287)
        return lambda a: (lg, pts, B, J, N, a.f32(B, N, J) if with_gamma else None, a.f32(B, J), a.f32(B, J, 3), a.f32(B, J))
    return make


simple("l3d_gmm_params", _gmm_params(16, 257, True), "gmm_params_gamma")
simple("l3d_gmm_params", _gmm_params(33, 129, False), "gmm_params_no_gamma")
simple("l3d_gmm_register", lambda: (lambda pi, ms, mt, vt: lambda a: (pi, ms, mt, vt, 3, 16, a.f32(3, 4, 4)))(
    torch.softmax(rnd(3, 16, seed=288), 1).contiguous(), rnd(3, 16, 3, seed=289), rnd(3, 16, 3, seed=290), rnd(3, 16, seed=291).abs_() + 0.1))


# ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ident", sorted(CASES))
def test_entry_point_keeps_its_memory_contract(ident):
    CASES[ident][1]()


# every entry point without an l3d_stream_t parameter launches nothing: host functions
EXEMPT = {
    "l3d_version": "returns a constant", "l3d_status_string": "returns a host string", "l3d_last_hip_error": "reads a host thread-local",
    "l3d_edgeconv_packed_v2_flag_index": "returns a constant",
    "l3d_bmm_f32_route": "host arithmetic on l3d_bmm_f32's pointers, strides and sizes: which kernel that call would run",
    **{n: "a size function: host arithmetic" for n in (
        "l3d_scatter_add_det_workspace_bytes", "l3d_knn_feature_workspace_bytes", "l3d_chamfer_loss_local_ws_bytes",
        "l3d_chamfer_forward_loss_ws_bytes", "l3d_soft_correspondence_workspace_floats", "l3d_emd_workspace_bytes",
        "l3d_layernorm_backward_workspace_floats", "l3d_colsum_rows_workspace_bytes", "l3d_wgrad_workspace_bytes", "l3d_split_bytes",
        "l3d_f16_image_bytes", "l3d_edgeconv_packed_floats")},
}


def test_every_entry_point_has_a_case_or_is_exempt():
    protos = mc.prototypes()
    covered = {e for entries, _ in (*CASES.values(), *HOST_CASES.values()) for e in entries}
    assert covered <= set(protos), sorted(covered - set(protos))
    for name in EXEMPT:
        assert name in protos and not mc.has_stream(protos[name]), f"{name} is exempt but takes a stream: it launches"
        assert name not in covered, f"{name} is exempt and has a case"
    missing = sorted(set(protos) - covered - set(EXEMPT))
    assert not missing, f"entry points without a memory-contract case: {missing}"
    # every entry of the contract table names a writable parameter of a real prototype
    for name, params in mc.CONTRACT.items():
        by_name = {p.name: p for p in protos[name].params}
        for pname, spec in params.items():
            assert pname in by_name and mc.is_writable(by_name[pname]), (name, pname)
            assert spec.kind in ("written", "inout", "scratch") and spec.quote, (name, pname)


# ------------------------------------------------------------------------------------------------------------------------------
# the harness on the CPU: a fake entry point in torch that breaks one rule at a time
Param = namedtuple("Param", "ctype name element indirection")
Proto = namedtuple("Proto", "restype params")
FAKE = Proto(None, (Param("const float *", "x", "float", 1), Param("int", "n", "int", 0), Param("float *", "workspace", "float", 1),
                    Param("float *", "y", "float", 1), Param("l3d_stream_t", "stream", "l3d_stream_t", 0)))
FAKE_CONTRACT = {"l3d_fake": {"workspace": Spec("scratch", "workspace: l3d_fake_workspace_floats(n) floats", ("l3d_fake_workspace_floats", lambda v: (v["n"],), 4))}}


def _fake_size(fn, n):
    assert fn == "l3d_fake_workspace_floats"
    return n


def _past_the_end(t, k):
    """element k past the end of t, through the raw pointer as a kernel would reach it"""
    return torch.empty(0, dtype=t.dtype).set_(t.untyped_storage(), t.storage_offset() + t.numel() + k, (1,), (1,))


def _fake(rule):
    """y = 2 x through the workspace; `rule` names the one mistake it makes"""
    def launch(name, x, n, ws, y):
        if rule == "reads its workspace before writing it":
            y.copy_(2 * x + 0 * torch.nan_to_num(ws) + torch.where(ws == 0, 1.0, 0.0))
            return
        if rule == "needs one more workspace byte than the size function says":
            _past_the_end(ws, 0).view(torch.uint8)[:1] = 7
        ws.copy_(2 * x)
        if rule == "adds into its output without setting it":
            y.add_(ws)
        elif rule == "skips the last element":
            y[:-1] = ws[:-1]
        else:
            y.copy_(ws)
        if rule == "writes one element into a guard":
            _past_the_end(y, 0)[0] = 1.0
        if rule == "flips a const input":
            x[3] = -x[3]
    return launch


def _check_fake(rule):
    x = torch.arange(1.0, 38.0)
    return check("l3d_fake", lambda a: (x.clone() if rule == "flips a const input" else x, 37, a.f32(37), a.f32(37)), launch=_fake(rule),
                 contract=FAKE_CONTRACT, proto=FAKE, sizefn=_fake_size, device="cpu")


def test_harness_passes_a_correct_launch():
    out = _check_fake(None)
    assert torch.equal(out["y"], 2 * torch.arange(1.0, 38.0))


@pytest.mark.parametrize("rule, parameter", [
    ("skips the last element", "`y`"), ("writes one element into a guard", "`y`"), ("adds into its output without setting it", "`y`"),
    ("reads its workspace before writing it", "`y`"), ("flips a const input", "`x`"),
    ("needs one more workspace byte than the size function says", "`workspace`")])
def test_harness_names_the_parameter_of_each_violation(rule, parameter):
    with pytest.raises(ContractError) as e:
        _check_fake(rule)
    assert "l3d_fake" in str(e.value) and parameter in str(e.value) and "offset" in str(e.value), str(e.value)


def test_harness_refuses_a_case_that_sizes_a_workspace_by_hand():
    x = torch.arange(1.0, 38.0)
    with pytest.raises(AssertionError, match="size function says"):
        check("l3d_fake", lambda a: (x, 37, a.f32(64), a.f32(37)), launch=_fake(None), contract=FAKE_CONTRACT, proto=FAKE, sizefn=_fake_size,
              device="cpu")


def test_harness_rearmed_workspace_runs_a_third_time():
    """a workspace with state ("the first 8 bytes zero before the first call, the kernel re-arms them"): a fake that forgets to re-arm
    passes the two fills and fails on the workspace it left"""
    proto = Proto(None, (Param("const float *", "x", "float", 1), Param("void *", "ws", "void", 1), Param("float *", "y", "float", 1),
                         Param("l3d_stream_t", "stream", "l3d_stream_t", 0)))
    contract = {"l3d_fake": {"ws": Spec("scratch", "the first 8 bytes zero before the first call (the kernel re-arms them)", keep=8)}}
    x = torch.arange(1.0, 6.0)

    def launch(rearm):
        def run(name, x, ws, y):
            ticket = ws[:8].view(torch.int64)
            y.copy_(x + ticket.float())
            ticket += 1
            if rearm:
                ticket.zero_()
        return run
    build = lambda a: (x, a.bytes(64, zero_first=8, key="ws"), a.f32(5))
    check("l3d_fake", build, launch=launch(True), contract=contract, proto=proto, device="cpu")
    with pytest.raises(ContractError, match="`y`.*second call"):
        check("l3d_fake", build, launch=launch(False), contract=contract, proto=proto, device="cpu")


# ------------------------------------------------------------------------------------------------------------------------------
# the same table under the public ops: every case of the two view tables, contiguous inputs, once per fill
def _under_fill(monkeypatch, fn, args, fill):
    from learning3d_amd import _lib
    log = []
    with monkeypatch.context() as m:
        layout_audit.install(m, inner=mc.filling_call(_lib.call, fill, log))
        out = fn(*args)
        torch.cuda.synchronize()
    return out, log


sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_views_models as view_models                                             # noqa: E402
import test_gpu_views_ops as view_ops                                                   # noqa: E402


@gpu
@pytest.mark.parametrize("name", sorted(view_ops.CASES))
def test_public_op_does_not_depend_on_what_its_outputs_held(name, monkeypatch):
    ops = view_ops
    spec = ops.CASES[name]()
    fn, args = spec[0], spec[1]
    fn(*args)                                           # (the first call fills the caches of weight images)
    out_a, log_a = _under_fill(monkeypatch, fn, args, mc.FILL_A)
    out_b, log_b = _under_fill(monkeypatch, fn, args, mc.FILL_B)
    assert log_a == log_b
    assert log_a or not spec[2], f"{name}: no writable tensor reached a launch"
    (ops.images_identical if name in ops.IMAGES else assert_identical)(out_a, out_b, f"{name}: outputs pre-filled with 0xFF against 0x00")


@gpu
@pytest.mark.parametrize("name", sorted(view_models.MODELS))
def test_model_does_not_depend_on_what_its_outputs_held(name, monkeypatch):
    net, call, count, n, shape, *batch = view_models.MODELS[name]()
    base = view_models.clouds(n, sum(map(ord, name)), count, *batch)
    args = [b if shape == "bnc" else b.transpose(1, 2).contiguous() for b in base]
    with torch.no_grad():
        call(net, *args)                                # (the first call fills the caches of weight images)
        out_a, log_a = _under_fill(monkeypatch, lambda *xs: call(net, *xs), args, mc.FILL_A)
        out_b, log_b = _under_fill(monkeypatch, lambda *xs: call(net, *xs), args, mc.FILL_B)
    assert log_a and log_a == log_b
    assert_identical(out_a, out_b, f"{name}: outputs pre-filled with 0xFF against 0x00", strides=False)
