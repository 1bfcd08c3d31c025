"""Partial / noisy registration pairs without a device: the new header in the open table, the surface of data_utils.partial, the
kept-count formula and the fp64 numpy model of the selection against the fixture (tests/golden/partial_seeded.npz, made from the
reference by make_golden_partial.py), the host-side status codes of l3d_crop_select and the feed's defaults."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import partial_fixture as pf     # noqa: E402

from learning3d_amd import _lib                     # noqa: E402
from learning3d_amd import data_utils as D          # noqa: E402
from learning3d_amd.data_utils import partial as P  # noqa: E402

NAME = "l3d_crop_select"


def test_header_parses_into_the_open_table():
    assert NAME in _lib.EXT_SIGNATURES and NAME in _lib.EXT_PROTOTYPES
    assert NAME not in _lib.SIGNATURES and NAME not in _lib.MODEL_SIGNATURES
    assert not set(_lib.EXT_CONSTANTS) & (set(_lib.CONSTANTS) | set(_lib.MODEL_CONSTANTS))
    assert (_lib.L3D_CROP_NEAREST, _lib.L3D_CROP_PLANE, _lib.L3D_CROP_MAX_N) == (pf.NEAREST, pf.PLANE, 8192)
    proto = _lib.EXT_PROTOTYPES[NAME]
    assert [p.name for p in proto.params] == ["points", "vec", "centre", "B", "N", "C", "mode", "K", "noise", "sigma", "clip", "idx", "mask",
                                              "out", "stream"]
    assert [p.element for p in proto.params] == ["float", "double", "float", "int", "int", "int", "int", "int", "float", "float", "float",
                                                 "int64_t", "float", "float", "l3d_stream_t"]
    const = [p.name for p in proto.params if p.ctype.startswith("const")]
    assert const == ["points", "vec", "centre", "noise", "sigma"] and proto.params[10].indirection == 0 and proto.restype is ctypes.c_int


def test_exports_and_signatures():
    for name in ("RegistrationData", "crop_select", "farthest_subsample_points", "jitter_pointcloud", "planar_crop", "plane_keep_count",
                 "uniform_2_sphere"):
        assert getattr(D, name) is getattr(P, name), name

    def defaults(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items() if v.kind is not v.KEYWORD_ONLY]
    empty = inspect.Parameter.empty
    assert defaults(P.farthest_subsample_points) == [("pointcloud", empty), ("num_subsampled_points", 768), ("view", None)]
    assert defaults(P.planar_crop) == [("points", empty), ("p_keep", 0.7), ("normal", None)]
    assert defaults(P.jitter_pointcloud) == [("pointcloud", empty), ("sigma", 0.04), ("clip", 0.05), ("noise", None)]
    assert defaults(P.uniform_2_sphere)[0] == ("num", None)
    assert defaults(P.RegistrationData.__init__)[1:] == [("algorithm", empty), ("data_class", empty), ("partial_source", False),
                                                          ("partial_template", False), ("noise", False), ("additional_params", {})]
    assert P.ALGORITHMS == ('PCRNet', 'PointNetLK', 'DCP', 'PRNet', 'iPCRNet', 'RPMNet', 'DeepGMR')
    with pytest.raises(Exception, match="not available"):
        P.transform_for("ICP")
    from learning3d_amd.ops import transform_functions as T
    kinds = {a: type(P.transform_for(a, 4)) for a in P.ALGORITHMS}
    assert kinds == {'PCRNet': T.PCRNetTransform, 'iPCRNet': T.PCRNetTransform, 'PointNetLK': T.PNLKTransform, 'RPMNet': T.RPMNetTransform,
                     'DCP': T.DCPTransform, 'PRNet': T.DCPTransform, 'DeepGMR': T.DeepGMRTransform}
    gmr, pnlk = P.transform_for('DeepGMR'), P.transform_for('PointNetLK')
    assert abs(gmr.angle_range - np.pi / 2) < 1e-12 and (pnlk.mag, pnlk.randomly) == (0.8, True)


def test_uniform_2_sphere_on_the_host_draws_in_the_references_order():
    np.random.seed(5)
    v = P.uniform_2_sphere()
    np.random.seed(5)
    phi, cos_theta = np.random.uniform(0.0, 2 * np.pi), np.random.uniform(-1.0, 1.0)
    assert v.shape == (3,) and v[2] == np.cos(np.arccos(cos_theta)) and v[0] == np.sin(np.arccos(cos_theta)) * np.cos(phi)
    many = P.uniform_2_sphere(7)
    assert many.shape == (7, 3) and np.allclose(np.linalg.norm(many, axis=1), 1.0, atol=1e-12)


def test_kept_count_formula_gives_the_references_counts():
    z = pf.load()
    for name, N in pf.PLANAR:
        assert P.plane_keep_count(N) == len(z[f"{name}_idx"]), name
    assert P.plane_keep_count(1024) == len(z["s_planar_idx_source"]) == len(z["s_planar_idx_template"]) == 717
    assert [P.plane_keep_count(n) for n in (7, 11, 101, 768, 1024, 2048)] == [5, 7, 70, 537, 717, 1433]
    g = np.random.default_rng(0)
    for n in (2, 3, 7, 11, 101, 768, 1024, 2048):           # numpy's own percentile on distinct values, q formed as the reference forms it
        d = g.permutation(n).astype(np.float64)
        for p_keep in (0.7, 0.5, 0.25):
            q = (1.0 - np.array(p_keep, dtype=np.float32)) * 100
            assert P.plane_keep_count(n, p_keep) == int((d > np.percentile(d, q)).sum()), (n, p_keep)
    assert P.plane_keep_count(1024, 1.0) == 1023 and P.plane_keep_count(2, 0.5) == 1


@pytest.mark.parametrize("name", [c[0] for c in pf.FARTHEST])
def test_numpy_model_gives_the_references_nearest_list_in_its_order(name):
    z = pf.load()
    N, K, C, sign = next(c[1:] for c in pf.FARTHEST if c[0] == name)
    pts, view, idx = z[f"{name}_points"], z[f"{name}_view"], z[f"{name}_idx"]
    assert pts.shape == (N, C) and idx.shape == (K,) and np.sign(view[0]) == sign and view.dtype == np.float64
    assert np.array_equal(pf.select(pts, view, None, pf.NEAREST, K), idx)
    gaps = np.diff(np.sort(pf.keys(pts, view, None, pf.NEAREST)))
    assert gaps.min() >= pf.NEAREST_GAP                      # the generator's condition on its seed
    # what fp64 keys are for: in fp32 the same clouds tie
    k32 = ((pts[:, :3] - view.astype(np.float32)) ** 2).sum(1, dtype=np.float32)
    assert N < 1024 or len(np.unique(k32)) < N


@pytest.mark.parametrize("name", [c[0] for c in pf.PLANAR])
def test_numpy_model_gives_the_references_planar_list(name):
    z = pf.load()
    pts, normal, centre, idx = z[f"{name}_points"], z[f"{name}_normal"], z[f"{name}_centre"], z[f"{name}_idx"]
    assert centre.dtype == np.float32 and normal.dtype == np.float64 and bool((np.diff(idx) > 0).all())
    assert np.array_equal(pf.select(pts, normal, centre, pf.PLANE, len(idx)), idx)


def test_numpy_model_gives_the_whole_samples():
    z = pf.load()
    for name, mode, vec in (("s_prnet", pf.NEAREST, "view"), ("s_planar", pf.PLANE, "normal")):
        for side, full in (("source", "source_full"), ("template", "template_full")):
            centre = z[f"{name}_centre_{side}"] if mode == pf.PLANE else None
            idx = z[f"{name}_idx_{side}"]
            assert np.array_equal(pf.select(z[f"{name}_{full}"], z[f"{name}_{vec}_{side}"], centre, mode, len(idx)), idx)
        assert np.array_equal(z[f"{name}_template"], z[f"{name}_template_full"][z[f"{name}_idx_template"]])
        assert np.array_equal(z[f"{name}_source"], pf.jitter(z[f"{name}_source_full"][z[f"{name}_idx_source"]], z[f"{name}_noise"], None, 0.05))
    assert np.array_equal(z["j_out"], pf.jitter(z["j_points"], z["j_unit"], np.float32(z["j_sigma"]), 0.05))
    assert np.array_equal(z["j_out"], pf.jitter(z["j_points"], z["j_noise"], None, 0.05))


def test_model_orders_ties_and_nans_by_the_headers_rule():
    pts = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [-0.0, 0, 0], [2, 0, 0]], dtype=np.float32)
    origin = np.zeros(3)
    assert pf.select(pts, origin, None, pf.NEAREST, 6).tolist() == [0, 4, 1, 2, 5, 3]        # -0 == +0 by index, twins by index, NaN last
    assert pf.select(pts, np.array([1.0, 0, 0]), np.zeros(3, np.float32), pf.PLANE, 3).tolist() == [1, 3, 5]   # NaN first, 2, the first twin
    assert pf.select(pts, origin, None, pf.PLANE, 6).tolist() == [0, 1, 2, 3, 4, 5]


def test_statuses_are_decided_on_the_host_before_any_launch():
    """-1 for a null pointer, a non-positive size, K > N, an unknown mode or no output; -2 for N > L3D_CROP_MAX_N, B > 65535, C < 3"""
    fn = getattr(_lib.lib(), NAME)
    one = ctypes.c_void_p(16)                      # never dereferenced: every call below returns before a launch

    def args(**kw):
        a = dict(points=one, vec=one, centre=one, B=1, N=8, C=3, mode=0, K=4, noise=None, sigma=None, clip=0.0, idx=one, mask=one, out=one)
        a.update(kw)
        return [*a.values(), None]
    for bad in (dict(K=9), dict(K=0), dict(B=0), dict(N=0, K=0), dict(C=0), dict(points=None), dict(vec=None), dict(mode=2), dict(mode=-1),
                dict(idx=None, mask=None, out=None), dict(mode=1, centre=None), dict(mode=1, vec=None)):
        assert fn(*args(**bad)) == _lib.L3D_ERR_INVALID_ARG == -1, bad
    for bad in (dict(N=_lib.L3D_CROP_MAX_N + 1), dict(B=65536), dict(C=2), dict(C=1), dict(mode=1, N=_lib.L3D_CROP_MAX_N + 1, K=5)):
        assert fn(*args(**bad)) == _lib.L3D_ERR_UNSUPPORTED == -2, bad


def test_cpu_tensors_raise_at_the_c_abi_wrapper():
    pts, view = torch.rand(1, 8, 3), torch.rand(1, 3, dtype=torch.float64)
    with pytest.raises(_lib.L3DError, match="device tensors only"):
        P.crop_select(pts, view, _lib.L3D_CROP_NEAREST, 4)
    with pytest.raises(_lib.L3DError, match="takes a torch.float64 tensor"):
        _lib.call(NAME, pts, view.float(), None, 1, 8, 3, 0, 4, None, None, 0.0, None, None, torch.empty(1, 4, 3))
    with pytest.raises(ValueError):
        P.farthest_subsample_points(torch.rand(8, 2), 4)


def test_feed_defaults_leave_the_new_options_off():
    sig = inspect.signature(D.ResidentRegistrationFeed.__init__)
    new = ("partial_source", "partial_template", "num_subsampled_points", "partial_method", "noise", "masks")
    assert [sig.parameters[k].default for k in new] == [False, False, 768, "farthest", False, False]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in new)
    old = ["self", "data", "labels", "batch_size", "num_points", "transform", "randomize_points", "seed", "drop_last", "rri_neighbors"]
    assert list(sig.parameters)[:len(old)] == old
    assert isinstance(inspect.getattr_static(D.ResidentRegistrationFeed, "for_algorithm"), classmethod)
