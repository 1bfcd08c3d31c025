"""Every public op whose tensor input reaches a kernel, on non-contiguous views of its inputs, under the launch audit.

`_lib.call` hands `tensor.data_ptr()` to the kernel without a look at the strides: whether the kernel reads the memory the caller
meant is decided by hand at each call site (f32c, f32a, .contiguous(), _as_bn3, an assert, or a stride argument).  One missed copy
gives no error -- finite, plausible, wrong numbers.  Here each tensor input in turn is a transposed view, a channel slice of a
wider buffer, a row slice that is non-dense across the batch, or one cloud expanded over the batch (index inputs: a transposed and
a stride-2 view), and the result must equal, bit for bit and in shape, dtype and strides, the result on the view's contiguous clone;
the two runs must launch the same entry points; the caller's buffer, skipped elements included, must be unchanged.  The audit
(tests/golden/layout_audit.py) refuses a mis-laid tensor before anything is launched, so a layout bug is a test failure and never a
kernel reading outside an allocation.

NONDETERMINISTIC is the list of ops whose two runs on the same contiguous input differ (a floating-point atomic): it is empty."""
import os
import sys

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import layout_audit                                                                     # noqa: E402
from seeded import seeded_params                                                        # noqa: E402
from view_cases import (assert_identical, float_views, has_entry, index_views, logged, run_on_views, same_bits,   # noqa: E402
                        whole_storage)

pytestmark = pytest.mark.gpu

NONDETERMINISTIC = {}        # op -> "file.hip:line" of the floating-point atomic that explains it.  Empty: every op here repeats its bits.

B, N, M, K = 2, 128, 96, 16


@pytest.fixture(autouse=True)
def audit(monkeypatch):
    return layout_audit.install(monkeypatch)


def rnd(*shape, seed=0, scale=1.0):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(1000 + seed)) * 2 - 1).mul_(scale).cuda()


def rint(hi, *shape, seed=0, dtype=torch.int64):
    return torch.randint(0, hi, shape, generator=torch.Generator().manual_seed(2000 + seed)).to(dtype).cuda()


def nograd(fn):
    def run(*args):
        with torch.no_grad():
            return fn(*args)
    return run


def views_of(args, which=None, kinds=None):
    """{i: views} for the tensor arguments `which` (default: all of them): float_views / index_views by dtype"""
    out = {}
    for i, a in enumerate(args):
        if isinstance(a, torch.Tensor) and (which is None or i in which):
            vs = float_views(a) if a.dtype.is_floating_point else index_views(a)
            vs = [(k, v) for k, v in vs if kinds is None or k in kinds]
            if vs:                                  # (a [1, N] tensor has no non-contiguous view of these kinds)
                out[i] = vs
    return out


def images_identical(got, want, what, strides=True):
    """an activation image (l3d_hip.h, l3d_f16_image_bytes kind 1) is "h | m' planes + 16 bytes: 2^-T, scratch": everything up to and
    including 2^-T is the result; the 12 bytes of scratch behind it are whatever the allocation held"""
    assert got.dtype == torch.uint8 and got.dim() == 1 and got.shape == want.shape, what
    assert_identical(got[:-12], want[:-12], what, strides)


IMAGES = {"split_rows_f16", "split_rows_f16_channel_first", "first_layer_f16_planes_channel_last", "first_layer_f16_planes_channel_first"}


# ------------------------------------------------------------------------------------------------------------------------------
# the cases: name -> () -> (fn, args, entries[, which])
def _common():
    from learning3d_amd.utils import model_common_utils as m
    return m


CASES = {}


def case(f):
    CASES[f.__name__] = f
    return f


@case
def knn_c3():
    return nograd(lambda x: _common().knn(x, K)), [rnd(B, 3, N, seed=1)], ["l3d_knn_graph"]


@case
def knn_c64():
    return nograd(lambda x: _common().knn(x, K)), [rnd(B, 64, N, seed=2)], ["l3d_knn_feature"]


@case
def square_distance():
    return nograd(_common().square_distance), [rnd(B, N, 3, seed=3), rnd(B, M, 3, seed=4)], ["l3d_square_distance"]


@case
def index_points_bs():
    return nograd(_common().index_points), [rnd(B, N, 8, seed=5), rint(N, B, 40, seed=5)], ["l3d_index_points"]


@case
def index_points_bsk():
    return nograd(_common().index_points), [rnd(B, N, 8, seed=6), rint(N, B, 24, 6, seed=6)], ["l3d_index_points"]


@case
def farthest_point_sample():
    return (nograd(lambda x: _common().farthest_point_sample(x, 32, start_with_first_point=True)), [rnd(B, N, 3, seed=7)],
            ["l3d_farthest_point_sample"])


@case
def knn_point():
    return nograd(lambda a, b: _common().knn_point(K, a, b)), [rnd(B, N, 3, seed=8), rnd(B, M, 3, seed=9)], ["l3d_knn_point"]


@case
def query_ball_point_cnt():
    return (nograd(lambda a, b: _common().query_ball_point(0.5, K, a, b, get_cnt=True)), [rnd(B, N, 3, seed=10), rnd(B, M, 3, seed=11)],
            ["l3d_query_ball_point"])


@case
def query_ball_point_itself():
    return (nograd(lambda a, b, it: _common().query_ball_point(0.5, K, a, b, itself_indices=it)),
            [rnd(B, N, 3, seed=12), rnd(B, M, 3, seed=13), rint(N, B, M, seed=13)], ["l3d_query_ball_point"])


@case
def get_graph_feature():
    return nograd(lambda x: _common().get_graph_feature(x, k=K)), [rnd(B, 3, N, seed=14)], ["l3d_knn_graph", "l3d_graph_feature"]


@case
def get_graph_feature_c64():
    return nograd(lambda x: _common().get_graph_feature(x, k=K)), [rnd(B, 64, N, seed=15)], ["l3d_knn_feature", "l3d_graph_feature"]


@case
def pointconv_knn_point():
    from learning3d_amd.utils import pointconv_util as p
    return nograd(lambda a, b: p.knn_point(K, a, b)), [rnd(B, N, 3, seed=16), rnd(B, M, 3, seed=17)], ["l3d_knn_point_expanded"]


@case
def pointconv_compute_density():
    from learning3d_amd.utils import pointconv_util as p
    return nograd(lambda a: p.compute_density(a, 0.2)), [rnd(B, N, 3, seed=18)], ["l3d_gaussian_density"]


@case
def lpfa_group():
    from learning3d_amd.utils import curvenet_util as c
    return nograd(c.lpfa_group), [rnd(B, 3, N, seed=19), rnd(B, 16, N, seed=20), rint(N, B, N, K, seed=20)], ["l3d_lpfa_group"]


@case
def curve_prepare():
    from learning3d_amd.utils import curvenet_util as c
    return nograd(c.curve_prepare), [rnd(B, 16, N, seed=21), rnd(16, seed=22)], ["l3d_curve_prepare"]


@case
def curve_walk():
    from learning3d_amd.utils import curvenet_util as c
    C_ = 16
    params = (rnd(2 * C_, seed=23), torch.ones(1).cuda(), torch.zeros(1).cuda(), rnd(2, 2 * C_, seed=24), torch.ones(2).cuda(), torch.zeros(2).cuda())
    return (nograd(lambda xa, adj, start: c.curve_walk(xa, adj, start, params, 5)),
            [rnd(B, N, C_, seed=25), rint(N, B, N, 8, seed=25), rint(N, B, 8, seed=26)], ["l3d_curve_walk"])


@case
def kabsch():
    from learning3d_amd.utils import svd
    return nograd(svd.kabsch), [rnd(B, 3, N, seed=27), rnd(B, 3, N, seed=28)], ["l3d_kabsch"]


@case
def soft_correspondence():
    from learning3d_amd.utils import svd
    return (nograd(svd.soft_correspondence), [rnd(B, 32, N, seed=29), rnd(B, 32, M, seed=30), rnd(B, 3, M, seed=31)],
            ["l3d_soft_correspondence"])


@case
def svd3x3_rotation():
    from learning3d_amd.utils import svd
    return nograd(svd.svd3x3_rotation), [rnd(B, 3, 3, seed=32)], ["l3d_svd3x3_rotation"]


def _svd_head(shape):
    from learning3d_amd.utils.svd import SVDHead
    head = SVDHead(32, input_shape=shape).cuda().eval()
    pts = (B, N, 3) if shape == "bnc" else (B, 3, N)
    return (nograd(head), [rnd(B, 32, N, seed=33), rnd(B, 32, N, seed=34), rnd(*pts, seed=35), rnd(*pts, seed=36)],
            ["l3d_soft_correspondence", "l3d_kabsch"])


@case
def svd_head_bnc():
    return _svd_head("bnc")


@case
def svd_head_bcn():
    return _svd_head("bcn")


@case
def transformer_layer_norm():
    from learning3d_amd.utils.transformer import LayerNorm
    ln = seeded_params(LayerNorm(64), 40).cuda().eval()
    return nograd(ln), [rnd(B, N, 64, seed=37)], ["l3d_layernorm_planes"]


@case
def transformer_layer_norm_planes():
    from learning3d_amd.utils.transformer import LayerNorm
    ln = seeded_params(LayerNorm(64), 41).cuda().eval()
    return nograd(ln), [rnd(B, 256, 64, seed=38)], ["l3d_layernorm_planes"]


def _attention_entry():
    from learning3d_amd.models import _fused
    return "l3d_attention_forward_f16b" if _fused.gemm_arith() == "f16x2" else "l3d_attention_forward_strided"


@case
def multi_headed_self_attention():
    from learning3d_amd.utils.transformer import MultiHeadedAttention
    att = seeded_params(MultiHeadedAttention(4, 256), 42).cuda().eval()
    return nograd(lambda x: att(x, x, x)), [rnd(B, N, 256, seed=39)], [_attention_entry()]


@case
def multi_headed_cross_attention():
    from learning3d_amd.utils.transformer import MultiHeadedAttention
    att = seeded_params(MultiHeadedAttention(4, 256), 43).cuda().eval()
    return nograd(lambda q, kv: att(q, kv, kv)), [rnd(B, N, 256, seed=40), rnd(B, N, 256, seed=41)], [_attention_entry()]


@case
def chamfer_distance_function():
    from learning3d_amd.losses.chamfer_distance import ChamferDistanceFunction
    return nograd(ChamferDistanceFunction.apply), [rnd(B, N, 3, seed=42), rnd(B, M, 3, seed=43)], ["l3d_chamfer_forward"]


def _chamfer_module():
    import importlib
    return importlib.import_module("learning3d_amd.losses.chamfer_distance")        # (the package exports a function of that name)


def _dists(seed):
    return [rnd(B, N, seed=seed).abs_(), rnd(B, M, seed=seed + 1).abs_()]


@case
def chamfer_partials():
    cd = _chamfer_module()
    return nograd(cd.chamfer_partials), _dists(44), ["l3d_chamfer_partials"]


@case
def chamfer_loss_local():
    cd = _chamfer_module()
    return nograd(cd.chamfer_loss_local), _dists(46), ["l3d_chamfer_loss_local_mb"]


@case
def chamfer_forward_loss():
    cd = _chamfer_module()
    return (nograd(lambda a, b: cd.chamfer_forward_loss(a, b, want="all")), [rnd(B, N, 3, seed=48), rnd(B, M, 3, seed=49)],
            ["l3d_chamfer_forward_loss"])


@case
def emd_function():
    from learning3d_amd.losses.emd import EMDFunction
    return nograd(EMDFunction.apply), [rnd(B, N, 3, seed=50), rnd(B, N, 3, seed=51)], ["l3d_emd_forward"]


@case
def euler_transform():
    from learning3d_amd.ops import transform_functions as t
    return nograd(t.euler_transform), [rnd(B, N, 3, seed=52), rnd(B, 3, seed=53), rnd(B, 3, seed=54)], ["l3d_euler_transform"]


@case
def twist_transform():
    from learning3d_amd.ops import transform_functions as t
    return nograd(t.twist_transform), [rnd(B, N, 3, seed=55), rnd(B, 6, seed=56)], ["l3d_twist_transform"]


@case
def quat_transform():
    from learning3d_amd.ops import transform_functions as t
    return nograd(t.quat_transform), [rnd(B, N, 3, seed=57), rnd(B, 7, seed=58)], ["l3d_quat_transform"]


@case
def se3_exp_map():
    from learning3d_amd.ops import se3
    return nograd(se3.ExpMap.apply), [rnd(B, 6, seed=59)], []                   # torch ops only: nothing to launch, on either side


def _pointwise_conv(cin, cout, channel_last, entry, seed):
    from learning3d_amd.models import _fused
    x = rnd(B, N, cin, seed=seed) if channel_last else rnd(B, cin, N, seed=seed)
    return (nograd(lambda x, w, scale, shift: _fused.pointwise_conv(x, w, scale, shift, relu=True, channel_last=channel_last)),
            [x, rnd(cout, cin, seed=seed + 1, scale=0.2), rnd(cout, seed=seed + 2).abs_().add_(0.5), rnd(B, cout, seed=seed + 3)], [entry])


@case
def pointwise_conv_channel_first():
    return _pointwise_conv(16, 32, False, "l3d_pointwise_conv", 60)


@case
def pointwise_conv_channel_last():
    return _pointwise_conv(16, 32, True, "l3d_pointwise_conv", 64)


@case
def pointwise_conv_split_channel_first():
    return _pointwise_conv(32, 256, False, "l3d_pointwise_conv_split", 68)


@case
def pointwise_conv_split_channel_last():
    return _pointwise_conv(32, 256, True, "l3d_pointwise_conv_split", 72)


@case
def pointwise_conv_maxpool():
    from learning3d_amd.models import _fused
    return (nograd(lambda x, w, scale, shift: _fused.pointwise_conv_maxpool(x, w, scale, shift, True, 8)),
            [rnd(B, 16, N, seed=76), rnd(32, 16, seed=77, scale=0.2), rnd(32, seed=78).abs_().add_(0.5), rnd(B, 32, seed=79)],
            ["l3d_pointwise_conv"])


def _linear_rows(cin, entry, seed):
    from learning3d_amd.models import _fused
    lin = seeded_params(nn.Linear(cin, 64), seed).cuda().eval()
    return nograd(lambda x: _fused.linear_rows(x, lin, relu=True)), [rnd(4, cin, seed=seed)], [entry]


@case
def linear_rows_256():
    return _linear_rows(256, "l3d_linear_rows", 80)


@case
def linear_rows_64():
    return _linear_rows(64, "l3d_pointwise_conv", 81)


@case
def split_rows_f16():
    from learning3d_amd.models import _fused
    return nograd(_fused.split_rows_f16), [rnd(B, N, 64, seed=82)], ["l3d_split_f16_rows"]


@case
def split_rows_f16_channel_first():
    from learning3d_amd.models import _fused
    return nograd(lambda x: _fused.split_rows_f16(x, channel_first=True)), [rnd(B, 64, N, seed=83)], ["l3d_split_f16_rows"]


def _first_layer(channel_last, seed):
    from learning3d_amd.models import _fused
    x = rnd(B, 256, 3, seed=seed) if channel_last else rnd(B, 3, 256, seed=seed)
    return (nograd(lambda x, w, shift: _fused.first_layer_f16_planes(x, w, shift, True, channel_last)),
            [x, rnd(128, 3, seed=seed + 1), rnd(128, seed=seed + 2)], ["l3d_first_layer_f16_planes"])


@case
def first_layer_f16_planes_channel_last():
    return _first_layer(True, 84)


@case
def first_layer_f16_planes_channel_first():
    return _first_layer(False, 87)


@case
def mask_select_topk():
    from learning3d_amd.models.masknet import mask_select
    return nograd(lambda m, p: mask_select(m, p, k=32)), [rnd(B, N, seed=90), rnd(B, N, 3, seed=91)], ["l3d_mask_select"]


@case
def mask_select_threshold():
    from learning3d_amd.models.masknet import mask_select
    return nograd(lambda m, p: mask_select(m, p, k=0, threshold=0.1)), [rnd(1, N, seed=92), rnd(1, N, 3, seed=93)], ["l3d_mask_select"]


@case
def train_layer_norm_ref():
    from learning3d_amd.models import _train
    return (nograd(lambda x, a, b: _train.layer_norm_ref(x, a, b, 1e-6)), [rnd(B, N, 64, seed=94), rnd(64, seed=95), rnd(64, seed=96)],
            ["l3d_layernorm_planes"])


def _conv_bn_act(train, seed):
    from learning3d_amd.models import _train
    conv = seeded_params(nn.Conv1d(16, 32, 1), seed).cuda()
    bn = seeded_params(nn.BatchNorm1d(32), seed + 1).cuda().train(train)
    return (nograd(lambda x: _train.conv_bn_act(x, conv, bn, relu=True)), [rnd(B, 16, N, seed=seed)],
            ["l3d_pointwise_conv", "l3d_bn_finalize", "l3d_bn_act_forward"] + (["l3d_channel_stats"] if train else []))


@case
def train_conv_bn_act_eval():
    return _conv_bn_act(False, 97)


@case
def train_conv_bn_act_batch_statistics():
    return _conv_bn_act(True, 99)      # (the running statistics move with every call; the output is normalised by the batch's own)


@case
def train_conv_act_no_bn():
    from learning3d_amd.models import _train
    conv = seeded_params(nn.Conv2d(16, 32, 1), 101).cuda()
    return nograd(lambda x: _train.conv_bn_act(x, conv, None, relu=True)), [rnd(B, 16, 32, 4, seed=101)], ["l3d_pointwise_conv"]


@case
def rows_linear():
    from learning3d_amd.models import _rows
    lin = seeded_params(nn.Linear(32, 48), 102).cuda()
    return nograd(lambda x: _rows.linear(x, lin, relu=True)), [rnd(B, N, 32, seed=102)], ["l3d_bmm_f32"]


@case
def rows_softmax_rows():
    from learning3d_amd.models import _rows
    return nograd(lambda x: _rows.softmax_rows(x, 0.5)), [rnd(B, N, M, seed=103, scale=4.0)], ["l3d_softmax_rows"]


@case
def rows_square_distance():
    from learning3d_amd.models import _rows
    return nograd(_rows.square_distance), [rnd(B, N, 3, seed=104), rnd(B, M, 3, seed=105)], ["l3d_square_distance"]


@case
def rows_index_points():
    from learning3d_amd.models import _rows
    return nograd(_rows.index_points), [rnd(B, N, 8, seed=106), rint(N, B, 24, 6, seed=106)], ["l3d_index_points"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_op_on_views_equals_op_on_contiguous_clone(name, audit):
    spec = CASES[name]()
    fn, args, entries = spec[:3]
    run_on_views(fn, args, views_of(args, spec[3] if len(spec) > 3 else None), entries, name, nondeterministic=name in NONDETERMINISTIC,
                 compare=images_identical if name in IMAGES else assert_identical)
    assert audit.checked > 0 or not entries


def test_three_clouds_batch_stride():
    """a third cloud: `wide[:, 1:1 + n]` of three clouds has a batch stride no contiguous tensor of its shape has"""
    from learning3d_amd.losses.chamfer_distance import ChamferDistanceFunction
    m = _common()
    a, b = rnd(3, N, 3, seed=110), rnd(3, M, 3, seed=111)
    run_on_views(nograd(m.square_distance), [a, b], views_of([a, b], kinds=("rows", "expand")), ["l3d_square_distance"], "square_distance, B = 3")
    run_on_views(nograd(ChamferDistanceFunction.apply), [a, b], views_of([a, b], kinds=("rows", "expand")), ["l3d_chamfer_forward"],
                 "ChamferDistanceFunction, B = 3")
    x = rnd(3, 3, N, seed=112)
    run_on_views(nograd(lambda x: m.knn(x, K)), [x], views_of([x], kinds=("rows", "transposed")), ["l3d_knn_graph"], "knn, B = 3")


# ------------------------------------------------------------------------------------------------------------------------------
# routes gated on layout: each side's log on its own, the values against fp64
def test_max_over_last_is_gated_on_contiguity():
    """models/_train.max_over_last: `x.is_contiguous()` gates l3d_max_last; a view takes torch's max.  A maximum is exact in every
    format, so both routes must equal the fp64 maximum exactly (the bar of test_gpu_grad_modules for this op's forward)."""
    from learning3d_amd.models import _train
    x = rnd(B, 32, N, K, seed=120)
    for kind, v in float_views(x, ("transposed", "channels", "rows", "expand")):
        dense = v.clone(memory_format=torch.contiguous_format)
        before = whole_storage(v).clone()
        with torch.no_grad():
            want, log = logged(_train.max_over_last, dense)
            got, vlog = logged(_train.max_over_last, v)
        assert log == ["l3d_max_last"] and vlog == [], (kind, log, vlog)
        ref = dense.double().max(dim=-1, keepdim=True)[0]
        assert got.shape == want.shape == ref.shape
        assert torch.equal(want.double(), ref) and torch.equal(got.double(), ref), kind
        assert torch.equal(whole_storage(v), before)


def test_sublayer_connection_transposed_add_is_gated_on_layout():
    """utils/transformer.SublayerConnection: x contiguous and the sublayer's result a transposed view of channel-first memory ->
    l3d_add_transposed; any other layout -> torch's add.  x + y is one rounding either way: both equal fp32(fp64 sum) exactly."""
    from learning3d_amd.utils.transformer import SublayerConnection
    sc = seeded_params(SublayerConnection(64), 121).cuda().eval()
    y_cf = rnd(B, 64, N, seed=122)                                 # what a fast sublayer returns: a [B,N,C] view of [B,C,N] memory
    x = rnd(B, N, 64, seed=123)
    for kind, v in [("contiguous", x)] + float_views(x):
        dense = v.clone(memory_format=torch.contiguous_format)
        with torch.no_grad():
            got, log = logged(sc, v, lambda normed: y_cf.transpose(1, 2))
        assert has_entry(log, "l3d_add_transposed") == (kind == "contiguous"), (kind, log)
        want = (dense.double() + y_cf.transpose(1, 2).double()).float()
        assert got.shape == want.shape and same_bits(got, want), kind


# ------------------------------------------------------------------------------------------------------------------------------
# the pointnet2_utils Functions assert contiguity like the reference: a view raises, nothing is launched
def _assert_only_cases():
    from learning3d_amd.utils import pointnet2_utils as p
    xyz, new = rnd(B, N, 3, seed=130), rnd(B, 32, 3, seed=131)
    feat = rnd(B, 8, N, seed=132)
    i32 = torch.int32
    return {
        "furthest_point_sample": (lambda a: p.furthest_point_sample(a, 16), [xyz], "l3d_furthest_point_sampling"),
        "gather_operation": (p.gather_operation, [feat, rint(N, B, 32, seed=133, dtype=i32)], "l3d_gather_points"),
        "knn": (lambda a, b: p.knn(4, a, b), [new, xyz], "l3d_knn"),
        "three_nn": (p.three_nn, [xyz, new], "l3d_three_nn"),
        "three_interpolate": (p.three_interpolate, [rnd(B, 8, 32, seed=134), rint(32, B, N, 3, seed=135, dtype=i32),
                                                    rnd(B, N, 3, seed=136).abs_()], "l3d_three_interpolate"),
        "grouping_operation": (p.grouping_operation, [feat, rint(N, B, 32, 8, seed=137, dtype=i32)], "l3d_group_points"),
        "ball_query": (lambda a, b: p.ball_query(0.5, 8, a, b), [xyz, new], "l3d_ball_query"),
    }


@pytest.mark.parametrize("name", ["furthest_point_sample", "gather_operation", "knn", "three_nn", "three_interpolate",
                                  "grouping_operation", "ball_query"])
def test_assert_only_wrappers_refuse_views_and_launch_nothing(name):
    from learning3d_amd import _lib
    fn, args, entry = _assert_only_cases()[name]
    with torch.no_grad():
        want, log = logged(fn, *args)
        again, _ = logged(fn, *args)
    assert log == [entry]
    assert_identical(again, want, name + ": two runs on the same input")
    views = views_of(args)
    assert len(views) == len(args)
    for i, kinds in views.items():
        for kind, v in kinds:
            before = whole_storage(v).clone()
            _lib.LAUNCH_LOG = log = []
            try:
                with torch.no_grad(), pytest.raises(AssertionError):
                    fn(*[v if j == i else a for j, a in enumerate(args)])
            finally:
                _lib.LAUNCH_LOG = None
            assert log == [], (name, i, kind, log)
            assert torch.equal(whole_storage(v), before)
