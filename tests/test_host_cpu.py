"""CPU-side tests: C-ABI library loads and exports every symbol include/l3d_hip.h declares (no
compute), host logic (argument validation, loud failure without a GPU), product path never touches
oracle/, and the N>1 path (gloo, world_size 2)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    """every entry point include/*.h declares: the boundary (l3d_hip.h) and the kernel-selection hooks (l3d_hip_testing.h)"""
    out = set()
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name.endswith(".h"):
            text = open(os.path.join(ROOT, "include", name)).read()
            text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
            out |= set(re.findall(r"\b(l3d_[a-z0-9_]+)\s*\(", text))
    return sorted(out)


def test_library_exports_every_declared_symbol():
    import ctypes
    from learning3d_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    syms = header_symbols()
    assert len(syms) >= 30
    for s in syms:
        assert hasattr(handle, s), f"{s} declared in include/l3d_hip.h but not exported"
    assert set(syms) == set(_lib.SIGNATURES), "ctypes table and header disagree"
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "l3d_hip.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(l3d_[a-z0-9_]+)\s*\(", text))) <= 98, "the boundary header grew past 98 entry points (90 + l3d_emd_workspace_bytes + l3d_probe_mfma_sustained, round 5; + l3d_chamfer_forward_loss, l3d_colsum_rows and their workspace sizes, l3d_split_f16_operand, round 6; + l3d_bmm_f32_route, the host-only query beside l3d_bmm_f32)"
    l = _lib.lib()
    assert l.l3d_version() >= 100
    assert b"invalid" in l.l3d_status_string(-1)


def test_prototypes_are_read_from_the_headers():
    """The ctypes table is derived from include/*.h: one prototype of every kind the parser must get right, held against
    literal expectations, and a header with a type outside the recognised set raises instead of producing a guess."""
    import ctypes as C
    from learning3d_amd import _lib
    P, I, L, F, D, SZ = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_double, C.c_size_t
    want = {
        "l3d_status_string": (C.c_char_p, [I]),
        "l3d_f16_image_bytes": (SZ, [I, L, I]),
        "l3d_bmm_f32": (I, [P, P, P, P, P, P, I, I, I, I, I, F, I, P, I, P, P]),
        "l3d_bmm_f32_route": (I, [P, P, P, P, I, I, I, I, I, I]),
        "l3d_bn_finalize": (I, [P, I, I, D, P, P, P, D, I, D, P, P, P, P, P, P, P, P]),
        "l3d_uniform_clouds": (I, [C.c_ulonglong, I, I, F, F, P, P]),
        "l3d_knn_graph": (I, [P, I, I, I, P, P]),
        "l3d_gaussian_density": (I, [P, I, I, F, P, P]),
    }
    for name, (restype, argtypes) in want.items():
        assert _lib.PROTOTYPES[name].restype is restype, name
        assert _lib.SIGNATURES[name] == argtypes, name
    assert len(_lib.SIGNATURES) == 113
    par = {name: [(p.ctype, p.name) for p in proto.params] for name, proto in _lib.PROTOTYPES.items()}
    assert par["l3d_knn_graph"][4] == ("int64_t *", "idx") and par["l3d_knn_graph"][5] == ("l3d_stream_t", "stream")
    assert par["l3d_bmm_f32"][1] == ("const long *", "a_strides") and par["l3d_bmm_f32"][11] == ("float", "alpha")
    assert par["l3d_edgeconv_pack"][0] == ("const float *const[]", "w")                 # an array of pointers
    assert par["l3d_uniform_clouds"][0] == ("unsigned long long", "seed")
    assert par["l3d_version"] == []
    # the integer #defines and the l3d_status enumerators come from the same place
    assert (_lib.L3D_OK, _lib.L3D_ERR_INVALID_ARG, _lib.L3D_ERR_UNSUPPORTED, _lib.L3D_ERR_LAUNCH) == (0, -1, -2, -3)
    assert (_lib.L3D_CONV_F16_TWO_PLANE, _lib.L3D_CONV_F16_OUT_UNSCALED, _lib.L3D_CONV_F16_SHIFT_N, _lib.L3D_KNN_MAX_K) == (1, 2, 4, 200)
    assert (_lib.L3D_BMM_ROUTE_YT_MASK, _lib.L3D_BMM_ROUTE_A_SHIFT, _lib.L3D_BMM_ROUTE_B_SHIFT, _lib.L3D_BMM_ROUTE_REMAPPED) == (3, 2, 4, 64)
    # the array form of a parameter, and what the parser must refuse
    protos, consts = _lib.parse_header("/* c */\n#define L3D_X 0x10\nint l3d_f(const long st[4], unsigned n,\n          l3d_stream_t stream);\n")
    assert consts == {"L3D_X": 16} and protos["l3d_f"].restype is I
    assert [(p.ctype, p.name) for p in protos["l3d_f"].params] == [("const long[]", "st"), ("unsigned", "n"), ("l3d_stream_t", "stream")]
    for bad in ("int l3d_f(const __half *x, int n);", "int l3d_f(struct s v);", "half l3d_f(void);", "int l3d_f(float *);",
                "int l3d_f(int (*cb)(int));"):
        with pytest.raises(_lib.L3DError, match=r"t\.h:3"):
            _lib.parse_header("\n\n" + bad + "\n", "t.h")


def test_an_entry_point_declared_by_two_headers_raises(tmp_path):
    """One table for every header of include/: the same name in two headers is an error that names both, not a silent overwrite."""
    from learning3d_amd import _lib
    (tmp_path / "a.h").write_text("#define L3D_A 1\nint l3d_f(const float *x, int n, l3d_stream_t stream);\n")
    (tmp_path / "b.h").write_text("#define L3D_B 2\nint l3d_g(int n);\n")
    protos, consts = _lib._parse_headers(str(tmp_path))
    assert sorted(protos) == ["l3d_f", "l3d_g"] and consts == {"L3D_A": 1, "L3D_B": 2}
    (tmp_path / "b.h").write_text("#define L3D_B 2\nint l3d_f(int n);\n")
    with pytest.raises(_lib.L3DError, match=r"l3d_f.*a\.h.*b\.h"):
        _lib._parse_headers(str(tmp_path))
    # the constants share one namespace too: the same value twice is fine, two values are not
    (tmp_path / "b.h").write_text("#define L3D_A 1\nint l3d_g(int n);\n")
    assert _lib._parse_headers(str(tmp_path))[1] == {"L3D_A": 1}
    (tmp_path / "b.h").write_text("#define L3D_A 3\nint l3d_g(int n);\n")
    with pytest.raises(_lib.L3DError, match=r"L3D_A is 1 in a\.h and 3 in b\.h"):
        _lib._parse_headers(str(tmp_path))


def test_call_checks_tensor_dtypes_before_devices():
    """_lib.call holds a tensor against the element type of the parameter it is passed for, before the device rule -- so on CPU
    tensors the dtype errors, and then the no-CPU-fallback error, are reached without a launch."""
    import ctypes as C
    from learning3d_amd import _lib
    f32, f64 = torch.zeros(1, 2, 8), torch.zeros(1, 2, 8, dtype=torch.float64)
    i32, i64 = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int64)
    out = torch.zeros(1, 2, 4)
    with pytest.raises(_lib.L3DError, match=r"l3d_gather_points.*`const float \*points`.*torch\.float32.*torch\.float64"):
        _lib.call("l3d_gather_points", 1, 2, 8, 4, f64, i32, out)
    with pytest.raises(_lib.L3DError, match=r"l3d_gather_points.*`const int32_t \*idx`.*torch\.int32.*torch\.int64"):
        _lib.call("l3d_gather_points", 1, 2, 8, 4, f32, i64, out)
    with pytest.raises(_lib.L3DError, match=r"l3d_gather_points.*`const float \*points`.*torch\.float16"):
        _lib.call("l3d_gather_points", 1, 2, 8, 4, f32.half(), i32, out)
    with pytest.raises(_lib.L3DError, match="no CPU fallback"):
        _lib.call("l3d_gather_points", 1, 2, 8, 4, f32, i32, out)
    # None for an optional pointer and a ctypes array for `const long *` get as far as the device rule
    st = (C.c_long * 4)(0, 0, 8, 1)
    with pytest.raises(_lib.L3DError, match="no CPU fallback"):
        _lib.call("l3d_bmm_f32", f32, st, f32, st, out, st, 1, 1, 2, 2, 8, 1.0, 0, None, 1, None)
    with pytest.raises(_lib.L3DError, match="no CPU fallback"):
        _lib.call("l3d_furthest_point_sampling", 1, 8, 4, torch.zeros(1, 8, 3), None, i32)
    # void * takes any dtype; a tensor for a scalar, a wrong argument count and an unknown name are errors
    with pytest.raises(_lib.L3DError, match="no CPU fallback"):
        _lib.call("l3d_split_rows", f32, 2, 8, torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(_lib.L3DError, match=r"l3d_gather_points.*`int npoints`.*by value"):
        _lib.call("l3d_gather_points", 1, 2, 8, i32, f32, i32, out)
    with pytest.raises(_lib.L3DError, match=r"l3d_gather_points.*8 arguments"):
        _lib.call("l3d_gather_points", 1, 2, 8, 4, f32, i32)
    with pytest.raises(KeyError):
        _lib.call("l3d_no_such_entry_point")
    log, _lib.LAUNCH_LOG = _lib.LAUNCH_LOG, []
    try:
        with pytest.raises(_lib.L3DError, match=r"l3d_knn_graph\[probe\]: .*invalid"):
            _lib.call("l3d_knn_graph", None, 1, 8, 4, None, None, tag="[probe]")       # stream given; NULL pointers: refused before any launch
        assert _lib.LAUNCH_LOG == ["l3d_knn_graph[probe]"]
    finally:
        _lib.LAUNCH_LOG = log


def test_argument_validation_without_gpu():
    from learning3d_amd import _lib
    l = _lib.lib()
    # null pointers / bad sizes are rejected before any launch
    assert l.l3d_knn_graph(None, 1, 8, 4, None, None) == -1
    assert l.l3d_chamfer_forward(None, None, 1, 1, 1, None, None, None, None, None) == -1
    assert l.l3d_ball_query(1, 0, 1, 0.5, 4, None, None, None, None, None) == -1
    # + the f16x2 copy, its biases, 16 scales; + the two-plane copy (2/3 of the planes), its biases, layer 1 scaled, 16 constants
    assert l.l3d_edgeconv_packed_floats(64, 64, 128, 256) == 46080 + 45568 + 67584 + 67584 + 448 + 16 + (45056 + 448 + 512 + 64 + 16)
    assert l.l3d_edgeconv_packed_floats(32, 32, 64, 128) == 0
    # round-2 entry points: same contract (null / non-positive -> -1; shapes the kernels do not take -> -2, before any launch)
    import ctypes as C
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    assert l.l3d_group_first_layer(None, None, None, None, None, None, None, 1, 8, 4, 2, 32, 1, None, None) == -1
    assert l.l3d_group_first_layer(p, None, None, p, p, p, p, 1, 8, 4, 2, 30, 1, p, None) == -2          # C1 % 4
    assert l.l3d_first_layer_f16_planes(None, 1, None, None, None, 1, 3, 128, 256, 1, None, None, None) == -1
    assert l.l3d_first_layer_f16_planes(p, 1, p, None, p, 1, 9, 128, 256, 1, p, None, None) == -2         # Cin > 8
    assert l.l3d_pointwise_conv_f16(p, p, None, None, 0, 1, 128, 256, 256, 0, 0, None, None, None, None, None, 128, None, 0, None) == -1   # no output asked for
    assert l.l3d_pointwise_conv_f16(p, p, None, None, 0, 1, 128, 256, 256, 0, 0, None, None, p, None, None, 128, None, 0, None) == -1      # image without obs
    assert l.l3d_pointwise_conv_f16(p, p, None, None, 0, 1, 128, 256, 256, 0, 0, None, None, None, None, p, 24, None, 0, None) == -2       # pool not a supported run length
    assert l.l3d_pointwise_conv_f16(p, p, None, None, 0, 1, 128, 128, 256, 0, 0, None, None, None, None, p, 8, None, 0, None) == -2        # narrow tile wants N % 512
    assert l.l3d_pointwise_conv_f16(p, p, None, None, 0, 1, 128, 256, 256, 0, 0, p, None, None, None, None, 0, p, 100, None) == -2        # group size % 256
    assert l.l3d_pointwise_conv_f16(p, p, None, None, 0, 1, 128, 256, 256, 0, 0, p, None, p, p, None, 0, None, 0, None) == -2          # fp32 rows AND an image
    assert l.l3d_pointwise_conv_f16(p, p, None, None, 0, 1, 128, 256, 256, 0, 8, p, None, None, None, None, 0, None, 0, None) == -1     # unknown flag
    assert l.l3d_pointwise_conv_f16(p, p, None, None, 0, 1, 128, 256, 256, 0, 2, p, None, None, None, None, 0, None, 0, None) == -2     # unscaled OUTPUT image without the two-plane input form / an image
    assert l.l3d_layernorm_planes_cf(p, p, p, 1e-6, 1, 512, 64, p, None, 2, None) == -1                            # unknown flag
    assert l.l3d_colsum_rows(p, 4, 8, 4, p, p, None) == -1                                                        # row stride < cols
    assert l.l3d_pointwise_conv_f16(p, p, None, None, 0, 1, 128, 256, 256, 0, 4, p, None, None, None, None, 0, None, 0, None) == -2     # column-indexed shift without the two-plane form
    assert l.l3d_split_f16_operand(p, 8, 16, 8, 0, p, None, None) == -1                                            # row stride < cols
    assert l.l3d_split_f16_operand(p, 8, 16, 16, 2, p, None, None) == -1                                           # no such kind
    assert l.l3d_layernorm_planes(p, p, p, 1e-6, 4, 520, None, p, None) == -2                                      # C > 512
    # round-3 entry points
    assert l.l3d_knn_variant(1, 8, 8, 4, p, p, p, p, 7, None) == -1                                                # no such variant
    assert l.l3d_knn_variant(1, 8, 8, 4, None, p, p, p, 0, None) == -1
    assert l.l3d_knn_variant(1, 8, 9000, 64, p, p, p, p, 2, None) == -2                                            # selection kernel: <= 8192 candidates
    assert l.l3d_knn_variant(1, 8, 64, 5, p, p, p, p, 3, None) == -2                                               # four-slot kernel: k <= 4
    assert l.l3d_layernorm_ref_backward(None, p, p, 1e-6, 4, 64, p, p, p, p, None) == -1
    assert l.l3d_layernorm_ref_backward(p, p, p, 1e-6, 4, 66, p, p, p, p, None) == -2                              # C % 4
    assert l.l3d_layernorm_backward_workspace_floats(8192, 512) == 256 * 2 * 512
    assert l.l3d_layernorm_backward_workspace_floats(6, 64) == 2 * 2 * 64
    # size limits, refused before any launch (the Python wrappers route these shapes elsewhere and must not raise)
    assert l.l3d_scatter_add_det(p, p, None, 1, 2, 1 << 22, 1024, 1, p, p, None) == -2          # (target << 10 | lane) would reach 0xFFFFFFFF
    assert l.l3d_scatter_add_det(p, p, None, 1, 2, 1 << 21, 2048, 1, p, p, None) == -2          # two placement ranges: T * 2 >= 2^22
    assert l.l3d_scatter_add_det(p, p, None, 1, 2, 524288, 8192, 1, p, p, None) == -2           # eight ranges: T * 8 >= 2^22
    assert l.l3d_furthest_point_sampling(1, 16385, 64, p, None, p, None) == -1                  # past 512 x 32 points: temp required
    assert l.l3d_farthest_point_sample(p, 1, 16385, 64, None, None, p, None) == -1
    assert l.l3d_furthest_point_sampling(1, 1 << 25, 64, p, p, p, None) == -2                   # tie key: 15 bits of k >> 10
    assert l.l3d_knn_feature(p, 1, 64, 16385, 20, p, p, None) == -2                             # FK_MAXNP = 16384
    assert l.l3d_edge_gather_max(p, p, 1, 64, 32769, 20, 0, p, 64 * 32769, None) == -2          # a channel row of N floats in LDS
    # l3d_bmm_f32_route: host arithmetic on the pointer's alignment, the strides and the sizes -- l3d_bmm_f32's statuses, else its choice
    def st(*s):
        return (C.c_long * 4)(*s)
    route = lambda a, sa, b, sb, *sizes: l.l3d_bmm_f32_route(a, sa, b, sb, *sizes)
    al, off = C.c_void_p(p.value & ~15), C.c_void_p((p.value & ~15) + 4)
    assert route(None, st(0, 0, 8, 1), al, st(0, 0, 8, 1), 1, 1, 8, 8, 8, 1) == -1
    assert route(al, st(0, 0, 8, 1), al, st(0, 0, 8, 1), 1, 1, 8, 0, 8, 1) == -1
    assert route(al, st(0, 0, 8, 1), al, st(0, 0, 8, 1), 1, 1, 8, 8, 8, 0) == -1                                   # parts < 1
    assert route(al, st(0, 0, 8, 1), al, st(0, 0, 8, 1), 256, 256, 8, 8, 8, 1) == -2                               # grid z > 65535
    assert l.l3d_bmm_f32(al, st(0, 0, 8, 1), al, st(0, 0, 8, 1), al, st(0, 0, 8, 1), 256, 256, 8, 8, 8, 1.0, 0, None, 1, None, None) == -2
    # A [2048 x 32] plain: 16-byte loads along k (1); B [32 x 1024] plain = rows contiguous (2); 16 x 8 tiles x 4 = 512: YT 2, remapped
    big = (4, 1, 2048, 1024, 32, 1)
    assert route(al, st(65536, 0, 32, 1), al, st(32768, 0, 1024, 1), *big) == 2 | 1 << 2 | 2 << 4 | 64
    assert route(al, st(65536, 0, 1, 2048), al, st(32768, 0, 1, 32), *big) == 2 | 2 << 2 | 1 << 4 | 64               # both transposed
    assert route(off, st(65536, 0, 32, 1), off, st(32768, 0, 1024, 1), *big) == 2 | 64                             # misaligned: scalar loads
    assert route(al, st(65536, 0, 32, 1), al, st(32768, 0, 1024, 1), 3, 1, 2048, 1024, 32, 1) == 1 | 1 << 2 | 2 << 4 | 64   # 384 tiles: YT 1
    assert route(al, st(65536, 0, 32, 1), al, st(32768, 0, 1024, 1), 4, 1, 2100, 1024, 32, 1) == 2 | 1 << 2 | 2 << 4  # 17 row tiles: plain order
    assert route(al, st(65536, 0, 32, 1), al, st(32768, 0, 64, 1), 64, 1, 2048, 64, 32, 1) == 1 | 1 << 2 | 2 << 4 | 64  # N <= 64 never takes YT 2


def test_product_path_fails_loudly_on_cpu_tensors():
    import learning3d_amd.utils as U
    from learning3d_amd.losses import ChamferDistanceLoss
    from learning3d_amd._lib import L3DError
    x = torch.rand(1, 3, 16)
    with pytest.raises(L3DError):
        U.knn(x, 4)
    with pytest.raises(L3DError):
        ChamferDistanceLoss()(torch.rand(1, 8, 3), torch.rand(1, 8, 3))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "learning3d_amd")
    bad = []
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(d, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b|liboracle|oracle/", src, flags=re.M):
                    bad.append(os.path.join(d, f))
    assert not bad, f"product files reference the oracle: {bad}"


def test_reference_api_surface():
    import learning3d_amd.utils as U
    import learning3d_amd.losses as Ls
    import learning3d_amd.models as Mo
    for name in ["knn", "get_graph_feature", "square_distance", "index_points", "farthest_point_sample",
                 "knn_point", "query_ball_point", "SVDHead", "pointnet2_utils"]:
        assert hasattr(U, name)
    for name in ["furthest_point_sample", "gather_operation", "knn", "three_nn", "three_interpolate",
                 "grouping_operation", "ball_query", "QueryAndGroup", "GroupAll"]:
        assert hasattr(U.pointnet2_utils, name)
    assert hasattr(Ls, "ChamferDistanceLoss") and hasattr(Ls, "EMDLoss")
    ref_keys = {"conv1.weight", "conv5.weight", "bn1.running_mean", "bn5.bias"}
    assert ref_keys <= set(Mo.DGCNN(emb_dims=64).state_dict())
    assert {"conv1.weight", "conv1.bias", "bn5.weight"} <= set(Mo.PointNet(use_bn=True).state_dict())
    assert {"conv4.weight", "linear3.bias", "conv7.weight"} <= set(Mo.PCN(detailed_output=True).state_dict())


def test_shard_bounds_cover_batch():
    from learning3d_amd.parallel import shard_bounds
    for B in (1, 7, 32, 256):
        for W in (1, 2, 3, 8):
            spans = [shard_bounds(B, r, W) for r in range(W)]
            assert spans[0][0] == 0 and spans[-1][1] == B
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))


WORKER = r"""
import os, sys
sys.path.insert(0, {root!r})
import numpy as np, torch, torch.distributed as dist
import oracle
from learning3d_amd import parallel
rank, world, _ = parallel.init_from_env(backend="gloo")
g = torch.Generator().manual_seed(0)
a = torch.rand((6, 64, 3), generator=g).numpy(); b = torch.rand((6, 80, 3), generator=g).numpy()
lo, hi = parallel.shard_bounds(6, rank, world)
d1, d2, _, _ = oracle.chamfer_forward(a[lo:hi], b[lo:hi])          # stands in for the HIP kernel on this rank
part = torch.tensor([np.sqrt(d1).astype(np.float64).sum(), np.sqrt(d2).astype(np.float64).sum(), d1.size, d2.size], dtype=torch.float64)
loss = parallel.allgather_chamfer_loss(part)
want = float(oracle.chamfer_loss(a, b))
assert abs(float(loss) - want) < 1e-6, (float(loss), want)
# pipelined exchange: step i's loss comes back from submit(i+1) / flush(), values scaled per step
pipe = parallel.PipelinedChamferLoss()
got = []
for step in range(4):
    scaled = part.clone(); scaled[:2] *= (step + 1)
    out = pipe.submit(scaled)
    assert (out is None) == (step == 0)
    if out is not None: got.append(float(out))
got.append(float(pipe.flush()))
assert pipe.flush() is None
for step, v in enumerate(got):
    assert abs(v - want * (step + 1)) < 1e-5 * (step + 1), (step, v, want)
print("RANK", rank, "OK", float(loss))
dist.barrier(); dist.destroy_process_group()
"""


def test_two_rank_gloo_chamfer_allgather(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT))
    import socket
    with socket.socket() as sk:                              # a free rendezvous port, not a fixed one
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", port, str(script)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("OK") == 2


def test_small_losses_match_their_definitions():
    """learning3d.losses' four torch-only losses against their closed forms."""
    import torch
    import torch.nn.functional as F
    from learning3d_amd.losses import RMSEFeaturesLoss, FrobeniusNormLoss, ClassificationLoss, CorrespondenceLoss
    g = torch.Generator().manual_seed(3)
    d = torch.randn((4, 7), generator=g)
    assert torch.allclose(RMSEFeaturesLoss()(d), (d ** 2).sum())
    P, G = torch.randn((3, 4, 4), generator=g), torch.randn((3, 4, 4), generator=g)
    want = ((P @ G - torch.eye(4)) ** 2).mean() * 16
    assert torch.allclose(FrobeniusNormLoss()(P, G), want)
    logp = F.log_softmax(torch.randn((5, 6), generator=g), dim=1)
    tgt = torch.tensor([0, 5, 2, 2, 1])
    assert torch.allclose(ClassificationLoss()(logp, tgt), -logp[torch.arange(5), tgt].mean())
    B, Nt, Ns = 2, 6, 5
    pred = torch.randn((B, Ns, Nt), generator=g)
    gt = torch.zeros((B, Nt, Ns))
    lab = torch.randint(0, Nt, (B, Ns), generator=g)
    for b in range(B):
        gt[b, lab[b], torch.arange(Ns)] = 1
    want = F.cross_entropy(pred.reshape(B * Ns, Nt), lab.reshape(-1))
    got = CorrespondenceLoss()(torch.zeros(B, 3, Nt), torch.zeros(B, 3, Ns), pred, gt)
    assert torch.allclose(got, want)


def test_kabsch_backward_matches_autograd_of_reference_sequence():
    """SVDHead's analytic Kabsch backward (learning3d_amd/utils/svd.py) against torch autograd through the reference's
    own op sequence (utils/svd.py:29-58: centring, H, torch.svd, V U^T, det fix with `reflect`, t), fp64, including
    clouds whose best orthogonal fit is a reflection (the det < 0 branch)."""
    import torch
    from learning3d_amd.utils.svd import kabsch_backward
    torch.manual_seed(0)
    B, N = 6, 40
    src = torch.randn(B, 3, N, dtype=torch.float64)
    corr = torch.randn(B, 3, N, dtype=torch.float64)
    mirror = torch.diag(torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64))
    corr[3:] = mirror @ src[3:] + 0.05 * torch.randn(3, 3, N, dtype=torch.float64)     # reflection is the best fit
    src.requires_grad_(); corr.requires_grad_()
    sc = src - src.mean(2, keepdim=True)
    cc = corr - corr.mean(2, keepdim=True)
    H = sc @ cc.transpose(2, 1)
    Rs, dets = [], []
    for i in range(B):
        u, s, v = torch.svd(H[i])
        r = v @ u.t()
        dets.append(float(torch.det(r.detach())))
        if dets[-1] < 0:
            r = (v @ mirror) @ u.t()
        Rs.append(r)
    assert min(dets) < 0 < max(dets)                       # both branches exercised
    R = torch.stack(Rs)
    t = (torch.matmul(-R, src.mean(2, keepdim=True)) + corr.mean(2, keepdim=True)).view(B, 3)
    gR, gt = torch.randn_like(R), torch.randn_like(t)
    ((R * gR).sum() + (t * gt).sum()).backward()
    g_src, g_corr = kabsch_backward(src.detach(), corr.detach(), R.detach(), gR, gt)
    assert (g_src - src.grad).abs().max() < 1e-10 * max(1.0, float(src.grad.abs().max()))
    assert (g_corr - corr.grad).abs().max() < 1e-10 * max(1.0, float(corr.grad.abs().max()))


def test_bench_self_launches_two_ranks_gloo():
    """`python bench.py --gpus 2` with no launcher around it must start its own ranks.  The
    --selftest-cpu mode runs the launcher, init_from_env, the loss all_gather (blocking and pipelined), the barrier /
    max-over-ranks bracket and the JSON line on gloo; no kernel and no oracle is involved."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--selftest-cpu"],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    j = json.loads(line)
    assert j["n_gpus"] == 2 and j["rccl_ranks"] == 2 and len(j["per_rank_s"]) == 2
    assert abs(j["loss_sync"] - j["loss_expected"]) < 1e-6 and abs(j["loss_pipelined"] - j["loss_expected"]) < 1e-6
    assert j["rank0_placement"]["torch_threads"] >= 1
    # --workload c5's exchange (all_gather_into_tensor of the shard digest) through the same launcher
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--selftest-cpu",
                          "--workload", "c5"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert j["workload"] == "c5" and j["rccl_ranks"] == 2 and j["digest"] == j["digest_expected"]


def _bn_stats_rank(rank, world, port, q, NB=8, mode="declared"):
    import os
    import numpy as np
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from learning3d_amd import parallel
    from learning3d_amd.models import _train
    rng = np.random.default_rng(5)
    z = rng.standard_normal((NB, 16, 300)).astype(np.float32)              # the WHOLE batch, same on every rank
    lo, hi = parallel.shard_bounds(z.shape[0], rank, world)
    if mode == "declared" and NB % world:
        parallel.declare_global_batch(NB, world)                              # uneven shards are declared, not asked for per layer
    elif mode == "shard":
        assert tuple(parallel.shard(torch.from_numpy(z[:5]), rank, world).shape[1:]) == (16, 300) and _train._SHARD_SIZES is None   # pure
        assert tuple(parallel.shard(torch.from_numpy(z), rank, world, declare=True).shape) == (hi - lo, 16, 300)   # declares what it cuts
    zs = z[lo:hi].astype(np.float64)
    # per-cloud fp64 partial sums of this rank's shard: the stand-in for l3d_channel_stats (tested on the GPU against numpy)
    part = torch.from_numpy(np.stack([zs.sum(-1), (zs ** 2).sum(-1)], axis=-1))
    if mode == "undeclared_after_even":
        # two steps of 4 + 4 clouds come first, undeclared; the last batch is 4 + 3.  Rank 0's local count (4) does not
        # change, rank 1's does: a per-count cache put the two ranks into different collectives here.
        ze = rng.standard_normal((8, 16, 300)).astype(np.float64)
        elo, ehi = parallel.shard_bounds(8, rank, world)
        pe = torch.from_numpy(np.stack([ze[elo:ehi].sum(-1), (ze[elo:ehi] ** 2).sum(-1)], axis=-1))
        for _ in range(2):
            assert tuple(_train.gather_cloud_partials(pe).shape) == (8, 16, 2)
    pg = _train.gather_cloud_partials(part)
    mean, var, n, tot = _train.stats_from_partials(pg, z.shape[2])
    q.put((rank, pg.numpy().tobytes(), tot.numpy().tobytes(), mean.numpy().tobytes(), var.numpy().tobytes(), n))
    dist.destroy_process_group()


@pytest.mark.parametrize("NB,mode", [(8, "declared"), (7, "declared"), (7, "undeclared"), (7, "shard"), (7, "undeclared_after_even")])
def test_two_rank_gloo_batchnorm_statistics_bit_identical(NB, mode):
    """train-mode BatchNorm statistics over a batch sharded across 2 ranks (gloo) equal the
    single-process statistics BIT FOR BIT: per-cloud fp64 partial sums, all_gather, addition in global cloud order.
    NB = 7: an uneven last batch (4 + 3 clouds), padded for the gather -- declared with parallel.declare_global_batch, declared by
    parallel.shard(declare=True), or NOT declared at all (the exchange discovers the sizes on every call: ADVICE r4 -- undeclared
    uneven shards used to launch a collective with mismatched sizes; ADVICE r5 -- also right behind even steps of the same local
    count on rank 0, where a per-count cache sent the ranks into different collectives)."""
    import socket
    import numpy as np
    import torch
    import torch.multiprocessing as mp
    from learning3d_amd.models import _train
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_bn_stats_rank, args=(r, 2, port, q, NB, mode)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    rng = np.random.default_rng(5)
    z = rng.standard_normal((NB, 16, 300)).astype(np.float32).astype(np.float64)
    part = torch.from_numpy(np.stack([z.sum(-1), (z ** 2).sum(-1)], axis=-1))
    mean, var, n, tot = _train.stats_from_partials(part, 300)
    for rank, pg, t, m, v, nn_ in got:
        assert pg == part.numpy().tobytes() and t == tot.numpy().tobytes()
        assert m == mean.numpy().tobytes() and v == var.numpy().tobytes() and nn_ == n


def test_emd_workspace_size_is_a_pure_host_function():
    """l3d_emd_workspace_bytes needs no device: remainders (n + m) + ten levels of ratios (10 (n + m)) + one cost partial per
    (512 k, 64 l) tile of the match kernel, floats, per cloud; 0 for nonsense sizes."""
    import ctypes
    from learning3d_amd import _lib
    h = ctypes.CDLL(_lib.LIB_PATH)
    h.l3d_emd_workspace_bytes.restype = ctypes.c_size_t
    assert h.l3d_emd_workspace_bytes(2, 100, 50) == 4 * 2 * (11 * 150 + 1)
    assert h.l3d_emd_workspace_bytes(32, 1024, 1024) == 4 * 32 * (11 * 2048 + 2 * 16)
    assert h.l3d_emd_workspace_bytes(0, 10, 10) == 0 and h.l3d_emd_workspace_bytes(1, -1, 10) == 0


def test_integration_md_shims_match_the_library():
    """INTEGRATION.md is the binding a maintainer would add: its python shims must compile, call only exported entry
    points with the number of arguments the C ABI declares, and the prose must not name a symbol that does not exist."""
    import ast
    import re
    from learning3d_amd import _lib
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    named = set(re.findall(r"\bl3d_[a-z0-9_]+\b", text))
    known = set(_lib.SIGNATURES)
    # prose may abbreviate families ("l3d_*_grad", "_workspace_bytes"); full names must exist
    unknown = {n for n in named if n not in known and n not in ("l3d_hip", "l3d_status")
               and not any(k.startswith(n) for k in known)}
    assert not unknown, f"INTEGRATION.md names entry points the library does not export: {sorted(unknown)}"
    blocks = re.findall(r"```python\n(.*?)```", text, flags=re.S)
    shims = [b for b in blocks if "_l3d." in b]
    assert len(shims) >= 4
    src = "\n".join(shims)
    tree = ast.parse(src)                                   # the shims are valid python
    calls = 0
    for node in ast.walk(tree):
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)
                and isinstance(node.func.value, ast.Name) and node.func.value.id == "_l3d"):
            name = node.func.attr
            assert name in known, name
            if any(isinstance(a, ast.Starred) for a in node.args):
                continue
            assert len(node.args) == len(_lib.SIGNATURES[name]), \
                f"{name}: shim passes {len(node.args)} arguments, the C ABI takes {len(_lib.SIGNATURES[name])}"
            calls += 1
    assert calls >= 14


def test_hot_kernels_compile_without_scratch():
    """No kernel of the library spills or indexes a private array (a spilled register in conv_f16_kernel was a silent
    35 % on its main loop, LABLOG R2.4h): EVERY code object in libl3d_hip.so is read (tools/kernel_meta.py: AMDGPU metadata notes, no
    GPU needed) and must show 0 bytes of scratch and 0 spilled registers -- except three named instantiations no BASELINE config
    launches (3-4 spilled registers) and the SVD head's score kernel, which measured faster with its spills than without.  The kernels of the benchmark step and the f16x2 GEMMs also keep a register budget."""
    import importlib.util
    from learning3d_amd import _lib
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    meta = km.kernel_metadata(_lib.LIB_PATH)
    assert len(meta) > 200                                   # every translation unit's code object was found
    allowed = {"_Z12topk2_kernelILi64ELi1ELi2EE": 4,          # knn_point with 32 < k <= 64 in the direct metric, two waves: no caller in configs 1-5
               "_Z15fold_mlp_kernelILi5EE": 3,                # PCN's folding decoder in the bf16x3 range-fallback arithmetic
               "_Z17knn_select_kernelILi128EE": 3,            # 64 < k <= 128 between two clouds: no caller in the reference
               "_Z15softcorr_kernelILi0EE": 27}               # SVD head's bf16x3 scores: two workgroups per CU WITH 27 spilled registers run
                                                              # 252 us, one without 304 (round 6, profiles/round6_dcp_forward_kernels.txt)
    dirty = {}
    for name, k in meta.items():
        sc, sp = k.get(".private_segment_fixed_size", 0), k.get(".vgpr_spill_count", 0)
        if sc or sp:
            dirty[name] = (sc, sp)
    for name, (sc, sp) in dirty.items():
        ok = [a for a in allowed if name.startswith(a)]
        assert ok and sp <= allowed[ok[0]] and sc <= 4 * allowed[ok[0]] + 8, f"{name}: {sc} bytes of scratch, {sp} spilled registers"
    assert not any("rocprim" in n for n in meta), "a library kernel is linked into libl3d_hip.so"
    hot = {"_Z15conv_f16_kernelILb0ELb0ELb0ELi3ELb0ELb0ELb0EE": 224,    # Linear layers / PCN (wide tile, three weight planes): VGPR budget 218 today
           "_Z15conv_f16_kernelILb0ELb0ELb0ELi2ELb0ELb0ELb0EE": 224,    # conv5 of the benchmark step (wide tile, two weight planes)
           "_Z15conv_f16_kernelILb1ELb0ELb0ELi3ELb0ELb0ELb0EE": 224,    # narrow tile
           "_Z15conv_f16_kernelILb0ELb0ELb0ELi3ELb1ELb0ELb0EE": 224,    # residual epilogue (the pointer network's sublayers)
           "_Z15conv_f16_kernelILb0ELb1ELb0ELi3ELb0ELb0ELb0EE": 232,    # + operand maxima (the fused q|k|v projection: 20 % of DCP's forward)
           "_Z15conv_f16_kernelILb0ELb0ELb1ELi3ELb0ELb0ELb0EE": 232,    # + pooled maxima over a group's K neighbours
           "_Z15conv_f16_kernelILb0ELb0ELb0ELi2ELb1ELb0ELb0EE": 224,    # round 6, the pointer network on two-plane images: residual epilogue,
           "_Z15conv_f16_kernelILb0ELb1ELb0ELi2ELb0ELb0ELb0EE": 224,    #   operand maxima,
           "_Z15conv_f16_kernelILb0ELb0ELb0ELi2ELb0ELb1ELb0EE": 224,    #   plane output with an unscaled residual
           "_Z15conv_f16_kernelILb0ELb0ELb0ELi2ELb0ELb0ELb1EE": 224,    # the training path's rows-as-weights product (bias along n)
           "_Z14bmm_f32_kernelILi2ELi1ELi1EE": 128,                 # the training GEMM's vector-fetch forms: four workgroups per CU
           "_Z14bmm_f32_kernelILi2ELi1ELi2EE": 128,
           "_Z14bmm_f32_kernelILi2ELi2ELi1EE": 128,
           "_Z14bmm_f32_kernelILi2ELi2ELi2EE": 128,
           "_Z26layernorm_planes_cf_kernelILi64ELi8EE": 128,
           "_Z20edgeconv_f16b_kernelILi5ELb1EE": 512,       # the two-plane, persistent kernel of the benchmark step
           "_Z20edgeconv_f16b_kernelILi5ELb0EE": 512,
           "_Z15knn_mfma_kernelILi8EE": 256,
           "_Z25chamfer_fwd_packed_kernel": 128,
           "_Z14featknn_kernel": 256,                       # all nine instantiations (round 6)
           "_Z19fold_mlp_f16_kernelILi5EE": 256}
    for prefix, vgpr_max in hot.items():
        ks = [k for n, k in meta.items() if n.startswith(prefix)]
        assert len(ks) >= 1, prefix                              # every instantiation behind the prefix
        for k in ks:
            assert k.get(".private_segment_fixed_size", 0) == 0 and k.get(".vgpr_spill_count", 0) == 0, (prefix, k)
            assert k.get(".vgpr_count", 0) <= vgpr_max, (prefix, k.get(".vgpr_count"))


def test_every_conditional_region_has_a_driver():
    """The product build compiles learning3d_amd/csrc with ONE set of flags, so a preprocessor region there is live only through a
    tool that builds the source with the macro set (a probe that includes it, tools/variant_lab.py, tools/build_variant_lib.py).
    Every macro in an #if / #ifdef / #elif condition (and in an #ifndef that is not the `#ifndef X / #define X v` default idiom)
    must be named by a file under tools/: a region nothing can switch on is deleted, not kept (LABLOG R15.1)."""
    csrc = os.path.join(ROOT, "learning3d_amd", "csrc")
    used = []                                                 # (file, line, macro)
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".hip", ".h")):
            continue
        lines = open(os.path.join(csrc, name)).read().split("\n")
        for i, line in enumerate(lines):
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", line)
            if not m:
                continue
            cond = re.sub(r"//.*|/\*.*?\*/", "", m.group(2))
            macros = set(re.findall(r"\b[A-Za-z_]\w*\b", cond)) - {"defined", "__HIPCC__", "__cplusplus"}
            if m.group(1) == "ifndef" and i + 1 < len(lines) and re.match(r"\s*#\s*define\s+%s\b" % re.escape(cond.strip()), lines[i + 1]):
                continue                                      # a default value (or an include guard), not a choice of code
            used += [(name, i + 1, mac) for mac in sorted(macros)]
    assert {"CF_TIMING", "CF_TIMELINE", "KS_TIMING"} <= {mac for _, _, mac in used}, "the scan misses conditions that are there"
    tools_text = ""
    for d, _, files in os.walk(os.path.join(ROOT, "tools")):
        for f in sorted(files):
            if f.endswith((".py", ".hip", ".cpp", ".h", ".inc", ".sh")):
                tools_text += open(os.path.join(d, f), errors="replace").read() + "\n"
    named = {mac for mac in {mac for _, _, mac in used} if re.search(r"(?:(?<!\w)|(?<=-D))%s(?!\w)" % re.escape(mac), tools_text)}   # X, or -DX
    orphans = [f"learning3d_amd/csrc/{name}:{line}: {mac}" for name, line, mac in used if mac not in named]
    assert not orphans, "conditional regions that no file under tools/ can switch on:\n" + "\n".join(orphans)
