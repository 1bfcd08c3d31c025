"""The launch-boundary audit (tests/golden/layout_audit.py) without a GPU: the wrapper it puts in front of `_lib.call` lets dense
tensors through, refuses views with the header's parameter name in the message, holds the six stride-taking entry points to the
strides they are passed, and is gone after the test.  The launch is a stub that records what reached it: nothing is launched."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import layout_audit                                      # noqa: E402
from layout_audit import LayoutError                     # noqa: E402


def st4(t):
    return (ctypes.c_long * 4)(*t.stride())


@pytest.fixture
def audited(monkeypatch):
    reached = []
    call = layout_audit.install(monkeypatch, inner=lambda name, *args, **kw: reached.append(name))
    return call, reached


def test_every_stride_parameter_of_the_headers_has_a_rule():
    from learning3d_amd import _lib
    assert layout_audit.uncovered_stride_parameters(_lib.PROTOTYPES) == []
    for (name, param), rule in layout_audit.STRIDED.items():           # each entry cites parameters its header declares
        names = [p.name for p in _lib.PROTOTYPES[name].params]
        sizes = [n for d in rule.dims for n in (d if isinstance(d, tuple) else (d,))]
        assert param in names and rule.stride in names and all(n in names for n in sizes), (name, param)
    for (name, step), (tensor, full) in layout_audit.DENSE_STEPS.items():
        assert {step, tensor, full} <= {p.name for p in _lib.PROTOTYPES[name].params}, name
    assert sorted({k[0] for k in layout_audit.STRIDED}) == ["l3d_attention_forward_f16b", "l3d_attention_forward_strided", "l3d_bmm_f32",
                                                            "l3d_bmm_f32_route", "l3d_colsum_rows", "l3d_edge_gather_max", "l3d_split_f16_operand"]


def test_a_new_stride_taking_entry_point_fails_the_audit(audited, monkeypatch):
    from learning3d_amd import _lib
    call, reached = audited
    protos, _ = _lib.parse_header("int l3d_new_thing(const float *x, long x_bstride, int B, l3d_stream_t stream);")
    assert layout_audit.uncovered_stride_parameters(protos) == [("l3d_new_thing", "x_bstride")]
    monkeypatch.setitem(_lib.PROTOTYPES, "l3d_new_thing", protos["l3d_new_thing"])
    with pytest.raises(LayoutError, match=r"l3d_new_thing.*`long x_bstride`.*no rule"):
        call("l3d_new_thing", torch.zeros(2, 8), 8, 2)                  # even a dense tensor: the entry point is unknown ground
    assert reached == []


def test_dense_tensors_pass_and_views_are_refused_by_parameter_name(audited):
    call, reached = audited
    pts, idx, out = torch.zeros(1, 4, 8), torch.zeros((1, 6), dtype=torch.int32), torch.zeros(1, 4, 6)
    call("l3d_gather_points", 1, 4, 8, 6, pts, idx, out)
    call("l3d_gather_points", 1, 4, 8, 6, pts, idx[:, :6], out.unsqueeze(0)[0])      # views that are dense pass too
    assert reached == ["l3d_gather_points"] * 2 and call.checked == 2
    transposed = torch.zeros(1, 8, 4).transpose(1, 2)
    stride2 = torch.zeros((1, 12), dtype=torch.int32)[:, ::2]
    expanded = torch.zeros(1, 1, 6).expand(1, 4, 6)
    sliced = torch.zeros(3, 4, 16)[1:2, :, :8]
    for args, param, strides in (((transposed, idx, out), r"`const float \*points`", r"\(32, 1, 4\)"),
                                 ((pts, stride2, out), r"`const int32_t \*idx`", r"\(12, 2\)"),
                                 ((pts, idx, expanded), r"`float \*out`", r"\(6, 0, 1\)"),
                                 ((sliced, idx, out), r"`const float \*points`", r"\(64, 16, 1\)")):
        with pytest.raises(LayoutError, match=rf"l3d_gather_points: parameter {param} got a tensor of shape \(.*\) and strides {strides}"):
            call("l3d_gather_points", 1, 4, 8, 6, *args)
    assert reached == ["l3d_gather_points"] * 2, "a refused call reached the launch"


def test_refusal_comes_before_every_check_of_the_real_call(monkeypatch):
    """through the real `call`: CPU tensors end in its `no CPU fallback`, so a LayoutError shows the audit ran first"""
    from learning3d_amd import _lib
    call = layout_audit.install(monkeypatch)
    pts, idx, out = torch.zeros(1, 4, 8), torch.zeros((1, 6), dtype=torch.int32), torch.zeros(1, 4, 6)
    with pytest.raises(_lib.L3DError, match="no CPU fallback"):
        call("l3d_gather_points", 1, 4, 8, 6, pts, idx, out)
    with pytest.raises(LayoutError, match="points"):
        call("l3d_gather_points", 1, 4, 8, 6, torch.zeros(1, 8, 4).transpose(1, 2), idx, out)
    with pytest.raises(_lib.L3DError, match="8 arguments"):               # malformed calls are left to `call`
        call("l3d_gather_points", 1, 4, 8, 6, pts, idx)


def test_bmm_strides_must_be_the_tensors_own(audited):
    call, reached = audited
    a = torch.zeros(2, 3, 16, 8).transpose(2, 3)                          # [2,3,8,16]: M = 8, K = 16, read through swapped strides
    b = torch.zeros(1, 1, 16, 4).expand(2, 3, 16, 4)                      # one matrix for the batch
    c = torch.zeros(2, 3, 8, 8)[..., :4]
    tail = (2, 3, 8, 4, 16, 1.0, 0, None, 1, None)
    call("l3d_bmm_f32", a, st4(a), b, st4(b), c, st4(c), *tail)
    assert reached == ["l3d_bmm_f32"]
    with pytest.raises(LayoutError, match=r"`const float \*A`.*strides \(384, 128, 1, 8\), but `a_strides` passes \(384, 128, 16, 1\)"):
        call("l3d_bmm_f32", a, st4(a.contiguous()), b, st4(b), c, st4(c), *tail)
    with pytest.raises(LayoutError, match=r"`const float \*B`.*`b_strides` passes"):
        call("l3d_bmm_f32", a, st4(a), b, st4(b.contiguous()), c, st4(c), *tail)
    with pytest.raises(LayoutError, match=r"`float \*C`.*`c_strides` passes"):
        call("l3d_bmm_f32", a, st4(a), b, st4(b), c, st4(c.contiguous()), *tail)
    with pytest.raises(LayoutError, match=r"`const float \*A`.*make it \(2, 3, 8, 16\)"):
        call("l3d_bmm_f32", a.transpose(2, 3), st4(a.transpose(2, 3)), b, st4(b), c, st4(c), *tail)
    wide = torch.zeros(1, 1, 8, 4).expand(2, 3, 8, 4)
    with pytest.raises(LayoutError, match=r"`float \*C`.*share memory"):
        call("l3d_bmm_f32", a, st4(a), b, st4(b), wide, st4(wide), *tail)
    assert reached == ["l3d_bmm_f32"]


@pytest.mark.parametrize("name", ["l3d_attention_forward_strided", "l3d_attention_forward_f16b"])
def test_attention_batch_strides(audited, name):
    call, reached = audited
    B, H, D, N, M = 2, 2, 32, 16, 24
    qkv = torch.zeros(B, 3 * H * D, N)                                    # q of a fused q|k|v projection
    kv = torch.zeros(B, 2 * H * D, M)
    q, k, v = qkv[:, :H * D], kv[:, :H * D], kv[:, H * D:]
    ctx = torch.zeros(B, H * D, N)

    def args(q, k, v, qs, ks, vs):
        head = (q, k, v, B, H, D, N, M, qs, ks, vs, 0.125)
        return head + ((ctx,) if name.endswith("strided") else (torch.zeros(16, dtype=torch.uint8), 0, ctx, None))
    call(name, *args(q, k, v, q.stride(0), k.stride(0), v.stride(0)))
    assert reached == [name]
    for i, p in enumerate("qkv"):
        wrong = [q.stride(0), k.stride(0), v.stride(0)]
        wrong[i] = H * D * (N if i == 0 else M)                           # the stride of a tensor of its own
        with pytest.raises(LayoutError, match=rf"`const float \*{p}`.*`{p}_bstride` passes {wrong[i]}"):
            call(name, *args(q, k, v, *wrong))
    qt = torch.zeros(B, N, H * D).transpose(1, 2)                        # the batch stride is right, the rest is not dense
    with pytest.raises(LayoutError, match=r"`const float \*q`.*strides \(1024, 1, 64\).*must be dense"):
        call(name, *args(qt, k, v, qt.stride(0), k.stride(0), v.stride(0)))
    with pytest.raises(LayoutError, match=r"`float \*ctx`.*not contiguous"):
        call(name, *args(q, k, v, q.stride(0), k.stride(0), v.stride(0))[:-2 if name.endswith("f16b") else -1],
             *((torch.zeros(B, N, H * D).transpose(1, 2),) + ((None,) if name.endswith("f16b") else ())))
    assert reached == [name]


def test_row_strides(audited):
    call, reached = audited
    x = torch.zeros(8, 32)[:, :16]
    img, ws, out = torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8), torch.zeros(16)
    call("l3d_split_f16_operand", x, 8, 16, x.stride(0), 1, img, None)
    call("l3d_colsum_rows", x, 8, 16, x.stride(0), ws, out)
    assert reached == ["l3d_split_f16_operand", "l3d_colsum_rows"]
    with pytest.raises(LayoutError, match=r"l3d_split_f16_operand.*`const float \*x`.*strides \(32, 1\), but `row_stride` passes 16"):
        call("l3d_split_f16_operand", x, 8, 16, 16, 1, img, None)
    with pytest.raises(LayoutError, match=r"l3d_colsum_rows.*`const float \*x`.*`row_stride` passes 16"):
        call("l3d_colsum_rows", x, 8, 16, 16, ws, out)
    xt = torch.zeros(16, 8).t()
    with pytest.raises(LayoutError, match=r"l3d_split_f16_operand.*strides \(1, 8\).*dense rows"):
        call("l3d_split_f16_operand", xt, 8, 16, xt.stride(0), 1, img, None)
    xe = torch.zeros(1, 16).expand(8, 16)
    with pytest.raises(LayoutError, match=r"l3d_colsum_rows.*strides \(0, 1\).*dense rows"):
        call("l3d_colsum_rows", xe, 8, 16, xe.stride(0), ws, out)
    assert len(reached) == 2


def test_edge_gather_max_output_slice(audited):
    call, reached = audited
    B, Cout, N, k = 2, 8, 16, 4
    pq, idx = torch.zeros(B, 2 * Cout, N), torch.zeros((B, N, k), dtype=torch.int64)
    out = torch.zeros(B, 32, N)[:, 8:8 + Cout]
    call("l3d_edge_gather_max", pq, idx, B, Cout, N, k, 0, out, out.stride(0))
    assert reached == ["l3d_edge_gather_max"]
    with pytest.raises(LayoutError, match=r"`float \*out`.*strides \(512, 16, 1\), but `out_bstride` passes 128"):
        call("l3d_edge_gather_max", pq, idx, B, Cout, N, k, 0, out, Cout * N)
    with pytest.raises(LayoutError, match=r"`const float \*pq`.*not contiguous"):
        call("l3d_edge_gather_max", torch.zeros(B, 4 * Cout, N)[:, :2 * Cout], idx, B, Cout, N, k, 0, out, out.stride(0))
    shared = torch.zeros(1, Cout, N).expand(B, Cout, N)
    with pytest.raises(LayoutError, match=r"`float \*out`.*share memory"):
        call("l3d_edge_gather_max", pq, idx, B, Cout, N, k, 0, shared, 0)
    assert reached == ["l3d_edge_gather_max"]


def test_shift_step_inside_a_dense_tensor(audited):
    call, reached = audited
    x, w, y = torch.zeros(2, 4, 16), torch.zeros(8, 4), torch.zeros(2, 8, 16)

    def conv(shift, step):
        call("l3d_pointwise_conv", x, 0, w, None, shift, step, 2, 4, 8, 16, 0, 0, y)
    conv(torch.zeros(2, 8), 8)
    conv(torch.zeros(8), 0)
    assert reached == ["l3d_pointwise_conv"] * 2
    with pytest.raises(LayoutError, match=r"`shift_bstride` is 4, neither 0 nor Cout = 8"):
        conv(torch.zeros(2, 8), 4)
    with pytest.raises(LayoutError, match=r"`const float \*shift`.*strides \(0, 1\).*not contiguous"):
        conv(torch.zeros(1, 8).expand(2, 8), 8)
    assert len(reached) == 2


@pytest.fixture
def call_restored_afterwards():
    """set up before `monkeypatch`, so torn down after it: what follows the yield sees the state pytest leaves behind"""
    from learning3d_amd import _lib
    original, patched = _lib.call, []
    yield patched
    assert patched and _lib.call is original and not hasattr(_lib.call, "checked")
    assert all(m.call is original for m in patched), "a module kept the audit's wrapper after the test"


def test_install_is_undone_at_teardown(call_restored_afterwards, monkeypatch):
    from learning3d_amd import _lib
    original = _lib.call
    call = layout_audit.install(monkeypatch)
    holders = [m for m in layout_audit.package_modules() if "call" in m.__dict__]
    assert _lib in holders and len(holders) >= 15 and all(m.call is call for m in holders) and call.original is original
    call_restored_afterwards.extend(holders)


def test_install_patches_every_module_and_restores_them():
    from learning3d_amd import _lib
    original = _lib.call
    with pytest.MonkeyPatch.context() as mp:
        call = layout_audit.install(mp)
        holders = [m for m in layout_audit.package_modules() if "call" in m.__dict__]
        assert _lib.call is call and call.original is original
        assert len(holders) >= 15 and all(m.call is call for m in holders)
    assert _lib.call is original and all(m.call is original for m in holders)
