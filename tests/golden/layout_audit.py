"""An audit of the launch boundary: `_lib.call` hands `tensor.data_ptr()` to a kernel and never looks at strides, so whether the
kernel reads the memory the caller meant is decided at each call site.  install() puts a wrapper in front of `call` -- in `_lib`
and in every loaded learning3d_amd module that imported the name -- which inspects every tensor argument BEFORE anything is
launched and raises LayoutError for a tensor the entry point cannot read as it lies.  No kernel runs on a refused tensor.

A tensor must be `is_contiguous()`, except for the parameters whose header declares a stride for them (STRIDED, keyed by entry point
and header parameter, never by a Python call site).  For those the stride passed must be the tensor's own and every dimension the
kernel treats as dense must be dense.  Every header parameter with `stride` in its name is listed, in STRIDED or in DENSE_STEPS: an
entry point that gains one without an entry here is refused (uncovered_stride_parameters), not waved through.

Not seen by the audit: what reaches the library as a ctypes value (`_lib.ptr(t)`, the pointer arrays of l3d_edgeconv_pack)."""
import sys
from collections import namedtuple

import torch


class LayoutError(Exception):
    """a tensor argument of a C-ABI call is laid out in a way the entry point does not read"""


# how a parameter with a declared stride is read.  stride: the header parameter that carries it; dims: the tensor's shape as the
# entry point's integer parameters (a tuple of names: their product); kind:
#   "strides4": the stride parameter is a host array of the four element strides of a 4-d tensor; no dimension need be dense
#   "batch":    the stride parameter is the step between clouds; the dimensions behind the first are dense
#   "rows":     the stride parameter is the step between the rows of a 2-d tensor; a row is dense and rows do not overlap
# written: the kernel writes it, so no two of its elements may share memory.
Strided = namedtuple("Strided", "stride kind dims written")

STRIDED = {
    # l3d_hip.h: `const long *a_strides, b_strides, c_strides`: "four element strides {batch1, batch2, row, column} (host arrays)"
    ("l3d_bmm_f32", "A"): Strided("a_strides", "strides4", ("nb1", "nb2", "M", "K"), False),
    ("l3d_bmm_f32", "B"): Strided("b_strides", "strides4", ("nb1", "nb2", "K", "N"), False),
    ("l3d_bmm_f32", "C"): Strided("c_strides", "strides4", ("nb1", "nb2", "M", "N"), True),
    # ... and the host-only query that takes the same operands (it reads the pointers' alignment and the strides, no memory)
    ("l3d_bmm_f32_route", "A"): Strided("a_strides", "strides4", ("nb1", "nb2", "M", "K"), False),
    ("l3d_bmm_f32_route", "B"): Strided("b_strides", "strides4", ("nb1", "nb2", "K", "N"), False),
    # l3d_hip.h: `long q_bstride, k_bstride, v_bstride`: "explicit batch strides (in floats) for q, k, v: channel slices of ONE fused
    # projection output [B, 3*H*D, N]"
    ("l3d_attention_forward_strided", "q"): Strided("q_bstride", "batch", ("B", ("H", "D"), "N"), False),
    ("l3d_attention_forward_strided", "k"): Strided("k_bstride", "batch", ("B", ("H", "D"), "M"), False),
    ("l3d_attention_forward_strided", "v"): Strided("v_bstride", "batch", ("B", ("H", "D"), "M"), False),
    ("l3d_attention_forward_f16b", "q"): Strided("q_bstride", "batch", ("B", ("H", "D"), "N"), False),
    ("l3d_attention_forward_f16b", "k"): Strided("k_bstride", "batch", ("B", ("H", "D"), "M"), False),
    ("l3d_attention_forward_f16b", "v"): Strided("v_bstride", "batch", ("B", ("H", "D"), "M"), False),
    # l3d_hip.h: `long row_stride`: "x [rows][C] fp32 with row stride `row_stride`"
    ("l3d_split_f16_operand", "x"): Strided("row_stride", "rows", ("rows", "C"), False),
    # l3d_hip.h: `long row_stride`: "out[c] = sum_r x[r row_stride + c]"
    ("l3d_colsum_rows", "x"): Strided("row_stride", "rows", ("rows", "cols"), False),
    # l3d_hip.h: `long out_bstride`: "out fp32 [B][Cout][N] with batch stride out_bstride floats (a slice of a concat buffer)"
    ("l3d_edge_gather_max", "out"): Strided("out_bstride", "batch", ("B", "Cout", "N"), True),
}

# `int shift_bstride` (l3d_hip.h: "shift is read at [b*shift_bstride + co]: 0 = one vector for the batch", else Cout) is a step inside a
# DENSE tensor, [Cout] or [B][Cout]: it exempts nothing, shift must be contiguous like any other tensor, and the step must be 0 or Cout.
DENSE_STEPS = {
    ("l3d_pointwise_conv", "shift_bstride"): ("shift", "Cout"),
    ("l3d_pointwise_conv_split", "shift_bstride"): ("shift", "Cout"),
    ("l3d_pointwise_conv_f16", "shift_bstride"): ("shift", "Cout"),
}


def uncovered_stride_parameters(prototypes):
    """[(entry point, parameter)] of every header parameter with `stride` in its name that neither table accounts for"""
    claimed = {(name, s.stride) for (name, _), s in STRIDED.items()} | set(DENSE_STEPS)
    return sorted((name, p.name) for name, proto in prototypes.items() for p in proto.params
                  if "stride" in p.name.lower() and (name, p.name) not in claimed)


def _describe(name, param, t):
    return f"{name}: parameter `{param.ctype}{'' if param.ctype.endswith('*') else ' '}{param.name}` got a tensor of shape " \
           f"{tuple(t.shape)} and strides {tuple(t.stride())}"


def _dense_from(t, first):
    """dimensions first.. of t lie as one dense row-major block (a dimension of size 1 has no stride to speak of)"""
    step = 1
    for d in range(t.dim() - 1, first - 1, -1):
        if t.shape[d] != 1 and t.stride(d) != step:
            return False
        step *= t.shape[d]
    return True


def _overlaps(t):
    """two elements of t share memory (sufficient test: sorted by stride, each dimension must step past the ones below it)"""
    dims = sorted((st, n) for st, n in zip(t.stride(), t.shape) if n > 1)
    reach = 0
    for st, n in dims:
        if st <= reach:
            return True
        reach += st * (n - 1)
    return False


def _host_values(value, n):
    """the first n values of a host array (a ctypes array, as the wrappers build it, or any sequence)"""
    return tuple(int(v) for v in value)[:n]


def _check_strided(name, proto, values, param, t, rule):
    say = _describe(name, param, t)
    shape = []
    for d in rule.dims:
        size = 1
        for n in (d if isinstance(d, tuple) else (d,)):
            size *= int(values[n])
        shape.append(size)
    if tuple(t.shape) != tuple(shape):
        raise LayoutError(f"{say}; the call's sizes {rule.dims} make it {tuple(shape)}")
    passed = values[rule.stride]
    if rule.kind == "strides4":
        passed = _host_values(passed, 4)
        if any(n > 1 and s != p for n, s, p in zip(t.shape, t.stride(), passed)):
            raise LayoutError(f"{say}, but `{rule.stride}` passes {passed}")
    elif rule.kind == "batch":
        if t.shape[0] > 1 and int(passed) != t.stride(0):
            raise LayoutError(f"{say}, but `{rule.stride}` passes {int(passed)}")
        if not _dense_from(t, 1):
            raise LayoutError(f"{say}: `{rule.stride}` covers the first dimension only, the others must be dense")
    else:
        if t.shape[0] > 1 and int(passed) != t.stride(0):
            raise LayoutError(f"{say}, but `{rule.stride}` passes {int(passed)}")
        if not _dense_from(t, 1) or (t.shape[0] > 1 and int(passed) < t.shape[1]):
            raise LayoutError(f"{say}: `{rule.stride}` takes dense rows that do not overlap")
    if rule.written and _overlaps(t):
        raise LayoutError(f"{say}: the kernel writes it, and elements of it share memory")


def check_call(lib, name, args):
    """raise LayoutError if l3d_<name>(*args) would hand a kernel a tensor it does not read as it lies; nothing is launched here"""
    proto = lib.PROTOTYPES.get(name)
    if proto is None or not (len(args) == len(proto.params) or len(args) + 1 == len(proto.params)):
        return                                           # `call` itself refuses these
    values = {p.name: a for p, a in zip(proto.params, args)}
    for p in proto.params:
        if "stride" in p.name.lower() and (name, p.name) not in DENSE_STEPS \
                and not any(k[0] == name and s.stride == p.name for k, s in STRIDED.items()):
            raise LayoutError(f"{name}: parameter `{p.ctype} {p.name}` declares a stride the layout audit has no rule for")
    for p, a in zip(proto.params, args):
        if not isinstance(a, torch.Tensor):
            continue
        rule = STRIDED.get((name, p.name))
        if rule is not None:
            _check_strided(name, proto, values, p, a, rule)
        elif not a.is_contiguous():
            raise LayoutError(f"{_describe(name, p, a)}: not contiguous, and the header declares no stride for it")
    for (entry, step), (tensor, full) in DENSE_STEPS.items():
        if entry == name and isinstance(values.get(tensor), torch.Tensor) and int(values[step]) not in (0, int(values[full])):
            raise LayoutError(f"{name}: `{step}` is {int(values[step])}, neither 0 nor {full} = {int(values[full])}")


def package_modules():
    return [m for n, m in sorted(sys.modules.items()) if m is not None and (n == "learning3d_amd" or n.startswith("learning3d_amd."))]


def install(monkeypatch, inner=None):
    """Replace `_lib.call`, and the name `call` in every loaded learning3d_amd module where it is `_lib.call`, by a wrapper that runs
    check_call and then `inner` (default: the real `call`).  monkeypatch restores all of them at teardown.  -> the wrapper; its
    `.checked` counts the calls it let through."""
    import glob
    import importlib
    import os
    import learning3d_amd
    from learning3d_amd import _lib
    top = os.path.dirname(os.path.abspath(learning3d_amd.__file__))
    for path in sorted(glob.glob(os.path.join(top, "**", "*.py"), recursive=True)):     # load every module now: one loaded later would
        rel = os.path.relpath(path, top)[:-3].replace(os.sep, ".")                      # import whatever `_lib.call` is at that time
        if rel != "build" and not rel.endswith("__init__"):
            importlib.import_module("learning3d_amd." + rel)
    original = _lib.call
    target = original if inner is None else inner

    def call(name, *args, **kw):
        check_call(_lib, name, args)
        call.checked += 1
        return target(name, *args, **kw)
    call.checked = 0
    call.original = original
    for mod in package_modules():
        if mod.__dict__.get("call") is original:
            monkeypatch.setattr(mod, "call", call)
    assert _lib.call is call
    return call
