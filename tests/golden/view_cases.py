"""Shared by the tests that hand ops, backward functions and models non-contiguous views (test_gpu_views_*.py): the view kinds, the
bitwise comparison, and run_on_views(), which runs one callable on a view and on the view's contiguous clone under the launch audit.

A correct wrapper hands its kernel the same bytes at an allocator-aligned address whichever way the caller's tensor lies, so the
two runs must agree in every bit, launch the same entry points, and leave the caller's memory -- the elements a view skips
included -- as it was."""
import torch

JUNK = 777.0             # what the elements a view skips hold: large enough to wreck any result that reads them


def leaves(out, path="out"):
    """[(path, tensor)] of a tensor | None | tuple / list / dict of those"""
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [(path, out)]
    if isinstance(out, (bool, int, float)):
        return [(path, torch.tensor(out))]
    if isinstance(out, dict):
        return [l for k in out for l in leaves(out[k], f"{path}[{k!r}]")]
    if isinstance(out, (tuple, list)):
        return [l for i, o in enumerate(out) for l in leaves(o, f"{path}[{i}]")]
    raise TypeError(f"{path}: {type(out)}")


def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def assert_identical(got, want, what, strides=True):
    got, want = leaves(got), leaves(want)
    assert [p for p, _ in got] == [p for p, _ in want], f"{what}: results of different structure"
    for (path, a), (_, b) in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {path} is {a.dtype} {tuple(a.shape)}, expected {b.dtype} {tuple(b.shape)}"
        if strides:
            assert a.stride() == b.stride(), f"{what}: {path} has strides {a.stride()}, expected {b.stride()}"
        if not torch.equal(bits(a), bits(b)):
            differ = int((a.detach() != b.detach()).sum())
            raise AssertionError(f"{what}: {path} differs in {differ} of {a.numel()} elements")


def whole_storage(t):
    """every byte of the buffer t is a view of"""
    s = t.untyped_storage()
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(s, 0, (s.nbytes(),), (1,))


def float_views(t, kinds=("transposed", "channels", "rows", "expand")):
    """[(kind, view)] of a contiguous float tensor t [B, ...]: non-contiguous views of t's shape.  All but `expand` hold t's values."""
    out = []
    for kind in kinds:
        if kind == "transposed" and t.dim() >= 2:          # a buffer stored in the other order
            v = t.transpose(-1, -2).contiguous().transpose(-1, -2)
        elif kind == "channels":                         # wide[..., :c] of a buffer with twice the channels
            wide = torch.full(t.shape[:-1] + (2 * t.shape[-1],), JUNK, dtype=t.dtype, device=t.device)
            wide[..., :t.shape[-1]] = t
            v = wide[..., :t.shape[-1]]
        elif kind == "rows" and t.dim() >= 2:              # wide[:, 1:1 + n]: non-dense across the batch, with a storage offset
            wide = torch.full((t.shape[0], t.shape[1] + 2) + t.shape[2:], JUNK, dtype=t.dtype, device=t.device)
            wide[:, 1:1 + t.shape[1]] = t
            v = wide[:, 1:1 + t.shape[1]]
        elif kind == "expand" and t.shape[0] > 1:          # one cloud for the whole batch, stride 0
            v = t[:1].clone().expand(t.shape)
        else:
            continue
        if not v.is_contiguous():                          # (a [B, 1, n] tensor has no transposed view worth the name)
            assert v.shape == t.shape
            out.append((kind, v))
    return out


def index_views(t):
    """[(kind, view)] of a contiguous integer tensor: a transposed and a stride-2 view holding t's values"""
    out = []
    if t.dim() >= 2:
        out.append(("transposed", t.transpose(-1, -2).contiguous().transpose(-1, -2)))
    wide = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    wide[..., ::2] = t
    out.append(("stride2", wide[..., ::2]))
    return [(k, v) for k, v in out if not v.is_contiguous()]


def grad_views(shape, seed, device="cuda"):
    """[(kind, g)] gradients of `shape` as autograd hands them on unchanged: a transposed view, a stride-2 slice, and a stride-0
    expand of a tensor with ones for the first and the last dimension ([1, C, 1]-like)"""
    gen = torch.Generator().manual_seed(seed)
    shape = tuple(shape)
    out = []
    if len(shape) >= 2:
        swapped = shape[:-2] + (shape[-1], shape[-2])
        out.append(("transposed", torch.randn(swapped, generator=gen).to(device).transpose(-1, -2)))
    out.append(("stride2", torch.randn(shape[:-1] + (2 * shape[-1],), generator=gen).to(device)[..., ::2]))
    small = (1,) + shape[1:-1] + ((1,) if len(shape) >= 2 else ())
    out.append(("expand", torch.randn(small, generator=gen).to(device).expand(shape)))
    return [(k, g) for k, g in out if not g.is_contiguous()]


def logged(fn, *args):
    """-> (fn(*args), the names of the C-ABI calls it made)"""
    from learning3d_amd import _lib
    assert _lib.LAUNCH_LOG is None
    _lib.LAUNCH_LOG = log = []
    try:
        out = fn(*args)
    finally:
        _lib.LAUNCH_LOG = None
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return out, log


def has_entry(log, entry):
    return any(name == entry or name.startswith(entry + "[") for name in log)


def run_on_views(fn, args, views, entries, what, strides=True, compare=assert_identical, nondeterministic=False):
    """fn(*args) with args[i] replaced by each view of `views` = {i: [(kind, view)]} in turn, against the same call on the view's
    contiguous clone.  entries: the entry points the call must launch (on both sides: the logs must be equal)."""
    assert views and all(views.values()), f"{what}: no views to test"
    for i, kinds in views.items():
        for kind, v in kinds:
            case = f"{what}, argument {i} as a {kind} view {tuple(v.shape)} / {v.stride()}"
            assert not v.is_contiguous()
            dense = v.clone(memory_format=torch.contiguous_format)
            assert dense.is_contiguous() and dense.data_ptr() % 16 == 0
            on_dense = [dense if j == i else a for j, a in enumerate(args)]
            on_view = [v if j == i else a for j, a in enumerate(args)]
            fn(*on_dense)                                  # (the first call fills the caches of weight images: not compared)
            want, log = logged(fn, *on_dense)
            again, log2 = logged(fn, *on_dense)
            for e in entries:
                assert has_entry(log, e), f"{case}: the contiguous run did not launch {e}: {log}"
            assert log2 == log, f"{case}: two contiguous runs launched {log} and {log2}"
            if not nondeterministic:
                compare(again, want, case + ": two runs on the SAME contiguous input (determinism precondition)", True)
            before = whole_storage(v).clone()
            got, vlog = logged(fn, *on_view)
            assert vlog == log, f"{case}: launched {vlog}, on the contiguous clone {log}"
            compare(got, want, case, strides)
            assert torch.equal(whole_storage(v), before), f"{case}: the caller's buffer was written to"
