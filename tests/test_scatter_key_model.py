"""CPU models of l3d_scatter_add_det's size limit (scatter_det.hip; no GPU): the deterministic backward of grouping / gather /
three_interpolate / index_points / get_graph_feature.

* The placement kernel sorts 32-bit words (target << 10 | lane) of a 1024-entry chunk with 0xFFFFFFFF as the padding of lanes past
  the range's end.  For every (T, ranges) the guard admits, no valid word may reach that sentinel (or overflow 32 bits): an entry
  that sorts as padding is counted but never placed, and its target's sum reads an unwritten workspace slot.
* Past the guard, pointnet2_utils._scatter_add_det splits the targets into windows with one spare target each.  Driven here
  through the real Python helper with a float32 numpy stand-in for the kernel call, the windowed sums equal one ascending-entry
  pass (np.add.at on float32 applies its entries in order: the header's contract) bit for bit."""
import numpy as np
import pytest
import torch

SENTINEL = 0xFFFFFFFF


def _divup(a, b):
    return -(-a // b)


def _largest_admitted_T(E):
    from learning3d_amd.utils.pointnet2_utils import _sd_fits
    lo, hi = 1, 1 << 24                                         # bisection on the guard the wrapper and the kernel share
    assert _sd_fits(1, lo, E) and not _sd_fits(1, hi, E)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _sd_fits(1, mid, E) else (lo, mid)
    return lo


@pytest.mark.parametrize("E", [1, 1000, 1024, 1025, 2048, 3072, 3073, 4096, 7168, 7169, 8192, 65536])   # every range class and its edges
def test_placement_words_never_reach_the_padding_sentinel(E):
    from learning3d_amd.utils.pointnet2_utils import _sd_ranges
    T = _largest_admitted_T(E)
    R = _sd_ranges(E)
    assert T * R < (1 << 22) <= (T + 1) * R                     # the guard's boundary, as scatter_det.hip states it
    assert R == (1 if E <= 1024 else 2 if E <= 3072 else 4 if E <= 7168 else 8)   # scatter_det.hip's sd_ranges, restated
    # and the library refuses one target more, before any launch (fake pointers: nothing is read)
    import ctypes
    from learning3d_amd import _lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert _lib.lib().l3d_scatter_add_det(p, p, None, 1, 2, T + 1, E, 1, p, p, None) == -2
    rlen = _divup(_divup(E, R), 1024) * 1024                    # a range: whole 1024-entry chunks (the kernel's rlen)
    lanes = np.arange(min(1024, rlen), dtype=np.uint64)
    targets = np.array([0, T // 2, T - 2, T - 1], dtype=np.uint64)[-min(T, 4):]
    words = (targets[:, None] << np.uint64(10)) | lanes[None, :]           # the kernel's (uint32)target << 10 | lane, unwrapped
    assert int(words.max()) < SENTINEL, (E, T, hex(int(words.max())))
    # the sort sees distinct words, padding strictly last
    w32 = words.astype(np.uint32)
    assert np.array_equal(w32.astype(np.uint64), words)
    assert len(np.unique(w32)) == w32.size


def test_the_old_guard_admitted_a_colliding_word():
    """what the CPU model catches: T * R > 2^22 let T = 2^22, R = 1 through, and there target 2^22 - 1 at lane 1023 is 0xFFFFFFFF"""
    from learning3d_amd.utils.pointnet2_utils import _sd_fits
    T = 1 << 22
    assert ((T - 1) << 10) | 1023 == SENTINEL
    assert not _sd_fits(1, T, 1024)


def _kernel_model(calls):
    """numpy stand-in for one l3d_scatter_add_det call: only shapes the guard admits, indices already in [0, T)"""
    from learning3d_amd.utils.pointnet2_utils import _sd_fits

    def call(src, idx, weight, T, div, dst):
        B, Cc = src.shape[0], src.shape[1]
        E = idx.numel() // B
        assert _sd_fits(B, T, E), (B, T, E)
        ix = idx.reshape(B, E).numpy()
        assert ix.min() >= 0 and ix.max() < T and idx.dtype == torch.int32
        calls.append(T)
        s, w = src.numpy(), None if weight is None else weight.reshape(B, E).numpy()
        out = np.zeros((B, Cc, T), np.float32)
        e = np.arange(E)
        for b in range(B):
            for c in range(Cc):
                v = s[b, c, e // div] if w is None else (s[b, c, e // div] * w[b]).astype(np.float32)
                np.add.at(out[b, c], ix[b], v)
        dst.copy_(torch.from_numpy(out))
    return call


@pytest.mark.parametrize("T,E,div,weighted", [(1 << 22, 1024, 1, False), (524289, 8192, 1, False), (524288, 8193, 3, True),
                                              (1000, 4096, 1, False)])
def test_windowed_scatter_equals_one_ascending_pass(monkeypatch, T, E, div, weighted):
    from learning3d_amd.utils import pointnet2_utils as P
    calls = []
    monkeypatch.setattr(P, "_scatter_add_det_call", _kernel_model(calls))
    rng = np.random.default_rng(T + E)
    B, Cc = 1, 2
    idx = rng.integers(0, T, (B, E)).astype(np.int32)
    idx[0, -1] = T - 1                                          # the last lane of the last chunk on the last target
    idx[0, rng.integers(0, E, 5)] = T - 1
    idx[0, :3] = 0
    src = rng.standard_normal((B, Cc, E // div)).astype(np.float32)
    w = rng.uniform(0, 1, (B, E // div, div)).astype(np.float32) if weighted else None
    got = P._scatter_add_det(torch.from_numpy(src), torch.from_numpy(idx), None if w is None else torch.from_numpy(w), T, div)
    want = np.zeros((B, Cc, T), np.float32)
    e = np.arange(E)
    for c in range(Cc):
        v = src[0, c, e // div] if w is None else (src[0, c, e // div] * w.reshape(B, E)[0]).astype(np.float32)
        np.add.at(want[0, c], idx[0], v)
    assert got.shape == (B, Cc, T)
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    assert len(calls) == (1 if P._sd_fits(B, T, E) else 2), calls
