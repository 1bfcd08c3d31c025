"""knn_mfma.hip at the edges of its tiling (64 queries per workgroup, 128 candidates per tile pair, 256 <= N <= 2048) against
the insertion kernel (knn.hip, variant 1), index for index -- including clouds whose duplicated points overflow the 64-key
candidate lists and take the tighter-bound and exact-tie paths."""
import numpy as np
import pytest
import torch

DEVICE = "cuda:0"


def _knn(x, k, variant):
    from learning3d_amd._lib import check, lib, ptr, stream_ptr
    B, N, _ = x.shape
    idx = torch.full((B, N, k), -7, dtype=torch.int64, device=x.device)
    check(lib().l3d_knn_graph_variant(ptr(x), B, N, k, ptr(idx), variant, stream_ptr()), "l3d_knn_graph_variant")
    return idx.cpu().numpy()


def _clouds(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, N, 3), generator=g)
    for b in range(0, B, 2):                                 # every other cloud: a run of 100 copies of one point and a
        lo = (37 * b) % (N - 200)                            # clump of 80 near-duplicates -- both overflow a 64-key list
        x[b, lo:lo + 100] = x[b, N - 1]
        x[b, lo + 100:lo + 180] = x[b, 0] + 1e-6 * torch.rand((80, 3), generator=g)
    return x.to(DEVICE).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 32])
@pytest.mark.parametrize("N", [256, 257, 1000, 1023, 1024, 1025, 2048])
def test_knn_mfma_tiling_edges_equal_insertion_kernel(B, N):
    x = _clouds(B, N, 1000 * B + N)
    for k in (1, 20, 24):
        a = _knn(x, k, 2)
        b = _knn(x, k, 1)
        assert (a >= 0).all() and (a < N).all(), f"k={k}: an index was left unwritten"
        assert np.array_equal(a, b), f"k={k}: {np.argwhere(a != b)[:5]}"
