"""CPU model of the pooled layers' index division (train.hip, tr_grad_in and the two VEC loops; no GPU).

A layer whose output is also max-pooled over runs of K consecutive positions finds the run of position p as
    n = (long)(((float)p + 0.5f) * (1.0f / (float)K))
instead of an integer division.  The kernels' comment calls that exact for every K <= 256 and p < 2^22; l3d_bn_backward_stats /
l3d_bn_act_backward require P < 2^22 and _ConvAffineAct raises past it.  Replayed here in numpy float32: the library is built
without contraction and without fast-math, so (float)p (exact below 2^24), the add (exact below 2^23), the correctly rounded
1.0f / K and the one rounded product are the same four operations on the device.

For a fixed K the product is non-decreasing in p, so its floor is: if it equals n at the first position n K of a run and at the last
one, n K + K - 1, it equals n on the whole run.  Checking both ends of every run below 2^22 is therefore checking every p."""
import numpy as np

LIMIT = 1 << 22


def pool_run(p, K):
    """the kernels' p / K in float32, for an int64 array p"""
    kinv = np.float32(1.0) / np.float32(K)
    return ((p.astype(np.float32) + np.float32(0.5)) * kinv).astype(np.int64)


def test_float_division_is_exact_at_every_run_boundary_below_2_to_the_22():
    for K in range(1, 257):
        first = np.arange(0, LIMIT, K, dtype=np.int64)                   # p = n K
        last = first + (K - 1)                                           # p = n K + K - 1 = (n + 1) K - 1
        last = last[last < LIMIT]
        assert np.array_equal(pool_run(first, K), first // K), K
        assert np.array_equal(pool_run(last, K), last // K), K
        assert int(pool_run(np.array([LIMIT - 1], np.int64), K)[0]) == (LIMIT - 1) // K       # the last position the kernels admit


def test_float_division_fails_first_at_4243964_over_255():
    """the limit the P < 2^22 guards stand for: the first wrong quotient past it"""
    p, K = 4243964, 255
    assert int(pool_run(np.array([p], np.int64), K)[0]) != p // K
    below = np.arange(LIMIT, p, dtype=np.int64)
    for k in range(1, 257):
        assert np.array_equal(pool_run(below, k), below // k), k         # nothing fails between 2^22 and that position
