"""What the tests of RPMNet's matching stage on HIP share (tests/test_rpmnet_match_cpu.py, tests/test_gpu_rpmnet_match.py):

  * forward64 / backward64 / fold64: the slack Sinkhorn with its potentials, the reverse sweep from them and the fold through
    log_alpha = -beta (dist - alpha), exactly as include/ext/l3d_rpmnet_match.h states them, in plain torch and fp64.  The CPU test
    holds them to torch.autograd through the package's own op sequence (autograd64); the GPU test holds the kernels to them.
  * match_case: dist, beta, alpha, xyz_ref and the four cotangents, with the affinity reaching +-amax.
  * reordered64: backward64 with every sum taken in another order -- the distance between two fp64 evaluations of the same formulas,
    the unit of a floor under the rounded-once bar; backward64(terms=True): the sum of the absolute terms behind every element.

Everything here is this project's own statement of the formulas; nothing is taken from another code base."""
import torch

EPS = 1e-5
TIER = 1e-5
COTANGENTS = ("d_perm", "d_rowsum", "d_weighted", "d_affinity")


def match_case(seed, B, J, K, amax=200.0, both_signs=False, dev="cpu"):
    """-> dict: dist [B,J,K] in [0, 4] (squared distances of unit features), beta, alpha [B], xyz_ref [B,K,3], and a cotangent for each
    of the four outputs, all fp32.  Most pairs lie near alpha: an affinity -beta (dist - alpha) of a few units, comparable with the
    slack's 0, so that every output depends on every input.  One pair in ten is far: beyond alpha, its affinity reaching -amax.
    both_signs: the far pairs lie on either side and the affinity reaches +-amax.  A row with an entry near +amax gives the slack
    exp(-amax) of its mass: d_alpha and much of d_log_alpha are then sums that cancel to rounding noise, and only a bar that knows
    the size of the terms (reordered64) can hold them."""
    g = torch.Generator().manual_seed(seed)
    dist = (2.0 + 0.04 * torch.randn((B, J, K), generator=g)).clamp_(0.0, 4.0)
    far = torch.rand((B, J, K), generator=g) < 0.1
    where = torch.rand((B, J, K), generator=g) * (4.0 if both_signs else 2.0) + (0.0 if both_signs else 2.0)
    dist = torch.where(far, where, dist)
    beta = (amax / 2.0) * (0.8 + 0.4 * torch.rand((B,), generator=g))
    alpha = 2.0 * (0.99 + 0.02 * torch.rand((B,), generator=g))
    case = {"dist": dist, "beta": beta, "alpha": alpha, "xyz_ref": torch.rand((B, K, 3), generator=g) * 2 - 1,
            "d_perm": torch.randn((B, J, K), generator=g), "d_rowsum": torch.randn((B, J), generator=g),
            "d_weighted": torch.randn((B, J, 3), generator=g), "d_affinity": torch.randn((B, J, K), generator=g)}
    return {n: t.to(dev) for n, t in case.items()}


def affinity32(case):
    """the fp32 affinity as RPMNet.compute_affinity forms it"""
    return -case["beta"][:, None, None] * (case["dist"] - case["alpha"][:, None, None])


def forward64(A, n_iters, xyz_ref=None, eps=EPS):
    """A [B,J,K] -> (potentials fp64 [n,B,J+K]: u_t then v_t, P [B,J,K], r [B,J], w [B,J,3] or None)"""
    A = A.double()
    B, J, K = A.shape
    zc, zr = A.new_zeros(B, J, 1), A.new_zeros(B, 1, K)
    v = A.new_zeros(B, K)
    u = A.new_zeros(B, J)
    pots = []
    for _ in range(n_iters):
        u = torch.logsumexp(torch.cat([A - v[:, None, :], zc], 2), dim=2)        # the slack column: A = 0, v = 0
        v = torch.logsumexp(torch.cat([A - u[:, :, None], zr], 1), dim=1)        # the slack row: A = 0, u = 0
        pots.append(torch.cat([u, v], 1))
    P = torch.exp(A - u[:, :, None] - v[:, None, :])
    r = P.sum(2)
    w = None if xyz_ref is None else (P @ xyz_ref.double()) / (r[:, :, None] + eps)
    return (torch.stack(pots) if pots else A.new_zeros(0, B, J + K)), P, r, w


def backward64(A, potentials, xyz_ref=None, eps=EPS, d_perm=None, d_rowsum=None, d_weighted=None, d_affinity=None, order=None,
               terms=False):
    """dA [B,J,K] fp64 from log_alpha A, the potentials [n,B,J+K] and whichever cotangents are given.
    order: None, or a function sum(t, dim) that replaces every torch.sum (reordered64); the three-term sums inside the exponentials
    are then associated the other way round too.
    terms: -> (dA, mag) with mag [B,J,K] the sum of the absolute values of the terms dA is the sum of: what an evaluation in fp64 can
    be accurate to is 2^-53 of mag, not of |dA| -- the terms of G alone cancel to eps / (r + eps) of their size in a row whose
    only cotangent is d_weighted"""
    S = order or (lambda t, dim: t.sum(dim))
    A = A.double()
    B, J, K = A.shape
    n = potentials.shape[0]
    pot = potentials.double()
    u = lambda t: pot[t - 1, :, :J]                                              # noqa: E731   u_t, t = 1..n
    v = lambda t: pot[t - 1, :, J:] if t >= 1 else A.new_zeros(B, K)             # noqa: E731   v_t, v_0 = 0
    un = u(n) if n else A.new_zeros(B, J)
    # the three-term sums in the exponents: (A - row) - column as written, and with `order` the other association
    ex = (lambda row, col: torch.exp((A - col[:, None, :]) - row[:, :, None])) if order else \
        (lambda row, col: torch.exp((A - row[:, :, None]) - col[:, None, :]))
    ex_r = (lambda row, col: torch.exp((A - row[:, :, None]) - col[:, None, :])) if order else \
        (lambda row, col: torch.exp((A - col[:, None, :]) - row[:, :, None]))
    P = ex(un, v(n))
    r = S(P, 2)
    inner, c0 = A.new_zeros(B, J, K), A.new_zeros(B, J)
    inner_mag = A.new_zeros(B, J, K)
    if d_weighted is not None:
        x = xyz_ref.double()
        Px = torch.stack([S(P * x[:, None, :, c], 2) for c in range(3)], -1)
        g = d_weighted.double() / (r[:, :, None] + eps)
        w = Px / (r[:, :, None] + eps)
        c0 = -((g[..., 0] * w[..., 0] + g[..., 1] * w[..., 1]) + g[..., 2] * w[..., 2])
        gx = (g[:, :, None, 0] * x[:, None, :, 0] + g[:, :, None, 1] * x[:, None, :, 1]) + g[:, :, None, 2] * x[:, None, :, 2]
        inner = inner + gx
        inner_mag = inner_mag + gx.abs() + c0.abs()[:, :, None]
    if d_rowsum is not None:
        c0 = c0 + d_rowsum.double()
        inner_mag = inner_mag + d_rowsum.double().abs()[:, :, None]
    inner = c0[:, :, None] + inner
    if d_perm is not None:
        inner = inner + d_perm.double()
        inner_mag = inner_mag + d_perm.double().abs()
    G = P * inner
    dA, mag = G.clone(), P * inner_mag
    if d_affinity is not None:
        dA = d_affinity.double() + dA
        mag = mag + d_affinity.double().abs()
    ubar_n, vbar = -S(G, 2), -S(G, 1)
    for t in range(n, 0, -1):
        Q = ex(u(t), v(t))
        ubar = -S(vbar[:, None, :] * Q, 2)
        if t == n:
            ubar = ubar_n + ubar
        R = ex_r(u(t), v(t - 1))
        dA = dA + (vbar[:, None, :] * Q + ubar[:, :, None] * R)
        mag = mag + (vbar.abs()[:, None, :] * Q + ubar.abs()[:, :, None] * R)
        vbar = -S(ubar[:, :, None] * R, 1)
    return (dA, mag) if terms else dA


def fold64(dA, dist, beta, alpha, order=None):
    """-> (dD [B,J,K], dbeta [B], dalpha [B]) of log_alpha = -beta (dist - alpha) per cloud, fp64"""
    S = order or (lambda t, dim: t.sum(dim))
    b, a = beta.double(), alpha.double()
    B = dA.shape[0]
    dD = -b[:, None, None] * dA
    dbeta = -S((dA * (dist.double() - a[:, None, None])).reshape(B, -1), 1)
    dalpha = b * S(dA.reshape(B, -1), 1)
    return dD, dbeta, dalpha


def fold_terms64(mag, dist, beta, alpha):
    """the sums of absolute terms behind fold64's three outputs, from backward64's mag"""
    b, a = beta.double(), alpha.double()
    B = mag.shape[0]
    return b[:, None, None] * mag, (mag * (dist.double() - a[:, None, None]).abs()).reshape(B, -1).sum(1), b * mag.reshape(B, -1).sum(1)


def _reversed_sum(t, dim):
    """the same terms added from the far end, pairwise by torch"""
    return t.flip(dim).cumsum(dim).select(dim, -1)


def reordered64(*args, **kw):
    """backward64 with every sum taken as a running sum from the far end"""
    return backward64(*args, order=_reversed_sum, **kw)


def reordered_fold64(*args):
    return fold64(*args, order=_reversed_sum)


def autograd64(case, n_iters, given, fold=True, eps=EPS):
    """The same gradients from torch.autograd in fp64 through the package's own op sequence: RPMNet.compute_affinity -> sinkhorn ->
    exp -> sum -> weighted template.  given: the names of the cotangents that arrive.
    fold: -> (dD, dbeta, dalpha); else the gradient at the fp32 affinity taken as the leaf -> dA"""
    from learning3d_amd.models import rpmnet
    net = rpmnet.RPMNet.__new__(rpmnet.RPMNet)                                   # compute_affinity reads no state
    x = case["xyz_ref"].double()
    if fold:
        leaves = [case[n].double().clone().requires_grad_() for n in ("dist", "beta", "alpha")]
        A = rpmnet.RPMNet.compute_affinity(net, leaves[1], leaves[0], alpha=leaves[2])
    else:
        leaves = [affinity32(case).double().clone().requires_grad_()]
        A = leaves[0]
    perm = torch.exp(rpmnet.sinkhorn(A, n_iters=n_iters, slack=True))
    rowsum = torch.sum(perm, dim=2)
    weighted = perm @ x / (torch.sum(perm, dim=2, keepdim=True) + eps)
    outs = {"d_perm": perm, "d_rowsum": rowsum, "d_weighted": weighted, "d_affinity": A}
    loss = sum((outs[n] * case[n].double()).sum() for n in given)
    return torch.autograd.grad(loss, leaves)
