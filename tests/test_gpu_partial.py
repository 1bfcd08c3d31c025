"""Partial / noisy registration pairs on the device: l3d_crop_select against the fp64 numpy model of its header
(golden/partial_fixture.py) and against the reference's own crops (tests/golden/partial_seeded.npz), the functions of
data_utils.partial from the recorded draws and from re-seeded np.random / torch, repeatability, the memory contract, graph replay,
the feed's invariants and two models fed end to end.  Everything is BIT-EXACT: the feature is a selection plus one fp32
multiplication and addition, so no test has a tolerance (the one bound, on the jitter, is the header's clip plus the rounding of
the addition, derived where it is used)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import memory_contract as mc     # noqa: E402
import partial_fixture as pf     # noqa: E402
from seeded import seeded_params    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAME = "l3d_crop_select"
CLIP = 0.05


def _mods():
    from learning3d_amd import _lib
    from learning3d_amd.data_utils import partial
    return _lib, partial


def _bits(a, b):
    """bit equality (a NaN equals the same NaN)"""
    a, b = a.detach().cpu().contiguous(), torch.as_tensor(b).contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(torch.uint8) == b.view(torch.uint8)).all())


def _operands(seed, B, N, C, mode, far=True):
    """seeded clouds in [-1,1]^3 (further columns ride along), the view points of farthest_subsample_points or unit normals, fp32 means"""
    g = np.random.default_rng(seed)
    pts = g.uniform(-1, 1, (B, N, C)).astype(np.float32)
    if mode == pf.NEAREST:
        vec = g.uniform(0, 1, (B, 3)) + (500.0 if far else 0.0) * g.choice([1.0, -1.0], (B, 1))
    else:
        vec = g.standard_normal((B, 3))
        vec /= np.linalg.norm(vec, axis=1, keepdims=True)
    centre = pts[:, :, :3].mean(axis=1, dtype=np.float32)
    return pts, vec, centre


def _launch(pts, vec, centre, mode, K, noise=None, sigma=None, clip=0.0, **want):
    """numpy / CPU operands -> the kernel's (idx, mask, out) on the device"""
    _, P = _mods()
    dev = lambda a, dt: None if a is None else torch.as_tensor(a).to(DEV, dt).contiguous()     # noqa: E731
    return P.crop_select(dev(pts, torch.float32), dev(vec, torch.float64), mode, K, centre=dev(centre, torch.float32),
                         noise=dev(noise, torch.float32), sigma=dev(sigma, torch.float32), clip=clip, **want)


def _hold_to_model(pts, vec, centre, mode, K, got, what=""):
    idx, mask, out = got
    want_idx, want_mask = pf.select_batch(pts, vec, centre, mode, K)
    assert np.array_equal(idx.cpu().numpy(), want_idx), what
    assert np.array_equal(mask.cpu().numpy(), want_mask), what
    assert _bits(out, torch.from_numpy(np.take_along_axis(pts, want_idx[:, :, None], axis=1))), what
    return want_idx


SHAPES = [(1, 1, 1), (3, 70, 37), (2, 255, 255), (2, 256, 1), (2, 257, 200), (2, 1024, 768), (1, 2048, 768), (2, 8192, 6000)]


@pytest.mark.parametrize("mode", [pf.NEAREST, pf.PLANE], ids=["nearest", "plane"])
@pytest.mark.parametrize("C", [3, 6, 5])
@pytest.mark.parametrize("B,N,K", SHAPES)
def test_kernel_against_the_numpy_model(B, N, K, C, mode):
    _lib, _ = _mods()
    assert SHAPES[-1][1] == _lib.L3D_CROP_MAX_N
    pts, vec, centre = _operands(100 * N + C, B, N, C, mode)
    _hold_to_model(pts, vec, centre, mode, K, _launch(pts, vec, centre, mode, K))


@pytest.mark.parametrize("mode", [pf.NEAREST, pf.PLANE], ids=["nearest", "plane"])
def test_base_pointers_misaligned_by_one_float(mode):
    _, P = _mods()
    B, N, C, K = 2, 257, 5, 200
    pts, vec, centre = _operands(7, B, N, C, mode)
    noise = np.random.default_rng(8).standard_normal((B, K, C)).astype(np.float32)

    def off(a, dtype):                                         # the same values, 4 bytes past a 256-byte boundary
        t = torch.as_tensor(a).to(DEV, dtype)
        flat = torch.empty(t.numel() + 1, dtype=dtype, device=DEV)
        flat[1:] = t.reshape(-1)
        v = flat[1:].view(t.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    aligned = _launch(pts, vec, centre, mode, K, noise=noise, clip=CLIP)
    idx = torch.empty(B * K + 1, dtype=torch.int64, device=DEV)[1:].view(B, K)
    mask = torch.empty(B * N + 1, device=DEV)[1:].view(B, N)
    out = torch.empty(B * K * C + 1, device=DEV)[1:].view(B, K, C)
    _lib = _mods()[0]
    _lib.call(NAME, off(pts, torch.float32), torch.as_tensor(vec).to(DEV), off(centre, torch.float32), B, N, C, mode, K, off(noise, torch.float32),
              None, CLIP, idx, mask, out)
    for a, b in zip(aligned, (idx, mask, out)):
        assert _bits(a, b.cpu())
    want_idx, _ = pf.select_batch(pts, vec, centre, mode, K)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert _bits(out, torch.from_numpy(pf.jitter(np.take_along_axis(pts, want_idx[:, :, None], axis=1), noise, None, CLIP)))


@pytest.mark.parametrize("mode", [pf.NEAREST, pf.PLANE], ids=["nearest", "plane"])
def test_duplicated_points_rank_by_index(mode):
    """twins across the K boundary (the lower index is kept), a run of twins inside the selection (listed by index in nearest mode),
    and a cloud that is one point N times (the first K indices)"""
    B, N, C, K = 3, 70, 3, 37
    pts, vec, centre = _operands(11, B, N, C, mode)            # (centre stays what it is: an input like any other)
    best_first = np.stack([np.argsort(pf.ordered_u64(pf.keys(pts[b], vec[b], centre[b], mode)) ^ np.uint64(0 if mode == pf.NEAREST else 2 ** 64 - 1),
                                      kind="stable") for b in range(B)])
    lo, hi = sorted((int(best_first[0, K - 1]), int(best_first[0, K])))
    pts[0, hi] = pts[0, lo]                                    # the K-th and the (K+1)-th best are one point
    twins = sorted(int(i) for i in best_first[1, 3:9])
    pts[1, twins] = pts[1, twins[2]]                           # six twins well inside the selection
    pts[2, :] = pts[2, 0]
    want = _hold_to_model(pts, vec, centre, mode, K, _launch(pts, vec, centre, mode, K))
    assert lo in want[0] and hi not in want[0]
    if mode == pf.NEAREST:
        assert want[1, 3:9].tolist() == twins
    else:
        assert set(twins) <= set(want[1].tolist())
    assert want[2].tolist() == list(range(K))


@pytest.mark.parametrize("mode", [pf.NEAREST, pf.PLANE], ids=["nearest", "plane"])
def test_a_nan_coordinate_ranks_above_every_number(mode):
    B, N, C, K = 2, 257, 6, 200
    pts, vec, centre = _operands(13, B, N, C, mode)
    pts[0, 17, 1] = np.nan
    pts[1, 5, 0] = pts[1, 200, 2] = np.nan
    centre = np.zeros((B, 3), dtype=np.float32)                # (a mean over a NaN would make every key a NaN)
    idx, mask, out = _launch(pts, vec, centre, mode, K)
    want = _hold_to_model(pts, vec, centre, mode, K, (idx, mask, out))
    if mode == pf.PLANE:                                       # the largest key: selected
        assert 17 in want[0] and {5, 200} <= set(want[1].tolist())
    else:                                                      # the largest key: the last to be selected, and K < N - 2
        assert 17 not in want[0] and not {5, 200} & set(want[1].tolist())
        full = _launch(pts, vec, centre, mode, N)
        assert _hold_to_model(pts, vec, centre, mode, N, full)[1, -2:].tolist() == [5, 200]


def test_k_equal_n():
    """nearest: a full sort; plane: nothing is ranked (vec and centre may be NULL), the jitter alone"""
    B, N, C = 2, 255, 5
    pts, vec, _ = _operands(17, B, N, C, pf.NEAREST)
    want = _hold_to_model(pts, vec, None, pf.NEAREST, N, _launch(pts, vec, None, pf.NEAREST, N))
    assert sorted(want[0].tolist()) == list(range(N))
    noise = np.random.default_rng(18).standard_normal((B, N, C)).astype(np.float32)
    sigma = np.array([0.03, 0.011], dtype=np.float32)
    idx, mask, out = _launch(pts, None, None, pf.PLANE, N, noise=noise, sigma=sigma, clip=CLIP)
    assert idx.cpu().tolist() == [list(range(N))] * B and bool((mask == 1).all())
    assert _bits(out, torch.from_numpy(pf.jitter(pts, noise, sigma, CLIP)))
    assert _bits(_launch(pts, None, None, pf.PLANE, N, noise=noise, sigma=sigma, clip=0.0)[2], torch.from_numpy(pf.jitter(pts, noise, sigma, 0.0)))


# ------------------------------------------------------------------------------------------------------------------------------
# the reference's own crops
def _seed_all(seed):
    np.random.seed(int(seed))
    torch.manual_seed(int(seed))


@pytest.mark.parametrize("name", [c[0] for c in pf.FARTHEST])
def test_farthest_subsample_points_gives_the_references_list(name):
    _, P = _mods()
    z = pf.load()
    pts, view, idx = z[f"{name}_points"], z[f"{name}_view"], z[f"{name}_idx"]
    K = len(idx)
    want_mask = np.zeros(len(pts), dtype=np.float32)
    want_mask[idx] = 1
    got = _launch(pts[None], view[None], None, pf.NEAREST, K)
    assert np.array_equal(got[0][0].cpu().numpy(), idx) and np.array_equal(got[1][0].cpu().numpy(), want_mask) and _bits(got[2][0], torch.from_numpy(pts[idx]))
    cpu = torch.from_numpy(pts)
    for part, mask in (P.farthest_subsample_points(cpu, K, view=view),               # the recorded draw
                       (_seed_all(z[f"{name}_seed"]), P.farthest_subsample_points(cpu, K))[1],     # np.random, in the reference's order
                       P.farthest_subsample_points(cpu.to(DEV), K, view=torch.from_numpy(view).to(DEV))):
        assert _bits(part, torch.from_numpy(pts[idx])) and np.array_equal(mask.cpu().numpy(), want_mask)
        assert part.is_cuda == mask.is_cuda
    part, mask = P.farthest_subsample_points(torch.from_numpy(np.stack([pts, pts[::-1]])), K, view=np.stack([view, view]))      # a batch
    assert _bits(part[0], torch.from_numpy(pts[idx])) and _bits(part[1], torch.from_numpy(pts[idx])) and mask.shape == (2, len(pts))


@pytest.mark.parametrize("name", [c[0] for c in pf.PLANAR])
def test_planar_crop_gives_the_references_list(name):
    _, P = _mods()
    z = pf.load()
    pts, normal, centre, idx = z[f"{name}_points"], z[f"{name}_normal"], z[f"{name}_centre"], z[f"{name}_idx"]
    K = len(idx)
    got = _launch(pts[None], normal[None], centre[None], pf.PLANE, K)                 # the reference's own centroid
    assert np.array_equal(got[0][0].cpu().numpy(), idx) and _bits(got[2][0], torch.from_numpy(pts[idx]))
    cpu = torch.from_numpy(pts)
    for part, kept in (P.planar_crop(cpu, normal=normal), (_seed_all(z[f"{name}_seed"]), P.planar_crop(cpu))[1],
                       P.planar_crop(cpu.to(DEV), normal=torch.from_numpy(normal))):
        assert np.array_equal(kept.cpu().numpy(), idx) and kept.dtype == torch.int64 and _bits(part, torch.from_numpy(pts[idx]))


def test_jitter_pointcloud_gives_the_references_values():
    _, P = _mods()
    z = pf.load()
    pts, want = torch.from_numpy(z["j_points"]), torch.from_numpy(z["j_out"])
    assert _bits(P.jitter_pointcloud(pts, noise=z["j_noise"]), want)
    _seed_all(z["j_seed"])
    assert _bits(P.jitter_pointcloud(pts), want)                                      # the reference's draws, in its order
    assert _bits(P.jitter_pointcloud(pts, sigma=7.0, noise=z["j_noise"]), want)       # `sigma` is ignored, as the reference ignores it
    sigma = np.array([np.float32(z["j_sigma"])])
    assert _bits(_launch(z["j_points"][None], None, None, pf.PLANE, len(pts), noise=z["j_unit"][None], sigma=sigma, clip=CLIP)[2][0], want)
    dev = P.jitter_pointcloud(pts.to(DEV), generator=torch.Generator(DEV).manual_seed(1))
    delta = (dev.cpu().double() - pts.double()).abs()
    assert dev.is_cuda and float(delta.max()) <= CLIP + 2.0 ** -23 * (1 + CLIP) and float(delta.max()) > 0


class _Recorded:
    """a stand-in for a transform: the reference's transformed source and igt, after the six np.random draws its transform makes"""

    def __init__(self, source, igt):
        self.source, self.igt_, self.index = source, igt, 0

    def __call__(self, template):
        for _ in range(6):
            np.random.uniform()
        self.igt = self.igt_
        return self.source


@pytest.mark.parametrize("name", [c[0] for c in pf.SAMPLES])
def test_whole_samples_from_the_stored_full_source(name):
    """the reference's RegistrationData sample from its transformed source on: step by step from the recorded draws, and as one
    RegistrationData.__getitem__ under the reference's seeds"""
    _, P = _mods()
    z = {k[len(name) + 1:]: v for k, v in pf.load().items() if k.startswith(name + "_")}
    full_t, full_s = torch.from_numpy(z["template_full"]), torch.from_numpy(z["source_full"])
    planar = name == "s_planar"
    if planar:
        source, idx_s = P.planar_crop(full_s, normal=z["normal_source"])
        template, idx_t = P.planar_crop(full_t, normal=z["normal_template"])
        t_mask, s_mask = P.intersection_masks(idx_s[None].to(DEV), idx_t[None].to(DEV), len(full_s))
        assert np.array_equal(idx_s.numpy(), z["idx_source"]) and np.array_equal(idx_t.numpy(), z["idx_template"])
        t_mask, s_mask = t_mask[0].cpu(), s_mask[0].cpu()
    else:
        source, s_mask = P.farthest_subsample_points(full_s, 768, view=z["view_source"])
        template, t_mask = P.farthest_subsample_points(full_t, 768, view=z["view_template"])
    assert _bits(template, torch.from_numpy(z["template"])) and _bits(P.jitter_pointcloud(source, noise=z["noise"]), torch.from_numpy(z["source"]))
    assert _bits(t_mask, torch.from_numpy(z["template_mask"])) and _bits(s_mask, torch.from_numpy(z["source_mask"]))

    params = {'partial_point_cloud_method': 'planar_crop'} if planar else {'use_masknet': True}
    ds = P.RegistrationData('PRNet', [(full_t, torch.zeros(1, dtype=torch.long))], partial_source=True, partial_template=True, noise=True,
                            additional_params=params)
    ds.transforms = _Recorded(full_s, torch.from_numpy(z["igt"]))
    _seed_all(z["seed"])
    sample = ds[0]
    assert len(sample) == (3 if planar else 5) and len(ds) == 1
    assert _bits(sample[0], torch.from_numpy(z["template"])) and _bits(sample[1], torch.from_numpy(z["source"])) and _bits(sample[2], torch.from_numpy(z["igt"]))
    assert _bits(ds.template_mask, torch.from_numpy(z["template_mask"])) and _bits(ds.source_mask, torch.from_numpy(z["source_mask"]))
    if not planar:
        assert sample[3] is ds.template_mask and sample[4] is ds.source_mask


def test_registration_data_runs_with_this_packages_transforms():
    _, P = _mods()
    g = torch.Generator().manual_seed(3)
    data = [(torch.rand((800, 3), generator=g) * 2 - 1, torch.tensor([i])) for i in range(3)]
    for algorithm, igt_shape in (("DCP", (4, 4)), ("PointNetLK", (4, 4)), ("iPCRNet", (1, 7))):
        ds = P.RegistrationData(algorithm, data, partial_source=True, additional_params={'use_masknet': True})
        template, source, igt, mask = ds[1]
        assert len(ds) == 3 and template.shape == (800, 3) and source.shape == (768, 3) and igt.shape == igt_shape and not source.is_cuda
        assert mask.shape == (800,) and float(mask.sum()) == 768
    gmr = P.RegistrationData("DeepGMR", data, additional_params={'nearest_neighbors': 4})
    template, source, igt = gmr[0]
    assert template.shape == source.shape == (800, 3 + 16) and bool(torch.isfinite(source).all())
    with pytest.raises(Exception, match="not available"):
        P.RegistrationData("ICP", data)


# ------------------------------------------------------------------------------------------------------------------------------
# repeatability and the memory contract
@pytest.mark.parametrize("mode", [pf.NEAREST, pf.PLANE], ids=["nearest", "plane"])
def test_same_bits_whatever_the_outputs_held_and_with_each_output_null(mode):
    _lib, _ = _mods()
    B, N, C, K = 3, 257, 6, 200
    pts, vec, centre = _operands(23, B, N, C, mode)
    noise = np.random.default_rng(24).standard_normal((B, K, C)).astype(np.float32)
    sigma = np.array([0.01, 0.04, 0.025], dtype=np.float32)
    ops = [torch.as_tensor(a).to(DEV) for a in (pts, vec, centre, noise, sigma)]

    def run(fill, idx=True, mask=True, out=True):
        o = [torch.full((B, K), -1 if fill != 0 else 0, dtype=torch.int64, device=DEV) if idx else None,
             torch.full((B, N), fill, device=DEV) if mask else None, torch.full((B, K, C), fill, device=DEV) if out else None]
        _lib.call(NAME, ops[0], ops[1], ops[2], B, N, C, mode, K, ops[3], ops[4], CLIP, *o)
        return o
    first = run(0.0)
    want_idx, want_mask = pf.select_batch(pts, vec, centre, mode, K)
    assert np.array_equal(first[0].cpu().numpy(), want_idx) and np.array_equal(first[1].cpu().numpy(), want_mask)
    assert _bits(first[2], torch.from_numpy(pf.jitter(np.take_along_axis(pts, want_idx[:, :, None], axis=1), noise, sigma, CLIP)))
    for fill in (float("nan"), 1e30):
        for a, b in zip(first, run(fill)):
            assert _bits(a, b.cpu())
    for keep in range(3):
        flags = [i == keep for i in range(3)]
        alone = run(float("nan"), *flags)
        assert _bits(alone[keep], first[keep].cpu()) and sum(o is not None for o in alone) == 1
        pair = run(float("nan"), *[not f for f in flags])
        assert all(_bits(pair[i], first[i].cpu()) for i in range(3) if i != keep)


@pytest.mark.parametrize("noisy", [False, True], ids=["copy", "noise"])
@pytest.mark.parametrize("mode", [pf.NEAREST, pf.PLANE], ids=["nearest", "plane"])
def test_memory_contract(mode, noisy):
    """guards, two fills, const inputs unchanged; tails in N and K, an odd C"""
    _lib, _ = _mods()
    B, N, C, K = 2, 70, 5, 37
    pts, vec, centre = _operands(29, B, N, C, mode)
    noise = np.random.default_rng(30).standard_normal((B, K, C)).astype(np.float32) if noisy else None
    sigma = np.array([0.02, 0.03], dtype=np.float32) if noisy else None
    ops = [None if a is None else torch.as_tensor(a).to(DEV) for a in (pts, vec, centre, noise, sigma)]
    got = mc.check(NAME, lambda ar: [ops[0], ops[1], ops[2], B, N, C, mode, K, ops[3], ops[4], CLIP, ar.out(torch.int64, B, K), ar.f32(B, N),
                                     ar.f32(B, K, C)], proto=_lib.EXT_PROTOTYPES[NAME])
    want_idx, want_mask = pf.select_batch(pts, vec, centre, mode, K)
    rows = np.take_along_axis(pts, want_idx[:, :, None], axis=1)
    assert np.array_equal(got["idx"].cpu().numpy(), want_idx) and np.array_equal(got["mask"].cpu().numpy(), want_mask)
    assert _bits(got["out"], torch.from_numpy(pf.jitter(rows, noise, sigma, CLIP) if noisy else rows))
    alone = mc.check(NAME, lambda ar: [ops[0], ops[1], ops[2], B, N, C, mode, K, ops[3], ops[4], CLIP, None, None, ar.f32(B, K, C)],
                     proto=_lib.EXT_PROTOTYPES[NAME])
    assert _bits(alone["out"], got["out"].cpu())


# ------------------------------------------------------------------------------------------------------------------------------
# the feed
def _dataset(M=6, P_=160, seed=41):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((M, P_, 3), generator=g) * 2 - 1).to(DEV), torch.arange(M).to(DEV)


def _feed(**kw):
    from learning3d_amd.data_utils import ResidentRegistrationFeed
    data, labels = _dataset()
    kw.setdefault("num_subsampled_points", 96)
    return ResidentRegistrationFeed(data, labels, batch_size=2, num_points=128, seed=5, **kw)


def test_default_options_are_bit_equal_to_a_feed_built_without_them():
    from learning3d_amd.data_utils import ResidentRegistrationFeed
    data, labels = _dataset()
    plain = ResidentRegistrationFeed(data, labels, batch_size=2, num_points=128, seed=5)
    spelled = ResidentRegistrationFeed(data, labels, batch_size=2, num_points=128, seed=5, partial_source=False, partial_template=False,
                                       num_subsampled_points=768, partial_method="farthest", noise=False, masks=False)
    masks_only = ResidentRegistrationFeed(data, labels, batch_size=2, num_points=128, seed=5, masks=True)    # nothing is cropped: no masks
    batches = [list(f) for f in (plain, spelled, masks_only)]
    assert len(batches[0]) == 3
    for other in batches[1:]:
        for a, b in zip(batches[0], other):
            assert len(a) == len(b) == 4 and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("method", ["farthest", "planar_crop"])
def test_feed_invariants(method):
    """from one batch's own transform and draws: a partial source is transform(template)[idx], template[mask == 1] is the partial
    template's point set, the planar masks pick the same original points on both sides, and the jitter stays inside clip"""
    _lib, P = _mods()
    planar = method == "planar_crop"
    feed = _feed(partial_source=True, partial_template=True, partial_method=method, noise=True, masks=True)
    clean = _feed(partial_source=True, partial_template=True, partial_method=method, masks=True)
    template = feed.data[:2, :128].contiguous()
    full = feed.transform(template)
    draws = feed.draw_partial(2)
    K = P.plane_keep_count(128) if planar else 96
    assert feed.num_kept == K and draws["noise"].shape == (2, K, 3) and draws["source"].dtype == torch.float64
    _lib.LAUNCH_LOG = log = []
    try:
        part_t, part_s, (t_mask, s_mask) = feed.crop_batch(template, full, draws)
    finally:
        _lib.LAUNCH_LOG = None
    assert log == [NAME, NAME]                                 # one launch per cropped cloud, the jitter inside the source's
    clean_t, clean_s, clean_masks = clean.crop_batch(template, full, {k: v for k, v in draws.items() if k in ("source", "template")})
    mode = pf.PLANE if planar else pf.NEAREST
    tn, fn = template.cpu().numpy(), full.cpu().numpy()
    centre = (lambda x: x.mean(dim=1).cpu().numpy()) if planar else (lambda x: None)
    idx_s, _ = pf.select_batch(fn, draws["source"].cpu().numpy(), centre(full), mode, K)
    idx_t, _ = pf.select_batch(tn, draws["template"].cpu().numpy(), centre(template), mode, K)
    assert _bits(clean_s, torch.from_numpy(np.take_along_axis(fn, idx_s[:, :, None], axis=1)))
    assert _bits(part_t, torch.from_numpy(np.take_along_axis(tn, idx_t[:, :, None], axis=1))) and torch.equal(part_t, clean_t)
    assert all(torch.equal(a, b) for a, b in zip((t_mask, s_mask), clean_masks))
    if planar:
        assert t_mask.shape == s_mask.shape == (2, K)
        for b in range(2):
            both = np.intersect1d(idx_s[b], idx_t[b])
            assert np.array_equal(idx_t[b][t_mask[b].cpu().numpy() == 1], both) and np.array_equal(idx_s[b][s_mask[b].cpu().numpy() == 1], both)
            assert 0 < len(both) < K
    else:
        assert t_mask.shape == s_mask.shape == (2, 128) and float(t_mask.sum()) == float(s_mask.sum()) == 2 * K
        for b in range(2):
            rows = lambda x: sorted(map(tuple, x.cpu().tolist()))     # noqa: E731
            assert rows(template[b][t_mask[b] == 1]) == rows(part_t[b]) and rows(full[b][s_mask[b] == 1]) == rows(clean_s[b])
    # out = fl(p + e), |e| <= clip: |out - p| <= clip + half an ulp of the sum, and |p| + clip < 4 here (|translation| <= 1, |x| <= sqrt 3)
    delta = (part_s.double() - clean_s.double()).abs()
    assert float(delta.max()) <= CLIP + 2.0 ** -24 * 4 and float(delta.max()) > 0
    assert _bits(part_s, torch.from_numpy(pf.jitter(clean_s.cpu().numpy(), draws["noise"].cpu().numpy(), draws["sigma"].cpu().numpy(), CLIP)))


def test_feed_yields_the_masks_behind_the_labels_and_noise_alone_is_one_launch():
    _lib, P = _mods()
    from learning3d_amd.data_utils import ResidentRegistrationFeed
    from learning3d_amd.ops.transform_functions import PNLKTransform
    batches = list(_feed(partial_source=True, noise=True, masks=True))
    assert len(batches) == 3
    template, source, igt, labels, source_mask = batches[0]
    assert template.shape == (2, 128, 3) and source.shape == (2, 96, 3) and igt.shape == (2, 4, 4) and labels.shape == (2,)
    assert source_mask.shape == (2, 128) and float(source_mask.sum()) == 2 * 96
    both = next(iter(_feed(partial_source=True, partial_template=True, masks=True)))
    assert len(both) == 6 and both[0].shape == both[1].shape == (2, 96, 3) and both[4].shape == both[5].shape == (2, 128)
    assert len(next(iter(_feed(partial_source=True, partial_template=True)))) == 4
    noisy, plain = _feed(noise=True), _feed()
    _lib.LAUNCH_LOG = log = []
    try:
        a = next(iter(noisy))
    finally:
        _lib.LAUNCH_LOG = None
    b = next(iter(plain))
    assert log.count(NAME) == 1 and torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and a[1].shape == b[1].shape
    delta = (a[1].double() - b[1].double()).abs()
    assert 0 < float(delta.max()) <= CLIP + 2.0 ** -24 * 4
    data, labels = _dataset()
    lk = ResidentRegistrationFeed.for_algorithm("PointNetLK", data, labels, batch_size=2, num_points=128, partial_source=True, num_subsampled_points=96)
    assert isinstance(lk.transform, PNLKTransform) and lk.transform.generator is lk.gen and next(iter(lk))[1].shape == (2, 96, 3)
    with pytest.raises(ValueError):
        _feed(partial_source=True, num_subsampled_points=129)


def test_a_feed_batch_replays_from_one_graph_on_one_stream():
    """the transform launch, both crops, the fused jitter and the masks, captured once and replayed twice over stale outputs"""
    from learning3d_amd.ops.transform_functions import euler_transform
    for method in ("farthest", "planar_crop"):
        feed = _feed(partial_source=True, partial_template=True, partial_method=method, noise=True, masks=True)
        template = feed.data[2:4, :128].contiguous()
        draws = feed.draw_partial(2)
        euler = torch.rand((2, 3), device=DEV, generator=feed.gen)
        shift = torch.rand((2, 3), device=DEV, generator=feed.gen)

        def run():
            source, igt = euler_transform(template, euler, shift)
            t, s, masks = feed.crop_batch(template, source, draws)
            return [t, s, igt, *masks]
        eager = [v.clone() for v in run()]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()                                              # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = run()
        for replay in range(2):
            for v in out:
                v.fill_(7)                                     # stale values must not survive a replay
            graph.replay()
            torch.cuda.synchronize()
            assert len(out) == 5 and all(torch.equal(a, b) for a, b in zip(out, eager)), (method, replay)


# ------------------------------------------------------------------------------------------------------------------------------
# end to end
def test_a_masks_batch_goes_through_masknet_and_a_partial_batch_through_prnet():
    from learning3d_amd.models import MaskNet, PRNet
    template, source, igt, labels, gt_mask = next(iter(_feed(partial_source=True, noise=True, masks=True)))
    net = seeded_params(MaskNet(), 3).to(DEV).eval()
    with torch.no_grad():
        masked_template, predicted = net(template, source)
    assert masked_template.shape == source.shape == (2, 96, 3) and predicted.shape == gt_mask.shape == (2, 128)
    assert bool(torch.isfinite(predicted).all()) and bool(torch.isfinite(masked_template).all())
    assert bool(torch.isfinite(torch.nn.functional.mse_loss(predicted, gt_mask)))

    template, source, igt, labels = next(iter(_feed(partial_source=True, partial_template=True, noise=True)))
    prnet = seeded_params(PRNet(emb_nn='pointnet', attention='identity', emb_dims=64, num_keypoints=32, num_subsampled_points=96, num_iters=1), 4)
    prnet = prnet.to(DEV).eval()
    with torch.no_grad():
        out = prnet(source, template, igt)
    assert out["est_R"].shape == (2, 3, 3) and out["est_t"].shape == (2, 3) and out["transformed_source"].shape == (2, 96, 3)
    assert all(bool(torch.isfinite(out[k]).all()) for k in ("est_R", "est_t", "est_T", "transformed_source", "loss"))
