"""Fixture of the partial / noisy registration pairs, from the REFERENCE on the CPU:

    python tests/golden/make_golden_partial.py

Needs the reference checkout make_golden.py reads (imported only through make_golden.import_reference, which puts the synthetic
dataset files in place first).  Writes partial_seeded.npz next to this file: arrays only.  It calls the reference's own functions
(data_utils.dataloaders: farthest_subsample_points, planar_crop, jitter_pointcloud, RegistrationData) and copies none of their code.

Per case np.random and torch are seeded, the reference runs, and the same seeds are set again to replay its draws in its order (the
view point; the plane normal; the jitter's standard deviation and normal_ tensor; for a whole sample the transform first), so that
the fixture holds the inputs, every draw and the reference's result:
  * farthest_subsample_points  (partial_fixture.FARTHEST): points, view, the reference's index list in its order
  * planar_crop                (partial_fixture.PLANAR):   points, normal, the reference's fp32 centroid, kept indices
  * jitter_pointcloud:         cloud, the 0.04 U draw, the clamped normal_(0, sigma) tensor, the unit normal_ tensor of the same seed
  * RegistrationData('PRNet', partial_source, partial_template, noise, use_masknet) and one planar_crop sample on the synthetic
    ModelNet40 files: the template, the reference's transformed full source and igt, every draw, and the returned tuple

The seed of a case is stepped until these hold -- conditions on the inputs, not measurements:
  * every gap between consecutive sorted fp64 nearest-mode keys is >= partial_fixture.NEAREST_GAP (one fp64 ulp there is ~1e-10);
  * the plane-mode key gap across the K boundary is >= partial_fixture.PLANE_GAP;
  * the view point has the sign the case asks for.
Then it asserts that partial_fixture's numpy model reproduces the reference's index lists, order included, that plane_keep_count
gives the reference's kept counts, and that sigma * (unit normal_) equals normal_(0, sigma) bit for bit in fp32.  Nothing is
masked out.  It also prints the host time of the reference's crop per cloud on this CPU (a single unloaded run)."""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg            # noqa: E402
import partial_fixture as pf        # noqa: E402

SEED_START = 9100
MAX_SEEDS = 200


def seed_all(seed):
    np.random.seed(seed)
    torch.manual_seed(seed)


def cloud(seed, N, C):
    g = np.random.default_rng(seed)
    xyz = g.uniform(-1, 1, (N, 3))
    if C == 3:
        return xyz.astype(np.float32)
    nrm = g.standard_normal((N, C - 3))
    return np.concatenate([xyz, nrm / np.linalg.norm(nrm, axis=1, keepdims=True)], axis=1).astype(np.float32)


def draw_view():
    return (np.random.random(size=(1, 3)) + np.array([[500, 500, 500]]) * np.random.choice([1, -1, 1, -1]))[0]


def nearest_gap(points, view):
    return float(np.diff(np.sort(pf.keys(points, view, None, pf.NEAREST))).min())


def plane_gap(points, normal, centre, K):
    k = np.sort(pf.keys(points, normal, centre, pf.PLANE))[::-1]
    return float(k[K - 1] - k[K]) if K < len(k) else float("inf")


def stepped(what, make):
    """make(seed) -> (ok, note, payload): the first seed from SEED_START on that meets the case's conditions"""
    for seed in range(SEED_START, SEED_START + MAX_SEEDS):
        ok, note, payload = make(seed)
        print(f"  {what}: seed {seed}: {note}" + ("" if ok else "  -- next seed"), flush=True)
        if ok:
            return seed, payload
    raise AssertionError(f"{what}: no seed met the conditions")


def farthest_case(Dl, out, name, N, K, C, sign, times):
    def make(seed):
        pts = cloud(seed, N, C)
        seed_all(seed)
        view = draw_view()
        gap = nearest_gap(pts, view)
        ok = gap >= pf.NEAREST_GAP and np.sign(view[0]) == sign
        if not ok:
            return False, f"smallest key gap {gap:.2e}, sign {int(np.sign(view[0])):+d}", None
        seed_all(seed)
        t0 = time.perf_counter()
        part, mask = Dl.farthest_subsample_points(torch.from_numpy(pts.copy()), K)
        times.append((N, time.perf_counter() - t0))
        # the reference returns rows and a mask; its order is read off the rows (the key gaps make every xyz row distinct)
        rows = {pts[i, :3].tobytes(): i for i in range(N)}
        idx = np.array([rows[r.tobytes()] for r in part.numpy()[:, :3]], dtype=np.int64)
        assert len(rows) == N and np.array_equal(part.numpy(), pts[idx]) and np.array_equal(np.flatnonzero(mask.numpy()), np.sort(idx))
        assert np.array_equal(pf.select(pts, view, None, pf.NEAREST, K), idx), "the fp64 model does not give the reference's list"
        return True, f"smallest key gap {gap:.2e}, sign {int(sign):+d}, model == reference", (pts, view, idx)
    seed, (pts, view, idx) = stepped(name, make)
    out.update({f"{name}_points": pts, f"{name}_view": view, f"{name}_idx": idx, f"{name}_seed": seed})


def planar_case(Dl, out, name, N):
    from learning3d_amd.data_utils.partial import plane_keep_count

    def make(seed):
        pts = cloud(seed, N, 3)
        seed_all(seed)
        part, idx_x = Dl.planar_crop(torch.from_numpy(pts.copy()))
        idx = idx_x.numpy().reshape(-1).astype(np.int64)
        seed_all(seed)
        normal = Dl.uniform_2_sphere()
        centre = np.mean(pts[:, :3], axis=0)
        K = len(idx)
        gap = plane_gap(pts, normal, centre, K)
        if gap < pf.PLANE_GAP:
            return False, f"boundary gap {gap:.2e}", None
        assert K == plane_keep_count(N), (K, plane_keep_count(N))
        assert np.array_equal(part.numpy(), pts[idx])
        assert np.array_equal(pf.select(pts, normal, centre, pf.PLANE, K), idx), "the fp64 model does not give the reference's list"
        return True, f"kept {K} of {N}, boundary gap {gap:.2e}, model == reference", (pts, normal, centre.astype(np.float32), idx)
    seed, (pts, normal, centre, idx) = stepped(name, make)
    out.update({f"{name}_points": pts, f"{name}_normal": normal, f"{name}_centre": centre, f"{name}_idx": idx, f"{name}_seed": seed})


def replay_jitter(shape):
    """the draws jitter_pointcloud makes, in its order -> (sigma fp64, the clamped normal_(0, sigma) tensor)"""
    sigma = 0.04 * np.random.random_sample()
    return sigma, torch.empty(shape).normal_(mean=0, std=sigma).clamp(-0.05, 0.05)


def jitter_case(Dl, out):
    seed = SEED_START
    pts = cloud(seed, 1024, 3)
    seed_all(seed)
    got = Dl.jitter_pointcloud(torch.from_numpy(pts.copy()))
    seed_all(seed)
    sigma, noise = replay_jitter(pts.shape)
    assert np.array_equal(got.numpy(), pts + noise.numpy())
    seed_all(seed)
    np.random.random_sample()
    unit = torch.empty(pts.shape).normal_(mean=0, std=1)
    scaled = (np.float32(sigma) * unit.numpy()).astype(np.float32)
    exact = np.array_equal(np.clip(scaled, np.float32(-0.05), np.float32(0.05)), noise.numpy())
    print(f"  jitter: sigma {sigma:.6f}, {int((noise.abs() == 0.05).sum())} of {noise.numel()} clamped, float32(sigma) * unit == normal_(0, sigma): {exact}")
    assert exact
    out.update(j_points=pts, j_sigma=np.float64(sigma), j_noise=noise.numpy(), j_unit=unit.numpy(), j_out=got.numpy(), j_seed=seed)


def sample_case(Dl, out, name, index, planar):
    from learning3d_amd.data_utils.partial import plane_keep_count
    data = Dl.ModelNet40Data(train=True, num_points=1024, download=False)
    params = {'partial_point_cloud_method': 'planar_crop'} if planar else {'use_masknet': True}

    def dataset():
        return Dl.RegistrationData('PRNet', data, partial_source=True, partial_template=True, noise=True, additional_params=params)

    def make(seed):
        template0 = data[index][0]
        seed_all(seed)
        ds = dataset()
        sample = ds[index]
        # the same draws again, in RegistrationData's order: the transform, the crop of the source, of the template, the jitter
        seed_all(seed)
        rp = dataset()
        full = rp.transforms(template0.clone())
        igt = rp.transforms.igt
        tn, fn = template0.numpy(), full.numpy()
        o = {"template_full": tn, "source_full": fn, "igt": igt.numpy()}
        if planar:
            n_s, n_t = Dl.uniform_2_sphere(), Dl.uniform_2_sphere()
            c_s, c_t = np.mean(fn, axis=0), np.mean(tn, axis=0)
            K = plane_keep_count(1024)
            gap = min(plane_gap(fn, n_s, c_s, K), plane_gap(tn, n_t, c_t, K))
            if gap < pf.PLANE_GAP:
                return False, f"boundary gap {gap:.2e}", None
            i_s, i_t = pf.select(fn, n_s, c_s, pf.PLANE, K), pf.select(tn, n_t, c_t, pf.PLANE, K)
            o.update(normal_source=n_s, normal_template=n_t, centre_source=c_s.astype(np.float32), centre_template=c_t.astype(np.float32),
                     template_mask=ds.template_mask.numpy(), source_mask=ds.source_mask.numpy())
        else:
            v_s, v_t = draw_view(), draw_view()
            K = 768
            gap = min(nearest_gap(fn, v_s), nearest_gap(tn, v_t))
            if gap < pf.NEAREST_GAP:
                return False, f"smallest key gap {gap:.2e}", None
            i_s, i_t = pf.select(fn, v_s, None, pf.NEAREST, K), pf.select(tn, v_t, None, pf.NEAREST, K)
            o.update(view_source=v_s, view_template=v_t, template_mask=sample[3].numpy(), source_mask=sample[4].numpy())
            assert len(sample) == 5 and np.array_equal(np.flatnonzero(o["template_mask"]), np.sort(i_t))
            assert np.array_equal(np.flatnonzero(o["source_mask"]), np.sort(i_s))
        sigma, noise = replay_jitter((K, 3))
        # the reference's sample is the model's rows, in the model's order, plus the replayed jitter: bit for bit
        assert np.array_equal(sample[0].numpy(), tn[i_t]), "template: the fp64 model does not give the reference's rows"
        assert np.array_equal(sample[1].numpy(), fn[i_s] + noise.numpy()), "source: the fp64 model does not give the reference's rows"
        assert np.array_equal(sample[2].numpy(), o["igt"])
        o.update(idx_source=i_s, idx_template=i_t, sigma=np.float64(sigma), noise=noise.numpy(), template=sample[0].numpy(), source=sample[1].numpy())
        return True, f"K {K}, gap {gap:.2e}, model == reference", o
    seed, o = stepped(name, make)
    out.update({f"{name}_{k}": v for k, v in o.items()})
    out[f"{name}_seed"] = seed


def main():
    torch.set_num_threads(8)
    mg.import_reference()
    import learning3d.data_utils.dataloaders as Dl
    out, times = {}, []
    for case in pf.FARTHEST:
        farthest_case(Dl, out, *case, times)
    for case in pf.PLANAR:
        planar_case(Dl, out, *case)
    jitter_case(Dl, out)
    for (name, index), planar in zip(pf.SAMPLES, (False, True)):
        sample_case(Dl, out, name, index, planar)
    for N in sorted({n for n, _ in times}):
        ts = [t for n, t in times if n == N]
        print(f"  the reference's farthest_subsample_points on this host CPU: N {N}: {1e3 * min(ts):.2f} .. {1e3 * max(ts):.2f} ms per cloud "
              f"({len(ts)} clouds; the first call of the run includes scikit-learn's set-up)")
    path = os.path.join(HERE, "partial_seeded.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"  partial_seeded.npz  {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    main()
