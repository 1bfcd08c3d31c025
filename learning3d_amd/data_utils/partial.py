"""Partial and noisy registration pairs (reference: data_utils/dataloaders.py:63-119 jitter_pointcloud, farthest_subsample_points,
uniform_2_sphere, planar_crop, and :250-330 RegistrationData).  The reference crops one cloud at a time on the host (scikit-learn's
NearestNeighbors under a Python metric, numpy's percentile); here a crop, its mask and the jitter of a whole batch are ONE launch of
l3d_crop_select (include/ext/l3d_partial.h), one workgroup per cloud.

Every function takes one cloud [N,C] or a batch [B,N,C], on the CPU or on the device.  CPU tensors are moved to the device, computed
there and handed back (transform_functions._on_gpu); nothing but the random draws is formed on the host.  With no explicit draws a
CPU input consumes np.random and torch's CPU generator in the reference's order, cloud by cloud -- np.random.random((1,3)) then
np.random.choice([1,-1,1,-1]) for a view point, np.random.uniform twice for a plane normal, np.random.random_sample() then
torch.empty(shape).normal_ for the jitter -- so a seeded script gets the reference's crops; a device input draws from a
torch.Generator on its device (`generator`, the device's default one when None) and never touches the host.

What differs from the reference, on purpose:
  * jitter_pointcloud returns a new tensor (the reference adds in place and returns its argument).  Like the reference it IGNORES its
    `sigma` argument: the standard deviation is 0.04 U(0,1), drawn per cloud.
  * planar_crop returns the kept indices as int64 [K] (the reference: a float tensor [1,K]); np.intersect1d takes both.
  * planar_crop's centroid is torch's fp32 mean on the device, numpy's is a sequential fp32 sum: the two can differ by an ulp, so the
    crop agrees with the reference's except where two points straddle the percentile within that ulp.  The kept COUNT is the
    reference's (plane_keep_count)."""
import numpy as np
import torch

from .. import _lib
from .._lib import call, f32c, on_device_of
from ..ops.transform_functions import _on_gpu

VIEW_OFFSET = 500.0          # farthest_subsample_points: the view point is U(0,1)^3 + (+-500, +-500, +-500), one sign for all three
JITTER_SCALE = 0.04          # jitter_pointcloud: sigma = 0.04 U(0,1), whatever its `sigma` argument says


def crop_select(points, vec, mode, K, centre=None, noise=None, sigma=None, clip=0.0, want_idx=True, want_mask=True, want_out=True):
    """l3d_crop_select on device tensors: points [B,N,C] fp32, vec [B,3] fp64, centre [B,3] fp32 (plane mode), noise [B,K,C], sigma [B]
    -> (idx int64 [B,K], mask [B,N], out [B,K,C]), None for an output that is not wanted.  The header states the arithmetic."""
    B, N, Cc = points.shape
    dev = points.device
    idx = torch.empty((B, K), dtype=torch.int64, device=dev) if want_idx else None
    mask = torch.empty((B, N), dtype=torch.float32, device=dev) if want_mask else None
    out = torch.empty((B, K, Cc), dtype=torch.float32, device=dev) if want_out else None
    with on_device_of(points):
        call("l3d_crop_select", points, vec, centre, B, N, Cc, int(mode), int(K), noise, sigma, float(clip), idx, mask, out)
    return idx, mask, out


def plane_keep_count(num_points, p_keep=0.7):
    """the number of points planar_crop keeps: those strictly above np.percentile(dist, q) with q = (float32(1) - float32(p_keep)) 100
    as the reference forms it (30.000002 for 0.7), under numpy's linear interpolation: N - 1 - floor(q (N - 1) / 100)"""
    q = float((np.float32(1.0) - np.float32(p_keep)) * np.float32(100))
    return int(num_points - 1 - int(np.floor(q * (num_points - 1) / 100.0)))


def uniform_2_sphere(num=None, device=None, generator=None):
    """A uniform direction on the 2-sphere (reference :79-104).  device None: the reference's numpy function on np.random (phi, then
    cos theta; [num,3], or [3] for num None).  With a device: an fp64 tensor of the same shape drawn from `generator` there."""
    if device is None:
        if num is not None:
            phi = np.random.uniform(0.0, 2 * np.pi, num)
            cos_theta = np.random.uniform(-1.0, 1.0, num)
        else:
            phi = np.random.uniform(0.0, 2 * np.pi)
            cos_theta = np.random.uniform(-1.0, 1.0)
        theta = np.arccos(cos_theta)
        return np.stack((np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)), axis=-1)
    u = torch.rand((2, 1 if num is None else num), dtype=torch.float64, device=device, generator=generator)
    phi, cos_theta = u[0] * (2 * np.pi), u[1] * 2 - 1
    sin_theta = torch.sqrt((1 - cos_theta * cos_theta).clamp_min(0))
    v = torch.stack([sin_theta * torch.cos(phi), sin_theta * torch.sin(phi), cos_theta], dim=-1)
    return v[0] if num is None else v


def draw_views(batch, device, generator=None):
    """[batch,3] fp64 view points of farthest_subsample_points, drawn on `device`"""
    u = torch.rand((batch, 4), dtype=torch.float64, device=device, generator=generator)
    return u[:, :3] + VIEW_OFFSET * torch.where(u[:, 3:] < 0.5, 1.0, -1.0)


def _batched(t):
    """-> (device fp32 contiguous [B,N,C], single, back)"""
    if t.dim() not in (2, 3) or t.shape[-1] < 3:
        raise ValueError(f"expected a cloud [N,C] or a batch [B,N,C] with C >= 3, got {tuple(t.shape)}")
    x, back = _on_gpu(t)
    single = x.dim() == 2
    return f32c(x.unsqueeze(0) if single else x), single, back


def _draws(value, shape, dtype, device):
    """an explicit draw -> a contiguous device tensor of `shape`"""
    v = torch.as_tensor(value).to(device=device, dtype=dtype).reshape(shape)
    return v.contiguous()


def _hand_back(single, back, *ts):
    out = []
    for t in ts:
        t = t[0] if single else t
        out.append(t.cpu() if back else t)
    return tuple(out)


def farthest_subsample_points(pointcloud, num_subsampled_points=768, view=None, *, generator=None):
    """The `num_subsampled_points` points nearest a far random view point, nearest first, and the mask of the kept points over the
    full cloud (reference :69-77).  view: [3] or [B,3] (fp64) instead of the draw.  -> (partial [..,K,C], gt_mask [..,N])."""
    x, single, back = _batched(pointcloud)
    B, N, _ = x.shape
    K = int(num_subsampled_points)
    if view is not None:
        v = _draws(view, (B, 3), torch.float64, x.device)
    elif back:
        v = torch.from_numpy(np.concatenate([np.random.random(size=(1, 3)) + np.array([[VIEW_OFFSET] * 3]) * np.random.choice([1, -1, 1, -1])
                                             for _ in range(B)], axis=0)).to(x.device)
    else:
        v = draw_views(B, x.device, generator)
    _, mask, out = crop_select(x, v, _lib.L3D_CROP_NEAREST, K, want_idx=False)
    return _hand_back(single, back, out, mask)


def planar_crop(points, p_keep=0.7, normal=None, *, generator=None):
    """The points farthest along a random direction from the centroid, a fraction p_keep of them, in their original order; x y z only
    (reference :106-119).  normal: [3] or [B,3] (fp64) instead of the draw.  -> (partial [..,K,3], idx int64 [..,K])."""
    x, single, back = _batched(points)
    x = x[:, :, :3].contiguous()
    B, N, _ = x.shape
    if normal is not None:
        n = _draws(normal, (B, 3), torch.float64, x.device)
    elif back:
        n = torch.from_numpy(np.stack([uniform_2_sphere() for _ in range(B)], axis=0)).to(x.device)
    else:
        n = uniform_2_sphere(B, x.device, generator)
    idx, _, out = crop_select(x, n.contiguous(), _lib.L3D_CROP_PLANE, plane_keep_count(N, p_keep), centre=x.mean(dim=1), want_mask=False)
    return _hand_back(single, back, out, idx)


def jitter_pointcloud(pointcloud, sigma=0.04, clip=0.05, noise=None, *, generator=None):
    """pointcloud + clamp(Normal(0, s), -clip, clip) with s = 0.04 U(0,1) per cloud (reference :63-67, which ignores `sigma`; so does
    this).  noise: the tensor to clamp and add, of the cloud's shape, instead of the draws.  -> a new tensor."""
    x, single, back = _batched(pointcloud)
    B, N, Cc = x.shape
    s = None
    if noise is not None:
        z = _draws(noise, (B, N, Cc), torch.float32, x.device)
    elif back:
        # the reference's calls, cloud by cloud: the standard deviation goes into normal_ as there
        z = torch.stack([torch.empty((N, Cc)).normal_(mean=0, std=JITTER_SCALE * np.random.random_sample()) for _ in range(B)]).to(x.device)
    else:
        s = JITTER_SCALE * torch.rand((B,), device=x.device, generator=generator)
        z = torch.randn((B, N, Cc), device=x.device, generator=generator)
    _, _, out = crop_select(x, None, _lib.L3D_CROP_PLANE, N, noise=z, sigma=s, clip=clip, want_idx=False, want_mask=False)
    return _hand_back(single, back, out)[0]


def intersection_masks(idx_source, idx_template, num_points):
    """planar path of RegistrationData (:299-304): idx_* int64 [B,K] kept indices of the two crops of clouds in correspondence ->
    (template_mask [B,Kt], source_mask [B,Ks]), 1.0 where the kept point was kept on the other side too.  Device work only."""
    B = idx_source.shape[0]
    kept_s = torch.zeros((B, num_points), dtype=torch.float32, device=idx_source.device).scatter_(1, idx_source, 1.0)
    kept_t = torch.zeros((B, num_points), dtype=torch.float32, device=idx_source.device).scatter_(1, idx_template, 1.0)
    return torch.gather(kept_s, 1, idx_template), torch.gather(kept_t, 1, idx_source)


ALGORITHMS = ('PCRNet', 'PointNetLK', 'DCP', 'PRNet', 'iPCRNet', 'RPMNet', 'DeepGMR')


def transform_for(algorithm, data_size=None, generator=None):
    """the transform RegistrationData gives each algorithm (reference :264-279), as this package's device transforms"""
    from ..ops import transform_functions as T
    if algorithm not in ALGORITHMS:
        raise Exception("Algorithm not available for registration.")
    if algorithm in ('PCRNet', 'iPCRNet'):
        return T.PCRNetTransform(data_size, angle_range=45, translation_range=1, generator=generator)
    if algorithm == 'PointNetLK':
        return T.PNLKTransform(0.8, True, generator=generator)
    if algorithm == 'RPMNet':
        return T.RPMNetTransform(0.8, True, generator=generator)
    if algorithm in ('DCP', 'PRNet'):
        return T.DCPTransform(angle_range=45, translation_range=1, generator=generator)
    return T.DeepGMRTransform(angle_range=90, translation_range=1, generator=generator)


class RegistrationData(torch.utils.data.Dataset):
    """reference: data_utils/dataloaders.py:250-330, same constructor, algorithm list, per-algorithm transform, `additional_params`
    (partial_point_cloud_method='planar_crop', use_masknet, nearest_neighbors for DeepGMR's RRI columns) and returned tuples:
    (template, source, igt), with use_masknet and a partial side also the masks (template_mask before source_mask).  `data_class` is any
    dataset of (cloud [N,C], label), e.g. data_utils.ModelNet40Data; it has no default here (the reference builds one at import).
    Each sample crosses to the device and back; ResidentRegistrationFeed does the same work for whole batches without the host."""

    def __init__(self, algorithm, data_class, partial_source=False, partial_template=False, noise=False, additional_params={}):
        super().__init__()
        self.algorithm = algorithm
        self.transforms = transform_for(algorithm, len(data_class))
        self.set_class(data_class)
        self.partial_template, self.partial_source, self.noise = partial_template, partial_source, noise
        self.additional_params = additional_params
        self.use_rri = False
        if algorithm == 'DeepGMR' and additional_params.get('nearest_neighbors', 0) > 0:
            self.use_rri = True
            self.nearest_neighbors = additional_params['nearest_neighbors']

    def __len__(self):
        return len(self.data_class)

    def set_class(self, data_class):
        self.data_class = data_class

    def __getitem__(self, index):
        from .device_feed import with_rri
        template, label = self.data_class[index]
        self.transforms.index = index                                  # for fixed transformations in PCRNet
        source = self.transforms(template)
        back = not source.is_cuda
        if self.additional_params.get('partial_point_cloud_method', None) == 'planar_crop':
            # the reference crops both clouds on this path whatever the partial_* flags say; the normals are drawn here, in its order,
            # so that both crops and the intersection of their index lists (:299-304) stay on the device
            normals = (uniform_2_sphere(), uniform_2_sphere()) if back else (None, None)
            num = max(source.shape[0], template.shape[0])
            source, gt_idx_source = planar_crop(_on_gpu(source)[0], normal=normals[0])
            template, gt_idx_template = planar_crop(_on_gpu(template)[0], normal=normals[1])
            t_mask, s_mask = intersection_masks(gt_idx_source[None], gt_idx_template[None], num)
            self.template_mask, self.source_mask = t_mask[0], s_mask[0]
            if back:
                source, template, self.template_mask, self.source_mask = source.cpu(), template.cpu(), t_mask[0].cpu(), s_mask[0].cpu()
        else:
            if self.partial_source:
                source, self.source_mask = farthest_subsample_points(source)
            if self.partial_template:
                template, self.template_mask = farthest_subsample_points(template)
        if self.noise:
            source = jitter_pointcloud(source)
        if self.use_rri:
            template, source = (with_rri(_on_gpu(t)[0][None], self.nearest_neighbors)[0] for t in (template, source))
            if back:
                template, source = template.cpu(), source.cpu()
        igt = self.transforms.igt
        if self.additional_params.get('use_masknet', False):
            if self.partial_source and self.partial_template:
                return template, source, igt, self.template_mask, self.source_mask
            elif self.partial_source:
                return template, source, igt, self.source_mask
            elif self.partial_template:
                return template, source, igt, self.template_mask
        else:
            return template, source, igt
