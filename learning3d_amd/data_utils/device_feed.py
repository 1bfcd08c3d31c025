"""Synthetic registration batches generated entirely on the device.

reference: data_utils/dataloaders.py:250-330 (RegistrationData: template from the dataset, source = transform(template),
igt from the transform) with ops/transform_functions.py:271-315 as the transform; one sample at a time on host cores.
RegistrationFeed yields whole batches {template, source, igt} without a host tensor or a copy: clouds from
l3d_uniform_clouds (seeded by (seed, batch index, element)), rigid transforms from DCPTransform (l3d_euler_transform).
"""
import torch

from .._lib import call
from .. import _lib
from ..ops.transform_functions import DCPTransform
from . import partial as _partial
from .rri import rri_features


def with_rri(cloud, k):
    """cloud [B,N,3] -> [B,N,3+4k]: DeepGMR's input format, the RRI features of the centred cloud behind the coordinates (reference:
    data_utils/dataloaders.py:314-317); k None: the cloud itself"""
    return cloud if k is None else torch.cat([cloud, rri_features(cloud, k, center=True)], dim=2)


def uniform_clouds(batch, num_points, lo=0.0, hi=1.0, seed=0, device="cuda"):
    """[batch, num_points, 3] ~ U(lo, hi) generated on `device` (reproducible in (seed, shape))."""
    out = torch.empty((batch, num_points, 3), dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        call("l3d_uniform_clouds", int(seed), batch, num_points, float(lo), float(hi), out)
    return out


class RegistrationFeed:
    """Iterator of device batches for DCP-style registration: (template [B,N,3], source [B,N,3], igt [B,4,4]).
    rri_neighbors=k: both clouds as [B,N,3+4k], DeepGMR's input (the same clouds and igt as without it)."""

    def __init__(self, batch_size, num_points=1024, angle_range=45, translation_range=1, lo=-0.5, hi=0.5, seed=0,
                 device="cuda", length=None, rri_neighbors=None):
        self.batch_size, self.num_points, self.rri_neighbors = batch_size, num_points, rri_neighbors
        self.lo, self.hi, self.seed, self.device, self.length = lo, hi, seed, torch.device(device), length
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)
        self.transform = DCPTransform(angle_range, translation_range, generator=gen)
        self._i = 0

    def __iter__(self):
        return self

    def __next__(self):
        if self.length is not None and self._i >= self.length:
            raise StopIteration
        template = uniform_clouds(self.batch_size, self.num_points, self.lo, self.hi,
                                  seed=(self.seed << 20) + self._i, device=self.device)
        source = self.transform(template)
        self._i += 1
        return with_rri(template, self.rri_neighbors), with_rri(source, self.rri_neighbors), self.transform.igt


class ResidentRegistrationFeed:
    """RegistrationData over a dataset that lives in HBM (reference: data_utils/dataloaders.py:184-227 ModelNet40Data --
    `data[idx][:num_points]`, optional per-sample point shuffle -- and :250-330 RegistrationData -- source =
    transform(template)).  ModelNet40's 9840 x 2048 x 3 training clouds are 242 MB: they fit once, and every batch is an
    index gather + one transform launch on the device -- no DataLoader workers, no host tensor, no copy per step.

    data [M,P,3] device tensor (labels [M] optional); `transform` is any of the device transforms of
    ops/transform_functions.py (DCPTransform by default).  Yields (template [B,N,3], source [B,N,3], igt, labels or None);
    one epoch = every cloud once, in a permutation seeded by (seed, epoch).  rri_neighbors=k: both clouds as [B,N,3+4k],
    DeepGMR's input (the same clouds and igt as without it).

    Partial and noisy pairs (reference :296-330; all off by default, and then the tuple and every value are what they are without
    them).  partial_source / partial_template: that cloud is cropped to its num_subsampled_points points nearest a far view point,
    nearest first (farthest_subsample_points).  partial_method='planar_crop': BOTH clouds are cropped by a random plane through their
    centroid instead, 70 % kept, in index order, as the reference does whatever the two flags say.  noise: jitter_pointcloud on the
    source.  masks: the reference's use_masknet -- the tuple grows behind the labels by template_mask, source_mask (those of the
    cropped sides; nearest: 1.0 at the kept points of the FULL cloud [B,N]; planar: over the KEPT points [B,K], 1.0 where the point
    was kept on the other side too).  A batch is the transform launch plus one l3d_crop_select per cropped cloud, the jitter fused
    into the source's; the draws come from the feed's device generator and nothing is read on the host."""

    def __init__(self, data, labels=None, batch_size=32, num_points=1024, transform=None, randomize_points=False, seed=0,
                 drop_last=True, rri_neighbors=None, *, partial_source=False, partial_template=False, num_subsampled_points=768,
                 partial_method="farthest", noise=False, masks=False):
        if not (data.is_cuda and data.dim() == 3 and data.shape[2] == 3):
            raise ValueError("data must be a device tensor [M, P, 3]")
        if num_points > data.shape[1]:
            raise ValueError("num_points exceeds the points per cloud of the dataset")
        self.data, self.labels = data.float().contiguous(), labels
        self.batch_size, self.num_points, self.randomize_points, self.drop_last = batch_size, num_points, randomize_points, drop_last
        self.gen = torch.Generator(device=data.device)
        self.seed, self.epoch, self.rri_neighbors = seed, 0, rri_neighbors
        self.transform = transform if transform is not None else DCPTransform(45, 1, generator=self.gen)
        if partial_method not in ("farthest", "planar_crop"):
            raise ValueError("partial_method is 'farthest' or 'planar_crop'")
        planar = partial_method == "planar_crop"
        kept = _partial.plane_keep_count(num_points) if planar else num_subsampled_points
        if (partial_source or partial_template or planar) and not 1 <= kept <= num_points:
            raise ValueError("the number of points kept must lie in 1 .. num_points")
        self.partial_source, self.partial_template, self.planar = bool(partial_source or planar), bool(partial_template or planar), planar
        self.num_kept, self.noise, self.masks = kept, bool(noise), bool(masks)

    @classmethod
    def for_algorithm(cls, name, data, labels=None, **kw):
        """the feed with the transform RegistrationData gives algorithm `name` ('DCP', 'PRNet', 'PointNetLK', 'RPMNet', 'PCRNet',
        'iPCRNet', 'DeepGMR'), drawing from the feed's generator; every other argument as the constructor's"""
        if "transform" in kw:
            raise TypeError("for_algorithm chooses the transform")
        feed = cls(data, labels, **kw)
        feed.transform = _partial.transform_for(name, None, generator=feed.gen)
        return feed

    def draw_partial(self, batch):
        """the draws of one batch's crops and jitter, from the feed's generator: a dict of device tensors (crop_batch's `draws`)"""
        dev, d = self.data.device, {}
        for side, on in (("source", self.partial_source), ("template", self.partial_template)):
            if on:
                d[side] = _partial.uniform_2_sphere(batch, dev, self.gen) if self.planar else _partial.draw_views(batch, dev, self.gen)
        if self.noise:
            rows = self.num_kept if self.partial_source else self.num_points
            d["sigma"] = _partial.JITTER_SCALE * torch.rand((batch,), device=dev, generator=self.gen)
            d["noise"] = torch.randn((batch, rows, 3), device=dev, generator=self.gen)
        return d

    def crop_batch(self, template, source, draws):
        """(template [B,N,3], source = transform(template), draw_partial's dict) -> (template, source, masks): the crops, the jitter and
        the masks of the options -- launches only, no draw and no host read (it can be captured into a graph).  masks: () unless
        asked for, else (template_mask, source_mask) of the cropped sides."""
        mode = _lib.L3D_CROP_PLANE if self.planar else _lib.L3D_CROP_NEAREST
        N, found = template.shape[1], {}
        for side, cloud, on in (("source", source, self.partial_source), ("template", template, self.partial_template)):
            jitter = dict(noise=draws["noise"], sigma=draws["sigma"], clip=0.05) if (self.noise and side == "source") else {}
            if on:
                found[side] = _partial.crop_select(cloud, draws[side], mode, self.num_kept, centre=cloud.mean(dim=1) if self.planar else None,
                                                   want_idx=self.planar and self.masks, want_mask=self.masks and not self.planar, **jitter)
            elif jitter:
                found[side] = _partial.crop_select(cloud, None, _lib.L3D_CROP_PLANE, N, want_idx=False, want_mask=False, **jitter)
        if "source" in found:
            source = found["source"][2]
        if "template" in found:
            template = found["template"][2]
        if not self.masks:
            return template, source, ()
        if self.planar:
            return template, source, _partial.intersection_masks(found["source"][0], found["template"][0], N)
        return template, source, tuple(found[side][1] for side, on in (("template", self.partial_template), ("source", self.partial_source)) if on)

    def __len__(self):
        M = self.data.shape[0]
        return M // self.batch_size if self.drop_last else -(-M // self.batch_size)

    def __iter__(self):
        self.gen.manual_seed((self.seed << 20) + self.epoch)
        self.epoch += 1
        perm = torch.randperm(self.data.shape[0], device=self.data.device, generator=self.gen)
        for i in range(len(self)):
            idx = perm[i * self.batch_size:(i + 1) * self.batch_size]
            if self.randomize_points:                          # ModelNet40Data.randomize (:214-216): shuffle, then keep the first N
                order = torch.rand((idx.numel(), self.data.shape[1]), device=self.data.device, generator=self.gen).argsort(dim=1)
                template = torch.gather(self.data[idx], 1, order[:, :self.num_points, None].expand(-1, -1, 3)).contiguous()
            else:
                template = self.data[idx, :self.num_points].contiguous()
            source = self.transform(template)
            masks = ()
            if self.partial_source or self.partial_template or self.noise:
                template, source, masks = self.crop_batch(template, source, self.draw_partial(template.shape[0]))
            yield (with_rri(template, self.rri_neighbors), with_rri(source, self.rri_neighbors), self.transform.igt,
                   (self.labels[idx] if self.labels is not None else None), *masks)
