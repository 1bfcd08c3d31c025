"""The on-disk half of the data feed: ModelNet40 and FlyingThings3D readers that put the WHOLE dataset
in HBM once and serve batches from there.

reference: data_utils/dataloaders.py
  :31-48    load_data           ply_data_{train,test}*.h5 -> data [M,2048,3(+3)] float32, label [M,1] int64
  :184-227  ModelNet40Data      __getitem__: data[idx][:num_points] (or a shuffle of the first num_points rows), label
  :230-247  ClassificationData  (points, label)
  :364-435  SceneflowDataset    TRAIN*/TEST*.npz -> random (train) or leading (test) npoints rows of both clouds, colours, flow,
                                mask; both clouds minus the mean of the sampled first cloud
behind a torch DataLoader with host workers.  At 10^4..10^5 clouds/s that path starves the GPU; the
datasets are small next to 288 GB of HBM (ModelNet40 train: 242 MB; the processed FlyingThings3D set: ~10 GB), so here

  disk -> numpy (np.load; the h5 files through a one-off converter, tools/modelnet40_h5_to_npz.py: h5py is not in this
          image) -> ONE pinned host buffer per array -> ONE asynchronous H2D copy -> resident tensors
  batch = index gather on the device (ModelNet40: l3d_index_points-style row gather; scene flow: l3d_sceneflow_batch, which
          also replays np.mean's summation order so the centred clouds are bit-identical to the reference's)

Two layers, as everywhere in this package:
  * `ModelNet40Data`, `ClassificationData`, `SceneflowDataset`: drop-in Dataset classes with the reference's constructor
    arguments, `__getitem__` results and numpy RNG call sequence (host arrays in, host tensors out) -- what the golden test
    compares with the reference's own classes;
  * `ResidentModelNet40`, `ResidentSceneflow`: the device feeds built on the same arrays.
"""
import glob
import os

import numpy as np
import torch

from .._lib import call

MODELNET_DIR = "modelnet40_ply_hdf5_2048"
SCENEFLOW_DIR = "data_processed_maxcut_35_20k_2k_8192"


def default_data_dir():
    """<package>/../data, where the reference keeps its datasets (dataloaders.py:20-21, :33-34)"""
    return os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "data")


# ----------------------------------------------------------------------------------------------------------- ModelNet40
def load_modelnet40(train, use_normals=False, root=None):
    """dataloaders.py:31-48 on the converted files: every `ply_data_{train|test}*.npz` under <root>/modelnet40_ply_hdf5_2048
    (keys `data`, `label`, optional `normal`, exactly the h5 datasets; tools/modelnet40_h5_to_npz.py writes them), concatenated
    in sorted file order (the reference's glob order is the file system's).  -> (data float32 [M,P,3|6], label int64 [M,1])"""
    root = root or default_data_dir()
    part = "train" if train else "test"
    files = sorted(glob.glob(os.path.join(root, MODELNET_DIR, f"ply_data_{part}*.npz")))
    if not files:
        raise FileNotFoundError(
            f"no ply_data_{part}*.npz under {os.path.join(root, MODELNET_DIR)}: convert the reference's h5 files once with "
            "tools/modelnet40_h5_to_npz.py (h5py is needed only there)")
    all_data, all_label = [], []
    for fn in files:
        with np.load(fn) as f:
            data = np.concatenate([f["data"][:], f["normal"][:]], axis=-1).astype("float32") if use_normals else f["data"][:].astype("float32")
            all_data.append(data)
            all_label.append(f["label"][:].astype("int64"))
    return np.concatenate(all_data, axis=0), np.concatenate(all_label, axis=0)


def read_classes_modelnet40(root=None):
    """dataloaders.py:221-227"""
    with open(os.path.join(root or default_data_dir(), MODELNET_DIR, "shape_names.txt"), "r") as f:
        return np.array(f.read().split("\n")[:-1])


class ModelNet40Data(torch.utils.data.Dataset):
    """Drop-in for data_utils/dataloaders.py:184-227 (download=... is accepted and ignored: there is no network; `root` is
    where the converted files live)."""

    def __init__(self, train=True, num_points=1024, download=False, randomize_data=False, use_normals=False, root=None):
        super().__init__()
        self.data, self.labels = load_modelnet40(train, use_normals, root)
        if not train:
            self.shapes = read_classes_modelnet40(root)
        self.num_points = num_points
        self.randomize_data = randomize_data

    def __getitem__(self, idx):
        current_points = self.randomize(idx) if self.randomize_data else self.data[idx].copy()
        current_points = torch.from_numpy(current_points[:self.num_points, :]).float()
        label = torch.from_numpy(self.labels[idx]).type(torch.LongTensor)
        return current_points, label

    def __len__(self):
        return self.data.shape[0]

    def randomize(self, idx):
        pt_idxs = np.arange(0, self.num_points)
        np.random.shuffle(pt_idxs)
        return self.data[idx, pt_idxs].copy()

    def get_shape(self, label):
        return self.shapes[label]


class ClassificationData(torch.utils.data.Dataset):
    """dataloaders.py:230-247"""

    def __init__(self, data_class):
        super().__init__()
        self.set_class(data_class)

    def __len__(self):
        return len(self.data_class)

    def set_class(self, data_class):
        self.data_class = data_class

    def get_shape(self, label):
        try:
            return self.data_class.get_shape(label)
        except Exception:
            return -1

    def __getitem__(self, index):
        return self.data_class[index]


def _to_device_once(arrays, device):
    """host arrays -> pinned staging buffers -> one asynchronous copy each on the current stream -> device tensors"""
    out = []
    for a in arrays:
        t = torch.from_numpy(np.ascontiguousarray(a))
        out.append(t.pin_memory().to(device, non_blocking=True) if torch.cuda.is_available() else t)
    return out


class ResidentModelNet40:
    """ModelNet40Data / ClassificationData served from HBM: (points [B,num_points,C], label [B,1]) per batch; one epoch is a
    seeded permutation of the clouds.  `batch(idx)` gives the reference's `__getitem__` rows for explicit cloud indices (no
    point shuffle) -- identical values, a whole batch per launch."""

    def __init__(self, train=True, num_points=1024, batch_size=32, randomize_data=False, use_normals=False, root=None, device="cuda",
                 seed=0, drop_last=True, arrays=None):
        data, labels = arrays if arrays is not None else load_modelnet40(train, use_normals, root)
        self.device = torch.device(device)
        self.data, self.labels = _to_device_once([data, labels], self.device)
        self.num_points, self.batch_size, self.randomize_data, self.drop_last = num_points, batch_size, randomize_data, drop_last
        self.gen = torch.Generator(device=self.device)
        self.seed, self.epoch = seed, 0

    def __len__(self):
        M = self.data.shape[0]
        return M // self.batch_size if self.drop_last else -(-M // self.batch_size)

    def batch(self, idx, order=None):
        """idx int64 [B] (device) -> (points, labels); order [B,num_points] int64: the per-cloud row permutation of
        ModelNet40Data.randomize (rows of the FIRST num_points points), None = data[idx][:num_points]"""
        rows = self.data[idx, :self.num_points]
        if order is not None:
            rows = torch.gather(rows, 1, order[:, :, None].expand(-1, -1, rows.shape[2]))
        return rows.contiguous(), self.labels[idx]

    def __iter__(self):
        self.gen.manual_seed((self.seed << 20) + self.epoch)
        self.epoch += 1
        perm = torch.randperm(self.data.shape[0], device=self.device, generator=self.gen)
        for i in range(len(self)):
            idx = perm[i * self.batch_size:(i + 1) * self.batch_size]
            order = None
            if self.randomize_data:
                order = torch.rand((idx.numel(), self.num_points), device=self.device, generator=self.gen).argsort(dim=1)
            yield self.batch(idx, order)


# ----------------------------------------------------------------------------------------------------- FlyingThings3D
_SF_KEYS = ("points1", "points2", "color1", "color2", "flow", "valid_mask1")


def list_sceneflow_files(root, partition):
    """dataloaders.py:378-387 (glob TRAIN*/TEST*.npz, minus the one file with NaNs), in sorted order"""
    pat = "TRAIN*.npz" if partition == "train" else "TEST*.npz"
    return [d for d in sorted(glob.glob(os.path.join(root, pat))) if "TRAIN_C_0140_left_0006-0" not in d]


def load_sceneflow_file(fn):
    """dataloaders.py:396-404"""
    with open(fn, "rb") as fp:
        data = np.load(fp)
        return (data["points1"].astype("float32"), data["points2"].astype("float32"), data["color1"].astype("float32"),
                data["color2"].astype("float32"), data["flow"].astype("float32"), data["valid_mask1"])


class SceneflowDataset(torch.utils.data.Dataset):
    """Drop-in for data_utils/dataloaders.py:364-435: same arguments, same numpy RNG call sequence, same outputs."""

    def __init__(self, npoints=1024, root="", partition="train"):
        if root == "":
            root = os.path.join(default_data_dir(), SCENEFLOW_DIR)
            if not os.path.exists(root):
                raise FileNotFoundError(f"{root} not found (the reference prints a download link and exits here, dataloaders.py:370-373)")
        self.npoints, self.partition, self.root = npoints, partition, root
        self.datapath = list_sceneflow_files(root, partition)
        self.cache, self.cache_size = {}, 30000

    def __getitem__(self, index):
        if index in self.cache:
            pos1, pos2, color1, color2, flow, mask1 = self.cache[index]
        else:
            pos1, pos2, color1, color2, flow, mask1 = load_sceneflow_file(self.datapath[index])
            if len(self.cache) < self.cache_size:
                self.cache[index] = (pos1, pos2, color1, color2, flow, mask1)
        if self.partition == "train":
            sample_idx1 = np.random.choice(pos1.shape[0], self.npoints, replace=False)
            sample_idx2 = np.random.choice(pos2.shape[0], self.npoints, replace=False)
            pos1, pos2 = pos1[sample_idx1, :], pos2[sample_idx2, :]
            color1, color2 = color1[sample_idx1, :], color2[sample_idx2, :]
            flow, mask1 = flow[sample_idx1, :], mask1[sample_idx1]
        else:
            pos1, pos2 = pos1[:self.npoints, :], pos2[:self.npoints, :]
            color1, color2 = color1[:self.npoints, :], color2[:self.npoints, :]
            flow, mask1 = flow[:self.npoints, :], mask1[:self.npoints]
        pos1_center = np.mean(pos1, 0)
        pos1 = pos1 - pos1_center
        pos2 = pos2 - pos1_center
        return pos1, pos2, color1, color2, flow, mask1

    def __len__(self):
        return len(self.datapath)


class ResidentSceneflow:
    """SceneflowDataset served from HBM.  All scenes must hold the same number of points per cloud (the processed set does:
    8192).  `batch(scene_idx, sample1, sample2)` = the reference's `__getitem__` for explicit scenes and row samples, one
    launch (l3d_sceneflow_batch); iteration draws the scene permutation and the without-replacement row samples on the device.
    Yields (pos1, pos2, color1, color2, flow [B,npoints,3] float32, mask1 [B,npoints] bool)."""

    def __init__(self, npoints=1024, root="", partition="train", batch_size=32, device="cuda", seed=0, drop_last=True, arrays=None):
        if arrays is None:
            if root == "":
                root = os.path.join(default_data_dir(), SCENEFLOW_DIR)
            files = list_sceneflow_files(root, partition)
            if not files:
                raise FileNotFoundError(f"no {'TRAIN' if partition == 'train' else 'TEST'}*.npz under {root}")
            per_file = [load_sceneflow_file(fn) for fn in files]
            if len({(p[0].shape, p[1].shape) for p in per_file}) != 1:
                raise ValueError("scenes with different point counts cannot share one resident array")
            arrays = [np.stack([p[i] for p in per_file]) for i in range(6)]
        arrays = list(arrays)
        arrays[5] = np.ascontiguousarray(arrays[5]).astype(np.uint8)            # numpy bool -> bytes
        self.device = torch.device(device)
        self.p1, self.p2, self.c1, self.c2, self.flow, self.mask = _to_device_once(arrays, self.device)
        self.npoints, self.partition, self.batch_size, self.drop_last = npoints, partition, batch_size, drop_last
        self.gen = torch.Generator(device=self.device)
        self.seed, self.epoch = seed, 0
        if npoints > min(self.p1.shape[1], self.p2.shape[1]) or npoints > 8192:
            raise ValueError("npoints exceeds the points per scene (or the kernel's 8192)")

    def __len__(self):
        F = self.p1.shape[0]
        return F // self.batch_size if self.drop_last else -(-F // self.batch_size)

    def batch(self, scene_idx, sample1=None, sample2=None):
        B, S = scene_idx.numel(), self.npoints
        dev = self.device
        o = [torch.empty((B, S, 3), dtype=torch.float32, device=dev) for _ in range(5)]
        om = torch.empty((B, S), dtype=torch.uint8, device=dev)
        s1 = sample1.to(torch.int32).contiguous() if sample1 is not None else None
        s2 = sample2.to(torch.int32).contiguous() if sample2 is not None else None
        with torch.cuda.device(dev):
            call("l3d_sceneflow_batch", self.p1, self.p2, self.c1, self.c2, self.flow, self.mask, scene_idx.to(torch.int64).contiguous(),
                 s1, s2, B, self.p1.shape[1], self.p2.shape[1], S, *o, om)
        return o[0], o[1], o[2], o[3], o[4], om.bool()

    def __iter__(self):
        self.gen.manual_seed((self.seed << 20) + self.epoch)
        self.epoch += 1
        F = self.p1.shape[0]
        perm = torch.randperm(F, device=self.device, generator=self.gen) if self.partition == "train" else torch.arange(F, device=self.device)
        for i in range(len(self)):
            idx = perm[i * self.batch_size:(i + 1) * self.batch_size]
            if self.partition == "train":                      # np.random.choice(n, npoints, replace=False): a random permutation's prefix
                s1 = torch.rand((idx.numel(), self.p1.shape[1]), device=self.device, generator=self.gen).argsort(dim=1)[:, :self.npoints]
                s2 = torch.rand((idx.numel(), self.p2.shape[1]), device=self.device, generator=self.gen).argsort(dim=1)[:, :self.npoints]
                yield self.batch(idx, s1, s2)
            else:
                yield self.batch(idx)
