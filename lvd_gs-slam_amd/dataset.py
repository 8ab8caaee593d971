"""The reference's datasets (utils/dataset.py): ``load_dataset(args, path, config)`` -> a ``MonocularDataset`` of the type the settings
name -- ``KITTI``, ``waymo``, ``dl3dv``, ``replica`` or ``tum`` -- with the reference's directory layouts and pose conventions, and the
contract ``SlamSequence`` / ``Camera.init_from_dataset`` read: ``dataset[idx] -> (image, depth, pose, mono_depth)`` plus the intrinsics.

    image       (3, H, W) float32 on ``device``: byte / 255, after the undistortion when the calibration says ``distorted``
    depth       first channel of the depth file / depth_scale, a host float64 array (as in the reference)
    mono_depth  first channel of the mono-depth file / (depth_scale * 5), a host float64 array
    pose        the float64 world-to-camera matrix on ``device``

A file is decoded once per frame: where the depth or mono-depth path IS the colour path (the KITTI and dl3dv placeholders) the decoded
colour frame serves (the reference decodes it up to three times).

``ingest="host"`` (the default) does the undistortion and the conversion in NumPy and uploads float32, and works without a GPU;
``ingest="fused"`` uploads the decoded bytes and makes one ``lvdgs_ingest_frame`` call (csrc/ingest.hip) -- 7.4 MB instead of 29.5 MB
over the bus for a 1920 x 1280 frame, no float64 frame on the host.  Both give the same bits: the arithmetic is fixed in
include/lvdgs.h.  Parity of the undistortion with the real ``cv2.remap`` is UNPINNED (OpenCV is not installed
where this was written).

``__getitem__`` is ``assemble(read(idx))``, a host half and a device half, so that ``FramePrefetcher`` can run the host half of the next
frames on worker threads while the loops work (the reference's loader is serial); ``planes="device"`` also makes the float32 depth
planes on the device (``lvdgs_ingest_depth``) and hands them to the loops beside the host arrays.  Both are opt-in.

Deviations from the reference: ``device`` is a keyword (default ``"cuda:0"``), not hard-coded; a calibration without ``depth_scale``
raises ``ValueError`` at construction (the reference hits an unbound name in ``__getitem__``); a colour file that does not decode to
three 8-bit channels is refused; the RealSense live class is out of scope."""
import ctypes as C
import glob
import json
import os
import queue
import threading

import numpy as np
import torch
from PIL import Image
from scipy.spatial.transform import Rotation

from . import _lib
from .graphics_utils import focal2fov

MAP_OUTSIDE = _lib.MAP_OUTSIDE
_MAP_LIMIT = np.float32(2.0 ** 20)


# ---- the arithmetic of include/lvdgs.h on the host ----
def undistort_map_host(width, height, fx, fy, cx, cy, dist):
    """(sx, sy), int32 (H, W): the fixed-point undistortion map of include/lvdgs.h, in NumPy float64."""
    k1, k2, p1, p2, k3 = (float(d) for d in dist)
    fx, fy, cx, cy = float(fx), float(fy), float(cx), float(cy)
    u = np.arange(int(width), dtype=np.float64)[None, :]
    v = np.arange(int(height), dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        x = np.broadcast_to((u - cx) / fx, (height, width))
        y = np.broadcast_to((v - cy) / fy, (height, width))
        r2 = x * x + y * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        out = []
        for m in ((fx * xd + cx).astype(np.float32), (fy * yd + cy).astype(np.float32)):
            inside = np.abs(m) < _MAP_LIMIT                       # False for NaN and the infinities
            s = np.rint(np.where(inside, m, np.float32(0)) * np.float32(32))   # m * 32 is exact; rint rounds ties to even
            out.append(np.where(inside, s.astype(np.int32), np.int32(MAP_OUTSIDE)))
    return out[0], out[1]


def remap_host(image, sx, sy):
    """The bilinear remap of include/lvdgs.h: ``image`` (H, W, 3) uint8 through the map ``(sx, sy)`` -> (H, W, 3) uint8."""
    H, W = image.shape[:2]
    valid = (sx != MAP_OUTSIDE) & (sy != MAP_OUTSIDE)
    ix, ax, iy, ay = sx >> 5, sx & 31, sy >> 5, sy & 31
    acc = np.zeros((H, W, 3), np.int32)
    for dx, dy, w in ((0, 0, (32 - ax) * (32 - ay)), (1, 0, ax * (32 - ay)), (0, 1, (32 - ax) * ay), (1, 1, ax * ay)):
        xx, yy = ix + dx, iy + dy
        inside = valid & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        px = image[np.where(inside, yy, 0), np.where(inside, xx, 0)].astype(np.int32)
        acc += np.where(inside, w, 0).astype(np.int32)[..., None] * px
    return ((acc + 512) >> 10).astype(np.uint8)


def convert_host(image):
    """(H, W, 3) uint8 -> (3, H, W) float32, contiguous: (float)((double)byte / 255.0)."""
    return np.ascontiguousarray((image.astype(np.float64) / 255.0).astype(np.float32).transpose(2, 0, 1))


def convert_depth_host(samples, divisor):
    """uint8 / uint16 samples -> float32: (float)((double)sample / divisor), the arithmetic of ``lvdgs_ingest_depth`` (include/lvdgs.h).
    It is the reference's float64 division followed by the cast to float32 every consumer of a depth plane applies."""
    samples = np.asarray(samples)
    if samples.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"convert_depth_host: samples must be uint8 or uint16, got {samples.dtype}")
    return (samples.astype(np.float64) / float(divisor)).astype(np.float32)


# ---- the device entry points ----
def _gpu(device, what):
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.LvdgsError(f"{what}: needs a GPU device, got {device} (ingest='host' is the mode that runs without one)")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def undistort_map_device(width, height, fx, fy, cx, cy, dist, device):
    """(sx, sy), int32 (H, W) on ``device``: one ``lvdgs_undistort_map`` call, no wait."""
    device = _gpu(device, "undistort_map_device")
    coeffs = (C.c_double * 5)(*[float(d) for d in dist])
    sx = torch.empty((int(height), int(width)), dtype=torch.int32, device=device)
    sy = torch.empty_like(sx)
    with _lib.on_device(device):
        _lib.check(_lib.lib().lvdgs_undistort_map(int(width), int(height), float(fx), float(fy), float(cx), float(cy), coeffs,
                                                  sx.data_ptr(), sy.data_ptr(), _lib.raw_stream(device)), "lvdgs_undistort_map")
    return sx, sy


def ingest_frame(src, sx=None, sy=None, *, want_u8=False):
    """One ``lvdgs_ingest_frame`` call: ``src`` (H, W, 3) uint8 on a GPU -- its rows may lie apart (a row stride of at least 3 W bytes), its
    pixels may not -- and optionally the map ``(sx, sy)`` of ``undistort_map_device`` -> the (3, H, W) float32 image; with ``want_u8`` also
    the (H, W, 3) bytes after the remap.  No host wait, no copy."""
    if not torch.is_tensor(src) or not src.is_cuda or src.dtype is not torch.uint8:
        raise _lib.LvdgsError("ingest_frame: src must be a uint8 tensor on a GPU (there is no CPU path)")
    if src.ndim != 3 or src.shape[2] != 3 or src.shape[0] < 1 or src.shape[1] < 1:
        raise ValueError(f"ingest_frame: src must be (H, W, 3) with H, W > 0, got {tuple(src.shape)}")
    H, W = int(src.shape[0]), int(src.shape[1])
    if src.stride(2) != 1 or src.stride(1) != 3 or (H > 1 and src.stride(0) < 3 * W):
        src = src.contiguous()
    pitch = int(src.stride(0)) if H > 1 else 3 * W
    if (sx is None) != (sy is None):
        raise ValueError("ingest_frame: sx and sy come together")
    device = src.device
    for m in (sx, sy):
        if m is not None and not (torch.is_tensor(m) and m.device == device and m.dtype is torch.int32 and m.is_contiguous() and tuple(m.shape) == (H, W)):
            raise ValueError("ingest_frame: sx / sy must be contiguous int32 (H, W) tensors on the frame's device")
    image = torch.empty((3, H, W), dtype=torch.float32, device=device)
    u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=device) if want_u8 else None
    a = _lib.IngestArgs(width=W, height=H, src=src.data_ptr(), src_row_bytes=pitch, map_sx=_lib.ptr(sx), map_sy=_lib.ptr(sy),
                        image=image.data_ptr(), image_u8=_lib.ptr(u8))
    with _lib.on_device(device):
        _lib.check(_lib.lib().lvdgs_ingest_frame(C.byref(a), _lib.raw_stream(device)), "lvdgs_ingest_frame")
    return (image, u8) if want_u8 else image


_WORD_DTYPES = tuple(d for d in (torch.int16, getattr(torch, "uint16", None)) if d is not None)


def ingest_depth(src, divisor):
    """One ``lvdgs_ingest_depth`` call: ``src`` (H, W) on a GPU, uint8 or 16-bit (int16 is read as unsigned: the bits of a uint16 file) --
    a view with a pixel and a row stride is taken as it is, e.g. ``frame[:, :, 0]`` of a frame's colour bytes -- and the divisor -> the
    (H, W) float32 plane ``(float)((double)sample / divisor)``.  No host wait, no copy."""
    if not torch.is_tensor(src) or not src.is_cuda or (src.dtype is not torch.uint8 and src.dtype not in _WORD_DTYPES):
        raise _lib.LvdgsError("ingest_depth: src must be a uint8 or 16-bit integer tensor on a GPU (there is no CPU path)")
    if src.ndim != 2 or src.shape[0] < 1 or src.shape[1] < 1:
        raise ValueError(f"ingest_depth: src must be (H, W) with H, W > 0, got {tuple(src.shape)}")
    H, W = int(src.shape[0]), int(src.shape[1])
    size = src.element_size()
    if (W > 1 and src.stride(1) < 1) or (H > 1 and src.stride(0) < W * max(src.stride(1), 1)):
        src = src.contiguous()
    stride = size * int(src.stride(1)) if W > 1 else size
    pitch = size * int(src.stride(0)) if H > 1 else W * stride
    out = torch.empty((H, W), dtype=torch.float32, device=src.device)
    a = _lib.IngestDepthArgs(width=W, height=H, src=src.data_ptr(), sample_type=_lib.DEPTH_SAMPLE_BYTE if size == 1 else _lib.DEPTH_SAMPLE_WORD,
                             pixel_stride=stride, src_row_bytes=pitch, divisor=float(divisor), out=out.data_ptr())
    with _lib.on_device(src.device):
        _lib.check(_lib.lib().lvdgs_ingest_depth(C.byref(a), _lib.raw_stream(src.device)), "lvdgs_ingest_depth")
    return out


# ---- parsers: which files make a sequence, and the world-to-camera pose of each frame ----
def _homogeneous(rotation, translation):
    T = np.eye(4)
    T[:3, :3] = rotation
    T[:3, 3] = translation
    return T


class KITTIParser:
    """``image_2/*.jpg`` (colour; also the depth and mono-depth placeholders) and one ``gt/*.txt`` per frame holding a 3 x 4
    camera-to-world matrix, both sorted and cut to ``[begin:end]``.  The first frame's translation is taken off every frame."""

    def __init__(self, input_folder, config):
        self.input_folder = input_folder
        self.begin, self.end = config["Dataset"]["begin"], config["Dataset"]["end"]
        self.color_paths = sorted(glob.glob(os.path.join(input_folder, "image_2", "*.jpg")))[self.begin:self.end]
        self.depth_paths = list(self.color_paths)
        self.mono_depth_paths = list(self.color_paths)
        self.n_img = len(self.color_paths)
        pose_files = sorted(glob.glob(os.path.join(input_folder, "gt", "*.txt")))[self.begin:self.end]
        if len(pose_files) < self.n_img:
            raise ValueError(f"{input_folder}: {self.n_img} frames but {len(pose_files)} pose files")
        self.poses = []
        origin = None
        for f in pose_files[:self.n_img]:
            arr = np.loadtxt(f, delimiter=" ")
            if arr.size != 12:
                raise ValueError(f"{f}: a pose file holds 12 numbers, this one {arr.size}")
            c2w = np.eye(4)
            c2w[:3, :] = arr.reshape(3, 4)
            if origin is None:
                origin = c2w[:3, 3].copy()
            c2w[:3, 3] -= origin
            self.poses.append(np.linalg.inv(c2w))


class dl3dvParser:
    """``rgb/*.png`` (colour and both placeholders) and ``cameras.json``: a list of ``cam_quat`` (x, y, z, w) / ``cam_trans``
    camera-to-world entries.  Both are cut to ``[begin:end]``; the first kept translation is taken off every frame."""

    def __init__(self, input_folder, config):
        self.input_folder = input_folder
        self.begin, self.end = config["Dataset"]["begin"], config["Dataset"]["end"]
        self.color_paths = sorted(glob.glob(os.path.join(input_folder, "rgb", "*.png")))[self.begin:self.end]
        self.depth_paths = list(self.color_paths)
        self.mono_depth_paths = list(self.color_paths)
        self.n_img = len(self.color_paths)
        with open(os.path.join(input_folder, "cameras.json"), "r") as f:
            cameras = json.load(f)[self.begin:self.end]
        origin = np.array(cameras[0]["cam_trans"])
        self.poses = []
        for cam in cameras:
            qx, qy, qz, qw = cam["cam_quat"]
            c2w = _homogeneous(Rotation.from_quat([qx, qy, qz, qw]).as_matrix(), list(cam["cam_trans"]) - origin)
            self.poses.append(np.linalg.inv(c2w))


class WaymoParser:
    """``rgb/*.png``, ``depth/*.png``, ``mono_depth/*.png`` and one ``gt/*.txt`` per frame holding a 4 x 4 camera-to-world matrix."""

    def __init__(self, input_folder):
        self.input_folder = input_folder
        self.color_paths = sorted(glob.glob(os.path.join(input_folder, "rgb", "*.png")))
        self.depth_paths = sorted(glob.glob(os.path.join(input_folder, "depth", "*.png")))
        self.mono_depth_paths = sorted(glob.glob(os.path.join(input_folder, "mono_depth", "*.png")))
        self.n_img = len(self.color_paths)
        pose_files = sorted(glob.glob(os.path.join(input_folder, "gt", "*.txt")))
        if len(pose_files) < self.n_img:
            raise ValueError(f"{input_folder}: {self.n_img} frames but {len(pose_files)} pose files")
        self.poses = [np.linalg.inv(np.loadtxt(f, delimiter=" ").reshape(4, 4)) for f in pose_files[:self.n_img]]


class ReplicaParser:
    """``results/frame*.png``, ``results/depth*.png``, ``results/mono*.png`` and ``traj.txt``: one line of 16 numbers per frame, the
    4 x 4 camera-to-world matrix."""

    def __init__(self, input_folder):
        self.input_folder = input_folder
        self.color_paths = sorted(glob.glob(os.path.join(input_folder, "results", "frame*.png")))
        self.depth_paths = sorted(glob.glob(os.path.join(input_folder, "results", "depth*.png")))
        self.mono_depth_paths = sorted(glob.glob(os.path.join(input_folder, "results", "mono*.png")))
        self.n_img = len(self.color_paths)
        with open(os.path.join(input_folder, "traj.txt"), "r") as f:
            lines = f.readlines()
        self.poses = [np.linalg.inv(np.array(list(map(float, lines[i].split()))).reshape(4, 4)) for i in range(self.n_img)]


def tum_associate(tstamp_image, tstamp_depth, tstamp_pose, max_dt=0.08):
    """For every image time stamp the nearest depth and pose stamps; the triple (i, j, k) is kept when both lie closer than ``max_dt``."""
    tstamp_depth, tstamp_pose = np.asarray(tstamp_depth, np.float64), np.asarray(tstamp_pose, np.float64)
    out = []
    for i, t in enumerate(tstamp_image):
        j = int(np.argmin(np.abs(tstamp_depth - t)))
        k = int(np.argmin(np.abs(tstamp_pose - t)))
        if np.abs(tstamp_depth[j] - t) < max_dt and np.abs(tstamp_pose[k] - t) < max_dt:
            out.append((i, j, k))
    return out


def tum_subsample(tstamp_image, associations, frame_rate=32):
    """The associations kept at ``frame_rate``: the first, then each whose image stamp lies more than 1 / frame_rate behind the last kept."""
    kept = [0] if associations else []
    for n in range(1, len(associations)):
        if tstamp_image[associations[n][0]] - tstamp_image[associations[kept[-1]][0]] > 1.0 / frame_rate:
            kept.append(n)
    return kept


class TUMParser:
    """``rgb.txt``, ``depth.txt``, ``mono_depth.txt`` (time stamp, file) and ``groundtruth.txt`` or ``pose.txt`` (a header line, then
    time stamp, tx ty tz, qx qy qz qw: camera-to-world), associated by ``tum_associate`` and thinned by ``tum_subsample`` at 32 Hz.

    UNPINNED: the reference's parser does not run under the installed NumPy (it asks for ``np.unicode_``, gone in NumPy 2) and needs
    ``trimesh``, which is not installed; no golden could be taken from it.  The rotation comes from
    ``scipy.spatial.transform.Rotation.from_quat`` (x, y, z, w), the matrix ``trimesh.transformations.quaternion_matrix`` builds from
    (w, x, y, z) for a unit quaternion."""

    def __init__(self, input_folder, frame_rate=32):
        self.input_folder = input_folder
        pose_list = next((p for p in (os.path.join(input_folder, n) for n in ("groundtruth.txt", "pose.txt")) if os.path.isfile(p)), None)
        if pose_list is None:
            raise FileNotFoundError(f"{input_folder}: neither groundtruth.txt nor pose.txt")

        def read(name, skip=0):      # the rows of a list file as strings: `skip` lines dropped, then blank and '#' lines
            with open(name, "r") as f:
                rows = [line.split() for line in f.read().splitlines()[skip:] if line.strip() and not line.lstrip().startswith("#")]
            return np.array(rows, dtype=str).reshape(len(rows), -1)

        image_data = read(os.path.join(input_folder, "rgb.txt"))
        depth_data = read(os.path.join(input_folder, "depth.txt"))
        mono_data = read(os.path.join(input_folder, "mono_depth.txt"))
        pose_vecs = read(pose_list, 1).astype(np.float64)
        tstamp_image = image_data[:, 0].astype(np.float64)
        associations = tum_associate(tstamp_image, depth_data[:, 0].astype(np.float64), pose_vecs[:, 0])
        self.color_paths, self.depth_paths, self.mono_depth_paths, self.poses = [], [], [], []
        for n in tum_subsample(tstamp_image, associations, frame_rate):
            i, j, k = associations[n]
            self.color_paths.append(os.path.join(input_folder, str(image_data[i, 1])))
            self.depth_paths.append(os.path.join(input_folder, str(depth_data[j, 1])))
            self.mono_depth_paths.append(os.path.join(input_folder, str(mono_data[i, 1])))
            c2w = _homogeneous(Rotation.from_quat(pose_vecs[k][4:8]).as_matrix(), pose_vecs[k][1:4])
            self.poses.append(np.linalg.inv(c2w))
        self.n_img = len(self.color_paths)


# ---- the dataset classes ----
class BaseDataset(torch.utils.data.Dataset):
    def __init__(self, args, path, config, *, device="cuda:0"):
        self.args, self.path, self.config = args, path, config
        self.device = device
        self.dtype = torch.float32
        self.num_imgs = 999999

    def __len__(self):
        return self.num_imgs

    def __getitem__(self, idx):
        pass


def _first_channel(array):
    return array[:, :, 0] if array.ndim == 3 else array


class FrameRecord:
    """One frame between ``MonocularDataset.read`` and ``assemble``.  ``read`` fills the host half: ``raw`` (H, W, 3) uint8, ``depth`` and
    ``mono_depth`` (the float64 arrays of the 4-tuple), ``pose`` (the float64 matrix, a host array) and, for ``planes="device"``, the
    files' own samples (``depth_samples`` / ``mono_samples``: None where the path is the colour path; the same array where both paths
    are one file).  ``assemble`` adds ``frame`` (the 4-tuple ``dataset[idx]`` returns) and the (H, W) float32 device planes ``depth32``
    / ``mono_depth32`` (None with ``planes="host"``)."""
    __slots__ = ("idx", "raw", "depth", "mono_depth", "pose", "depth_samples", "mono_samples", "frame", "depth32", "mono_depth32", "ready")

    def __init__(self, idx, raw, depth, mono_depth, pose, depth_samples=None, mono_samples=None):
        self.idx, self.raw, self.depth, self.mono_depth, self.pose = idx, raw, depth, mono_depth, pose
        self.depth_samples, self.mono_samples = depth_samples, mono_samples
        self.frame = self.depth32 = self.mono_depth32 = None
        self.ready = None       # FramePrefetcher: the event after this frame's work on its side stream


def _upload(array, device):
    return torch.from_numpy(array).to(device)


class MonocularDataset(BaseDataset):
    """Calibration, the undistortion map and ``__getitem__`` (utils/dataset.py:263-344); the subclasses say which files.

    ``__getitem__`` is ``assemble(read(idx))``: ``read`` is the host half (decodes, the two float64 divisions; callable from any thread,
    it writes nothing shared), ``assemble`` the device half (the upload, ``ingest_image``, the pose tensor).  ``planes="device"``
    (needs ``ingest="fused"``): ``assemble`` also makes the float32 planes ``depth32`` / ``mono_depth32`` on the device by
    ``lvdgs_ingest_depth`` -- from the colour bytes already there for a placeholder path, else from the file's 8- or 16-bit samples,
    uploaded once -- and ``frame(idx)`` returns the record that carries them beside the unchanged 4-tuple."""

    def __init__(self, args, path, config, *, device="cuda:0", ingest="host", planes="host"):
        super().__init__(args, path, config, device=device)
        if ingest not in ("host", "fused"):
            raise ValueError(f"ingest: 'host' or 'fused', got {ingest!r}")
        if planes not in ("host", "device"):
            raise ValueError(f"planes: 'host' or 'device', got {planes!r}")
        if planes == "device" and ingest != "fused":
            raise ValueError("planes='device' needs ingest='fused': the planes are made from bytes that mode puts on the device")
        self.ingest, self.planes = ingest, planes
        cal = config["Dataset"]["Calibration"]
        self.fx, self.fy, self.cx, self.cy = cal["fx"], cal["fy"], cal["cx"], cal["cy"]
        self.width, self.height = cal["width"], cal["height"]
        self.fovx, self.fovy = focal2fov(self.fx, self.width), focal2fov(self.fy, self.height)
        self.K = np.array([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]])
        self.disorted = cal["distorted"]      # (the reference's spelling: the attribute other code reads)
        self.dist_coeffs = np.array([cal["k1"], cal["k2"], cal["p1"], cal["p2"], cal["k3"]])
        if "depth_scale" not in cal:
            raise ValueError("Dataset.Calibration.depth_scale is missing: the depth and mono-depth inputs cannot be scaled")
        self.has_depth = True
        self.depth_scale = cal["depth_scale"]
        self.scene_info = {"nerf_normalization": {"radius": 5, "translation": np.zeros(3)}}
        self._map = None        # (sx, sy) of the calibration, made at the first distorted frame: arrays (host) or device tensors (fused)
        self.color_paths, self.depth_paths, self.mono_depth_paths, self.poses = [], [], [], []

    def _take(self, parser):
        self.num_imgs = parser.n_img
        self.color_paths, self.depth_paths, self.mono_depth_paths = parser.color_paths, parser.depth_paths, parser.mono_depth_paths
        self.poses = parser.poses

    def undistort_map(self):
        """The calibration's fixed-point map (include/lvdgs.h), made once: NumPy arrays in host mode, device tensors in fused mode."""
        if self._map is None:
            geo = (self.width, self.height, self.fx, self.fy, self.cx, self.cy, self.dist_coeffs)
            self._map = undistort_map_host(*geo) if self.ingest == "host" else undistort_map_device(*geo, self.device)
        return self._map

    def decode_color(self, path):
        """The colour file as an (H, W, 3) uint8 array; anything else is refused."""
        image = np.array(Image.open(path))
        if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
            raise ValueError(f"{path}: a colour frame must decode to three 8-bit channels, got shape {image.shape} dtype {image.dtype}")
        if image.shape[:2] != (self.height, self.width):
            raise ValueError(f"{path}: the frame is {image.shape[1]} x {image.shape[0]}, the calibration says {self.width} x {self.height}")
        return np.ascontiguousarray(image)

    def load_image(self, path):
        """First channel of a depth file."""
        return _first_channel(np.array(Image.open(path)))

    def ingest_image(self, raw, want_u8=False, *, src=None):
        """(H, W, 3) uint8 on the host -> the frame's (3, H, W) float32 tensor on ``device`` (with ``want_u8``: and the bytes after the
        undistortion, on ``device``), by this dataset's mode.  ``src``: fused mode, ``raw`` already on the device."""
        sx, sy = self.undistort_map() if self.disorted else (None, None)
        if self.ingest == "fused":
            if src is None:
                src = _upload(raw, _gpu(self.device, "ingest='fused'"))
            return ingest_frame(src, sx, sy, want_u8=want_u8)
        u8 = remap_host(raw, sx, sy) if self.disorted else raw
        image = torch.from_numpy(convert_host(u8)).to(device=self.device, dtype=self.dtype)
        return (image, torch.from_numpy(u8).to(self.device)) if want_u8 else image

    def read(self, idx):
        """The host half of a frame -> a ``FrameRecord``: every file decoded once, the two float64 divisions.  No device call, nothing
        shared is written: any thread may call it."""
        color_path = self.color_paths[idx]
        raw = self.decode_color(color_path)
        depth_path, mono_path = self.depth_paths[idx], self.mono_depth_paths[idx]
        depth_src = raw[:, :, 0] if depth_path == color_path else self.load_image(depth_path)
        mono_src = raw[:, :, 0] if mono_path == color_path else (depth_src if mono_path == depth_path else self.load_image(mono_path))
        depth = depth_src / self.depth_scale
        mono_depth = mono_src / (self.depth_scale * 5)
        rec = FrameRecord(idx, raw, depth, mono_depth, self.poses[idx])
        if self.planes == "device":
            for src in (depth_src, mono_src):
                if src.dtype not in (np.uint8, np.uint16):
                    raise ValueError(f"frame {idx}: planes='device' takes 8- or 16-bit depth files, this one decodes to {src.dtype}")
            if depth_path != color_path:
                rec.depth_samples = np.ascontiguousarray(depth_src)
            if mono_path != color_path:
                rec.mono_samples = rec.depth_samples if mono_path == depth_path else np.ascontiguousarray(mono_src)
        return rec

    def assemble(self, rec, upload=None):
        """The device half of a frame: ``read``'s record -> the 4-tuple (also kept as ``rec.frame``).  ``upload(host array) -> device
        tensor`` replaces the plain copy of fused mode (``FramePrefetcher``: its pinned ring)."""
        if self.planes == "device" or (self.ingest == "fused" and upload is not None):
            dev = _gpu(self.device, "ingest='fused'")
            put = upload if upload is not None else (lambda a: _upload(a, dev))
            src = put(rec.raw)
            image = self.ingest_image(rec.raw, src=src)
            if self.planes == "device":
                # a 16-bit plane travels as int16: the same bits, a dtype every torch copy takes
                words = lambda a: a.view(np.int16) if a.dtype == np.uint16 else a
                ds = src[:, :, 0] if rec.depth_samples is None else put(words(rec.depth_samples))
                ms = src[:, :, 0] if rec.mono_samples is None else (ds if rec.mono_samples is rec.depth_samples else put(words(rec.mono_samples)))
                rec.depth32 = ingest_depth(ds, self.depth_scale)
                rec.mono_depth32 = ingest_depth(ms, self.depth_scale * 5)
        else:
            image = self.ingest_image(rec.raw)
        # (through `upload` the pose goes the frame's way: a plain copy from pageable memory would wait for the stream)
        pose = torch.from_numpy(rec.pose).to(device=self.device) if upload is None else upload(np.ascontiguousarray(rec.pose))
        rec.frame = (image, rec.depth, pose, rec.mono_depth)
        return rec.frame

    def frame(self, idx):
        """``dataset[idx]`` as a record: ``frame(idx).frame`` is that 4-tuple, ``depth32`` / ``mono_depth32`` the device planes."""
        rec = self.read(idx)
        self.assemble(rec)
        return rec

    def __getitem__(self, idx):
        return self.assemble(self.read(idx))


class dl3dvDataset(MonocularDataset):
    def __init__(self, args, path, config, **kw):
        super().__init__(args, path, config, **kw)
        self._take(dl3dvParser(config["Dataset"]["dataset_path"], config))


class KITTIDataset(MonocularDataset):
    def __init__(self, args, path, config, **kw):
        super().__init__(args, path, config, **kw)
        self._take(KITTIParser(config["Dataset"]["dataset_path"], config))


class WaymoDataset(MonocularDataset):
    def __init__(self, args, path, config, **kw):
        super().__init__(args, path, config, **kw)
        self._take(WaymoParser(config["Dataset"]["dataset_path"]))


class TUMDataset(MonocularDataset):
    def __init__(self, args, path, config, **kw):
        super().__init__(args, path, config, **kw)
        self._take(TUMParser(config["Dataset"]["dataset_path"]))


class ReplicaDataset(MonocularDataset):
    def __init__(self, args, path, config, **kw):
        super().__init__(args, path, config, **kw)
        self._take(ReplicaParser(config["Dataset"]["dataset_path"]))


_TYPES = {"tum": TUMDataset, "replica": ReplicaDataset, "waymo": WaymoDataset, "KITTI": KITTIDataset, "dl3dv": dl3dvDataset}


def load_dataset(args, path, config, *, device="cuda:0", ingest="host", planes="host"):
    """The dataset of ``config["Dataset"]["type"]`` (utils/dataset.py:404-416)."""
    kind = config["Dataset"]["type"]
    if kind not in _TYPES:
        raise ValueError(f"Unknown dataset type {kind!r}: one of {sorted(_TYPES)}")
    return _TYPES[kind](args, path, config, device=device, ingest=ingest, planes=planes)


# ---- frames read ahead of the loops ----
PREFETCH_WORKERS = 4         # the default: PIL's decoders release the interpreter lock and four threads read about three times the frames
                             # of one (profiles/ingest_prefetch.json); a constant, never taken from the machine's CPU count
PREFETCH_MAX_WORKERS = 16


class _Pending:
    """One frame on its way through a worker: ``done`` is set once ``record`` or ``error`` is."""
    __slots__ = ("done", "record", "error")

    def __init__(self):
        self.done, self.record, self.error = threading.Event(), None, None


class FramePrefetcher:
    """Reads the frames of ``dataset`` ahead of the loop that consumes them.  ``order`` is the sequence of indices the consumer will
    ask for; ``workers`` daemon threads run ``dataset.read`` (host only: decode and the float64 divisions) for at most ``depth`` frames
    beyond the one last taken; ``take(idx)`` returns what ``dataset[idx]`` returns (``frame(idx)``: the record, with the device planes).
    It stands where a dataset stands: ``len()``, ``[idx]``, and every other attribute is the dataset's.

    Threads and the device.  A worker makes no HIP and no torch-device call; every upload and launch is made by the thread that calls
    ``take``.  With ``ingest="fused"`` on a GPU that thread, while it hands out frame i, also enqueues the upload and ingest of frames
    whose decode has finished on ONE side stream, from a small ring of pinned buffers (a slot is reused only once the event after its
    copy has completed; with no slot free the frame waits for its own turn and takes the plain copy of ``dataset[idx]``).  The
    consumer's stream takes the frame over with ``wait_event`` and every tensor handed out is marked ``record_stream`` for it.
    ``take`` never synchronises.  In host mode ``assemble`` runs at the frame's turn, as ``dataset[idx]`` does.

    A worker's exception is raised by ``take`` at that frame's turn, as it was raised; the frames after it stay available.  A ``take``
    out of ``order`` is a direct ``dataset`` read.  A wait for a worker ends after ``timeout`` seconds with ``TimeoutError``.
    ``close()`` (or leaving the ``with`` block) stops and joins the workers."""

    def __init__(self, dataset, order, depth=3, workers=PREFETCH_WORKERS, timeout=120.0):
        if int(depth) < 1:
            raise ValueError(f"FramePrefetcher: depth must be at least 1, got {depth}")
        if int(workers) < 1:
            raise ValueError(f"FramePrefetcher: workers must be at least 1, got {workers}")
        workers = min(int(workers), PREFETCH_MAX_WORKERS)            # capped: more decode threads than this only contend
        if not all(callable(getattr(dataset, name, None)) for name in ("read", "assemble", "frame")):
            raise TypeError("FramePrefetcher: the dataset must split a frame into read / assemble (lvdgs.dataset.MonocularDataset)")
        self.dataset, self.order, self.depth, self.timeout = dataset, list(order), int(depth), float(timeout)
        self._cursor = 0              # position in `order` of the next frame in turn
        self._submitted = 0           # positions below this have been given to the workers
        self._pending = {}            # position -> _Pending
        self._todo = queue.Queue()
        self._stop = threading.Event()
        self._closed = False
        self._side = self._consumer_device = None
        self._ring, self._ring_slots = [], 4 * (self.depth + 1)      # colour, two planes and the pose of every frame in flight
        if getattr(dataset, "disorted", False):
            dataset.undistort_map()                                  # made here, before the first worker starts
        if getattr(dataset, "ingest", "host") == "fused" and torch.device(dataset.device).type == "cuda" and torch.cuda.is_available():
            self._consumer_device = _gpu(dataset.device, "FramePrefetcher")
            self._side = torch.cuda.Stream(self._consumer_device)
            self._side.wait_stream(torch.cuda.current_stream(self._consumer_device))     # the undistortion map was made there
        self._threads = [threading.Thread(target=self._work, name=f"lvdgs-prefetch-{k}", daemon=True) for k in range(int(workers))]
        for t in self._threads:
            t.start()
        self._refill()

    # -- the workers: host only --
    def _work(self):
        while not self._stop.is_set():
            try:
                job = self._todo.get(timeout=0.5)
            except queue.Empty:
                continue
            if job is None:
                return
            idx, pending = job
            try:
                pending.record = self.dataset.read(idx)
            except BaseException as e:       # handed to take(), which raises it at the frame's turn
                pending.error = e
            pending.done.set()

    def _refill(self):
        """Give the workers every position up to ``depth`` beyond the one last taken (``_cursor - 1``)."""
        limit = min(len(self.order), self._cursor + self.depth)
        while self._submitted < limit:
            p = self._pending[self._submitted] = _Pending()
            self._todo.put((self.order[self._submitted], p))
            self._submitted += 1

    # -- the consumer's thread --
    def _slot(self, nbytes):
        """A free pinned buffer of at least ``nbytes``: [buffer, event of its last copy], or None when every slot is in flight."""
        for slot in self._ring:
            if slot[1] is None or slot[1].query():
                if slot[0].numel() < nbytes:
                    slot[0] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
                slot[1] = None
                return slot
        if len(self._ring) < self._ring_slots:
            self._ring.append([torch.empty(nbytes, dtype=torch.uint8, pin_memory=True), None])
            return self._ring[-1]
        return None

    def _ring_free(self, count):
        return self._ring_slots - len(self._ring) + sum(1 for s in self._ring if s[1] is None or s[1].query()) >= count

    def _upload(self, array):
        """A host array -> a device tensor of its dtype and shape, copied from a pinned slot on the current (side) stream."""
        array = np.ascontiguousarray(array)
        flat = array.reshape(-1).view(np.uint8)
        slot = self._slot(flat.size)
        if slot is None:
            return _upload(array, self._consumer_device)
        staged = slot[0][:flat.size]
        np.copyto(staged.numpy(), flat)
        out = torch.empty(flat.size, dtype=torch.uint8, device=self._consumer_device)
        out.copy_(staged, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(self._consumer_device))
        return out.view(torch.from_numpy(array).dtype).view(array.shape)

    def _stage(self, rec):
        """Enqueue ``rec``'s device half on the side stream."""
        with torch.cuda.stream(self._side):
            self.dataset.assemble(rec, upload=self._upload)
            rec.ready = torch.cuda.Event()
            rec.ready.record(self._side)

    def _stage_ahead(self):
        """Frames after the cursor whose decode has finished, in order, while the ring has room for a whole frame."""
        for pos in range(self._cursor, self._submitted):
            p = self._pending[pos]
            if not p.done.is_set() or p.error is not None:
                break
            if p.record.frame is None:
                if not self._ring_free(4):
                    break
                self._stage(p.record)

    def frame(self, idx):
        """``take(idx)`` as the record (``dataset.frame(idx)``)."""
        if self._closed:
            raise RuntimeError("FramePrefetcher: take() after close()")
        if self._cursor >= len(self.order) or self.order[self._cursor] != idx:
            return self.dataset.frame(idx)                            # out of order: a direct read, nothing waits
        p = self._pending.pop(self._cursor)
        self._cursor += 1
        self._refill()
        if not p.done.wait(self.timeout):
            raise TimeoutError(f"FramePrefetcher: frame {idx} was not read within {self.timeout:g} s")
        if p.error is not None:
            raise p.error
        rec = p.record
        if self._side is None:
            self.dataset.assemble(rec)
            return rec
        if rec.frame is None:
            self._stage(rec)
        current = torch.cuda.current_stream(self._consumer_device)
        current.wait_event(rec.ready)
        for t in (rec.frame[0], rec.frame[2], rec.depth32, rec.mono_depth32):
            if t is not None:
                t.record_stream(current)
        self._stage_ahead()
        return rec

    def take(self, idx):
        return self.frame(idx).frame

    def __getitem__(self, idx):
        return self.take(idx)

    def __len__(self):
        return len(self.dataset)

    def __getattr__(self, name):          # (only what this object lacks: the dataset's intrinsics, paths, static_mask, ...)
        if name.startswith("_") or name == "dataset":
            raise AttributeError(name)
        return getattr(self.dataset, name)

    def close(self):
        if self._closed:
            return
        self._closed = True
        self._stop.set()
        for _ in self._threads:
            self._todo.put(None)
        for t in self._threads:
            t.join(self.timeout)
        self._pending.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
