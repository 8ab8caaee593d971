"""``lvdgs.config_utils.load_config`` and ``lvdgs.dataset`` without a GPU: the settings loader against the stored merge of the
reference's, the dataset classes in host mode against what the reference's OWN classes returned on the same files
(tests/golden/dataset.npz, made by tests/golden/make_dataset_golden.py), the host mode's undistortion against the independent oracle
(tests/ingest_oracle.py) on the cases of tests/ingest_cases.py, the entry points' refusals."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import ingest_cases as ic
import ingest_oracle as orc
from lvdgs import _lib, dataset as D
from lvdgs.config_utils import load_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TREES = ("kitti", "dl3dv", "waymo", "replica")


# ---- load_config ----
def test_load_config_merges_the_committed_kitti_pair_like_the_reference():
    cfg = load_config(os.path.join(GOLDEN, "configs", "mono", "KITTI", "07.yaml"))
    assert cfg == json.load(open(os.path.join(GOLDEN, "config_07.json")))


def test_load_config_does_not_depend_on_the_working_directory(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cfg = load_config(os.path.join(GOLDEN, "configs", "mono", "waymo", "405841.yaml"))
    assert cfg["Dataset"]["type"] == "waymo" and cfg["Dataset"]["Calibration"]["distorted"] is True
    assert cfg["Training"]["mapping_itr_nosingle"] == 30 and cfg["Training"]["tracking_itr_num"] == 100   # the child's and the base's


def test_load_config_refuses_a_cycle_and_a_missing_parent(tmp_path):
    (tmp_path / "a.yaml").write_text('inherit_from: "b.yaml"\nx: 1\n')
    (tmp_path / "b.yaml").write_text('inherit_from: "a.yaml"\ny: 2\n')
    with pytest.raises(ValueError, match="cycle"):
        load_config(str(tmp_path / "a.yaml"))
    (tmp_path / "c.yaml").write_text('inherit_from: "nowhere/base.yaml"\nx: 1\n')
    with pytest.raises(FileNotFoundError):
        load_config(str(tmp_path / "c.yaml"))
    (tmp_path / "d.yaml").write_text("x: {p: 1, q: 2}\n")
    (tmp_path / "e.yaml").write_text('inherit_from: "d.yaml"\nx: {q: 3}\nz: 4\n')
    assert load_config(str(tmp_path / "e.yaml")) == {"inherit_from": "d.yaml", "x": {"p": 1, "q": 3}, "z": 4}


# ---- the dataset classes against the reference's outputs ----
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "dataset.npz"))


def rebuild_tree(golden, name, root):
    """The golden tree ``name`` written from its stored bytes under ``root`` -> its settings, pointing there."""
    for i, rel in enumerate(golden[f"{name}/files"]):
        path = os.path.join(root, str(rel))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(golden[f"{name}/file/{i}"].tobytes())
    cfg = json.loads(str(golden[f"{name}/config"]))
    cfg["Dataset"]["dataset_path"] = str(root)
    return cfg


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", TREES)
def test_host_mode_returns_what_the_reference_classes_returned(golden, tmp_path, name):
    cfg = rebuild_tree(golden, name, tmp_path / name)
    ds = D.load_dataset(None, None, cfg, device="cpu", ingest="host")
    root = cfg["Dataset"]["dataset_path"]
    for attr, key in (("color_paths", "color_order"), ("depth_paths", "depth_order"), ("mono_depth_paths", "mono_order")):
        assert [os.path.relpath(p, root) for p in getattr(ds, attr)] == [os.path.normpath(str(p)) for p in golden[f"{name}/{key}"]], attr
    assert len(ds) == ds.num_imgs == 4 and ds.dtype is torch.float32 and ds.device == "cpu"
    for k in range(len(ds)):
        image, depth, pose, mono = ds[k]
        assert image.dtype is torch.float32 and pose.dtype is torch.float64
        assert same_bits(image.numpy(), golden[f"{name}/image/{k}"]), (name, k, "image")
        assert same_bits(depth, golden[f"{name}/depth/{k}"]), (name, k, "depth")
        assert same_bits(mono, golden[f"{name}/mono/{k}"]), (name, k, "mono depth")
        assert same_bits(pose.numpy(), golden[f"{name}/pose/{k}"]), (name, k, "pose")
        assert same_bits(ds.poses[k], golden[f"{name}/pose/{k}"])


def test_the_attributes_the_loops_read(golden, tmp_path):
    from lvdgs.graphics_utils import focal2fov
    cfg = rebuild_tree(golden, "waymo", tmp_path / "w")
    ds = D.load_dataset(None, None, cfg, device="cpu")
    cal = cfg["Dataset"]["Calibration"]
    assert (ds.fx, ds.fy, ds.cx, ds.cy, ds.width, ds.height) == tuple(cal[k] for k in ("fx", "fy", "cx", "cy", "width", "height"))
    assert ds.fovx == focal2fov(ds.fx, ds.width) and ds.fovy == focal2fov(ds.fy, ds.height)
    assert np.array_equal(ds.K, [[ds.fx, 0, ds.cx], [0, ds.fy, ds.cy], [0, 0, 1]]) and ds.dist_coeffs.shape == (5,) and ds.disorted is False
    assert ds.scene_info["nerf_normalization"]["radius"] == 5 and ds.ingest == "host"
    assert D.load_dataset(None, None, cfg).device == "cuda:0"       # the default, as the reference hard-codes it


def test_a_shared_path_is_decoded_once(golden, tmp_path, monkeypatch):
    """KITTI's depth and mono-depth placeholders ARE the colour file: one decode per frame, not three."""
    from PIL import Image
    cfg = rebuild_tree(golden, "kitti", tmp_path / "k")
    ds = D.load_dataset(None, None, cfg, device="cpu")
    opened = []
    real = Image.open
    monkeypatch.setattr(Image, "open", lambda p, *a, **k: (opened.append(p), real(p, *a, **k))[1])
    ds[0]
    assert opened == [ds.color_paths[0]]
    cfg = rebuild_tree(golden, "waymo", tmp_path / "w")
    ds = D.load_dataset(None, None, cfg, device="cpu")
    del opened[:]
    ds[1]
    assert opened == [ds.color_paths[1], ds.depth_paths[1], ds.mono_depth_paths[1]]


def test_refusals_of_the_dataset_layer(golden, tmp_path):
    from PIL import Image
    cfg = rebuild_tree(golden, "waymo", tmp_path / "w")
    bad = json.loads(json.dumps(cfg))
    bad["Dataset"]["type"] = "euroc"
    with pytest.raises(ValueError, match="Unknown dataset type"):
        D.load_dataset(None, None, bad, device="cpu")
    bad = json.loads(json.dumps(cfg))
    del bad["Dataset"]["Calibration"]["depth_scale"]
    with pytest.raises(ValueError, match="depth_scale"):
        D.load_dataset(None, None, bad, device="cpu")
    with pytest.raises(ValueError, match="ingest"):
        D.load_dataset(None, None, cfg, device="cpu", ingest="gpu")
    ds = D.load_dataset(None, None, cfg, device="cpu")
    Image.fromarray(np.zeros((32, 48), np.uint8)).save(ds.color_paths[0])                 # one channel
    with pytest.raises(ValueError, match="three 8-bit channels"):
        ds[0]
    Image.fromarray(np.zeros((32, 48, 4), np.uint8)).save(ds.color_paths[1])              # four channels
    with pytest.raises(ValueError, match="three 8-bit channels"):
        ds[1]
    Image.fromarray(np.zeros((32, 48), np.uint16)).save(ds.color_paths[2])                # 16 bits
    with pytest.raises(ValueError, match="three 8-bit channels"):
        ds[2]
    fused = D.load_dataset(None, None, cfg, device="cpu", ingest="fused")                 # no quiet fall-back to the host mode
    with pytest.raises(_lib.LvdgsError, match="GPU"):
        fused[3]


# ---- the tum parser's rules, on hand-made lists ----
def test_tum_association_and_subsampling_rules():
    # Rule 1: an image stamp is kept when BOTH the nearest depth stamp and the nearest pose stamp lie closer than 0.08 s; the triple names them.
    t_img = np.array([0.00, 0.01, 0.05, 0.50, 1.00])
    t_dep = np.array([0.02, 0.57, 1.07])
    t_pos = np.array([0.00, 0.04, 0.42, 0.99, 2.00])
    #  0.00: depth 0.02 (0.02), pose 0.00          -> kept (0, 0, 0)
    #  0.01: depth 0.02 (0.01), pose 0.00 (0.01)   -> kept (1, 0, 0)
    #  0.05: depth 0.02 (0.03), pose 0.04 (0.01)   -> kept (2, 0, 1)
    #  0.50: depth 0.57 (0.07), pose 0.42 (0.08: not closer than 0.08) -> dropped
    #  1.00: depth 1.07 (0.07), pose 0.99          -> kept (4, 2, 3)
    assoc = D.tum_associate(t_img, t_dep, t_pos)
    assert assoc == [(0, 0, 0), (1, 0, 0), (2, 0, 1), (4, 2, 3)]
    # Rule 2: the first association is kept, then each whose image stamp is MORE than 1 / frame_rate behind the last kept one.
    assert D.tum_subsample(t_img, assoc, frame_rate=32) == [0, 2, 3]        # 0.01 - 0.00 < 1 / 32; 0.05 - 0.00 > 1 / 32; 1.00 - 0.05 > 1 / 32
    assert D.tum_subsample(t_img, assoc, frame_rate=1) == [0]              # 1.00 - 0.00 is not MORE than 1
    assert D.tum_subsample(t_img, [], 32) == []


def test_tum_parser_on_a_hand_made_directory(tmp_path):
    from scipy.spatial.transform import Rotation
    quat = Rotation.from_rotvec([0.1, -0.2, 0.3]).as_quat()      # (x, y, z, w)
    (tmp_path / "rgb.txt").write_text("# colour\n0.00 rgb/a.png\n0.01 rgb/b.png\n0.10 rgb/c.png\n")
    (tmp_path / "depth.txt").write_text("0.005 depth/a.png\n0.11 depth/c.png\n")
    (tmp_path / "mono_depth.txt").write_text("0.00 mono/a.png\n0.01 mono/b.png\n0.10 mono/c.png\n")
    (tmp_path / "groundtruth.txt").write_text("# timestamp tx ty tz qx qy qz qw\n0.00 1.0 2.0 3.0 0 0 0 1\n0.10 -1.0 0.5 2.0 " + " ".join(repr(float(q)) for q in quat) + "\n")
    p = D.TUMParser(str(tmp_path))
    assert [os.path.relpath(x, tmp_path) for x in p.color_paths] == ["rgb/a.png", "rgb/c.png"]          # b is 0.01 s behind a: thinned at 32 Hz
    assert [os.path.relpath(x, tmp_path) for x in p.depth_paths] == ["depth/a.png", "depth/c.png"]
    assert [os.path.relpath(x, tmp_path) for x in p.mono_depth_paths] == ["mono/a.png", "mono/c.png"]
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = Rotation.from_quat(quat).as_matrix(), [-1.0, 0.5, 2.0]
    assert np.allclose(p.poses[1] @ c2w, np.eye(4), atol=1e-12) and np.allclose(np.linalg.inv(p.poses[0])[:3, 3], [1.0, 2.0, 3.0])
    assert "UNPINNED" in D.TUMParser.__doc__


# ---- the host mode's arithmetic against the oracle ----
@pytest.mark.parametrize("name", sorted(ic.SMALL))
def test_the_oracle_s_two_forms_agree(name):
    """The per-pixel statement of the header's rule and the array form used for the full frame."""
    c = ic.case(name)
    sx, sy = orc.undistort_map_loop(c["W"], c["H"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"])
    assert same_bits(sx, ic.reference_map(name)[0]) and same_bits(sy, ic.reference_map(name)[1])
    img = ic.pixels(name, "noise")
    assert same_bits(orc.remap_loop(img, sx, sy), ic.reference(name, "noise", True)[0])
    assert same_bits(orc.convert_loop(img), ic.reference(name, "noise", False)[1])


def test_the_cases_hold_what_they_are_for():
    W, H = ic.SMALL["outside"]["W"], ic.SMALL["outside"]["H"]
    sx, sy = ic.reference_map("outside")
    assert (sx < -32).any() and (sx > 32 * W).any() and (sy < -32).any() and (sy > 32 * H).any()      # off the image on every side
    share = ((sx < 0) | (sx > 32 * (W - 1)) | (sy < 0) | (sy > 32 * (H - 1))).mean()
    assert 0.1 < share < 0.9, share
    c = ic.SMALL["ties"]
    ties = [(u, v) for v in range(c["H"]) for u in range(c["W"]) if (u * (u * u + v * v)) % 32 == 16 and u * (1 + (u * u + v * v) / 1024) < 2 ** 20]
    assert len(ties) > 50
    sx, _ = ic.reference_map("ties")
    up = dn = 0
    for u, v in ties:
        exact2 = 64 * u + u * (u * u + v * v) // 16          # twice mapx * 32: an odd integer at a tie
        assert exact2 % 2 == 1 and sx[v, u] % 2 == 0 and abs(2 * int(sx[v, u]) - exact2) == 1     # rounded to the even neighbour
        up += 2 * int(sx[v, u]) > exact2
        dn += 2 * int(sx[v, u]) < exact2
    assert up > 0 and dn > 0                                  # ties that round up and ties that round down
    for name in ("past_2^20", "not_finite"):
        sx, sy = ic.reference_map(name)
        assert (sx == orc.OUTSIDE).any() and (sy == orc.OUTSIDE).any() and (sx != orc.OUTSIDE).any(), name
    big = ic.SMALL["past_2^20"]
    x = (0 - big["cx"]) / big["fx"]
    assert abs(big["fx"] * x * (1 + big["dist"][0] * x * x)) > 2 ** 20      # finite and beyond the limit: not a NaN case


@pytest.mark.parametrize("kind", ic.KINDS)
@pytest.mark.parametrize("name", sorted(ic.SMALL))
def test_host_mode_undistortion_equals_the_oracle(name, kind):
    c = ic.case(name)
    sx, sy = D.undistort_map_host(c["W"], c["H"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"])
    want_sx, want_sy = ic.reference_map(name)
    assert same_bits(sx, want_sx) and same_bits(sy, want_sy)
    img = ic.pixels(name, kind)
    want_u8, want = ic.reference(name, kind, True)
    got_u8 = D.remap_host(img, sx, sy)
    assert same_bits(got_u8, want_u8)
    assert same_bits(D.convert_host(got_u8), want)
    assert same_bits(D.convert_host(img), ic.reference(name, kind, False)[1])


def test_host_mode_on_a_full_waymo_frame_equals_the_oracle():
    c = ic.case(ic.FULL)
    sx, sy = D.undistort_map_host(c["W"], c["H"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"])
    assert same_bits(sx, ic.reference_map(ic.FULL)[0]) and same_bits(sy, ic.reference_map(ic.FULL)[1])
    got = D.remap_host(ic.pixels(ic.FULL, "noise"), sx, sy)
    assert same_bits(got, ic.reference(ic.FULL, "noise", True)[0])


def test_zero_coefficients_with_distorted_true_return_the_input(golden, tmp_path):
    """An all-zero distortion is the identity map: every sx, sy a multiple of 32 on its own pixel, the bytes unchanged."""
    cfg = rebuild_tree(golden, "waymo", tmp_path / "w")
    plain = D.load_dataset(None, None, cfg, device="cpu")
    cfg2 = json.loads(json.dumps(cfg))
    cfg2["Dataset"]["Calibration"]["distorted"] = True
    ds = D.load_dataset(None, None, cfg2, device="cpu")
    sx, sy = ds.undistort_map()
    v, u = np.mgrid[0:ds.height, 0:ds.width]
    assert np.array_equal(sx, 32 * u) and np.array_equal(sy, 32 * v)
    for k in range(len(ds)):
        assert same_bits(ds[k][0].numpy(), plain[k][0].numpy())
    c = ic.case(ic.FULL)
    sx, sy = D.undistort_map_host(c["W"], c["H"], c["fx"], c["fy"], c["cx"], c["cy"], (0.0,) * 5)
    v, u = np.mgrid[0:c["H"], 0:c["W"]]
    assert np.array_equal(sx, 32 * u) and np.array_equal(sy, 32 * v)      # Waymo's intrinsics too: (u - cx) / fx * fx + cx comes back to u


def test_a_distorted_tree_in_host_mode(golden, tmp_path):
    cfg = rebuild_tree(golden, "replica", tmp_path / "r")
    cfg["Dataset"]["Calibration"].update(distorted=True, k1=0.2, k2=-0.05, p1=0.01, p2=-0.004, k3=0.02)
    ds = D.load_dataset(None, None, cfg, device="cpu")
    cal = cfg["Dataset"]["Calibration"]
    sx, sy = orc.undistort_map(cal["width"], cal["height"], cal["fx"], cal["fy"], cal["cx"], cal["cy"], ds.dist_coeffs)
    from PIL import Image
    raw = np.array(Image.open(ds.color_paths[2]))
    image, depth, _, _ = ds[2]
    assert same_bits(image.numpy(), orc.convert(orc.remap(raw, sx, sy)))
    assert same_bits(depth, golden["replica/depth/2"])          # the depth is not undistorted (nor is the reference's)
    image, u8 = ds.ingest_image(raw, want_u8=True)
    assert same_bits(u8.numpy(), orc.remap(raw, sx, sy))


# ---- the C side without a GPU ----
def test_the_outside_mark_is_the_oracle_s():
    assert _lib.MAP_OUTSIDE == orc.OUTSIDE == -2 ** 31


def ingest_refusals():
    """(what, changes to a valid argument block, a word of the message).  The pointers are never dereferenced: every call is refused
    before a launch."""
    return [("zero width", dict(width=0), "image size"), ("negative height", dict(height=-3), "image size"),
            ("src NULL", dict(src=None), "NULL"), ("image NULL", dict(image=None), "NULL"),
            ("only sx", dict(map_sx=4096), "exactly one"), ("only sy", dict(map_sy=4096), "exactly one"),
            ("short pitch", dict(src_row_bytes=3 * 16 - 1), "src_row_bytes"), ("negative pitch", dict(src_row_bytes=-48), "src_row_bytes")]


def valid_ingest_args(**over):
    a = dict(width=16, height=8, src=256, src_row_bytes=48, map_sx=None, map_sy=None, image=512, image_u8=None)
    a.update(over)
    return _lib.IngestArgs(**a)


def test_refusals_of_both_entry_points_without_a_gpu():
    L = _lib.lib()
    assert L.lvdgs_ingest_frame(None, None) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error()
    for what, over, word in ingest_refusals():
        assert L.lvdgs_ingest_frame(C.byref(valid_ingest_args(**over)), None) == _lib.E_INVALID, what
        assert word.encode() in L.lvdgs_last_error(), (what, L.lvdgs_last_error())
    dist = (C.c_double * 5)(0.1, 0.0, 0.0, 0.0, 0.0)
    call = lambda W=16, H=8, fx=10.0, fy=10.0, cx=8.0, cy=4.0, d=dist, sx=256, sy=512: L.lvdgs_undistort_map(W, H, fx, fy, cx, cy, d, sx, sy, None)
    for what, kw, word in [("zero width", dict(W=0), "image size"), ("negative height", dict(H=-1), "image size"), ("dist NULL", dict(d=None), "NULL"),
                           ("sx NULL", dict(sx=None), "NULL"), ("sy NULL", dict(sy=None), "NULL"), ("fx zero", dict(fx=0.0), "fx"),
                           ("fy NaN", dict(fy=float("nan")), "fy"), ("cx infinite", dict(cx=float("inf")), "cx")]:
        assert call(**kw) == _lib.E_INVALID, what
        assert word.encode() in L.lvdgs_last_error(), (what, L.lvdgs_last_error())
