"""Per-view camera intrinsics on the host side: the table form of capture.Capture (constructors, collapse of equal rows, downscale, mvps,
ray / raster agreement), COLMAP reconstructions whose images use different cameras (load_colmap(per_view_intrinsics=True), save_colmap,
the reference's ColmapDataset as recorded in tests/golden/colmap_pv.npz by tests/golden/make_golden_colmap_pv.py) and the DTU format
(load_dtu / save_dtu against a float64 construction).  Host code only."""
import os
import shutil
import struct

import numpy as np
import pytest
import torch

from nerf2mesh_amd import capture as C, synthetic

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = os.path.join(HERE, "golden", "colmap_tiny")

# four rows, all different: fx != fy, principal points off-centre by non-integer amounts (a 5 x 7 view)
ROWS = np.array([[9.5, 7.25, 3.3, 2.85], [8.75, 8.1, 3.9, 2.2], [10.2, 6.9, 3.05, 2.65], [7.6, 7.7, 3.55, 2.4]])

# ------------------------------------------------------------------------------------------------- the COLMAP set with three cameras
# (id, model id, width, height, params): PINHOLE, PINHOLE, SIMPLE_RADIAL -- focal lengths and centres all different, one of them with
# values that are no fp32 numbers, one with a distortion parameter (ignored)
PV_CAMERAS = [(1, 1, 12, 10, [14.0, 13.0, 6.5, 4.25]), (2, 1, 12, 10, [15.5, 12.25, 6.125, 4.75]), (3, 2, 12, 10, [13.3, 5.9, 5.1, 0.05])]
PV_ROWS = {1: (14.0, 13.0, 6.5, 4.25), 2: (15.5, 12.25, 6.125, 4.75), 3: (13.3, 13.3, 5.9, 5.1)}


def rewrite_cameras(root, cams):
    with open(os.path.join(root, "sparse", "0", "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(cams)))
        for cid, model, w, h, params in cams:
            f.write(struct.pack("<iiQQ", cid, model, w, h))
            f.write(np.asarray(params, dtype="<f8").tobytes())


def rewrite_camera_ids(root, id_of):
    """Sets the camera id of the n-th image record of images.bin to id_of(n); returns the ids in the order of the sorted image keys."""
    name = os.path.join(root, "sparse", "0", "images.bin")
    blob = bytearray(open(name, "rb").read())
    count, at, out = struct.unpack_from("<Q", blob, 0)[0], 8, {}
    for n in range(count):
        iid = struct.unpack_from("<i", blob, at)[0]
        at += 4 + 56                                  # the image id, q + t
        struct.pack_into("<i", blob, at, id_of(n))
        out[iid] = id_of(n)
        at = blob.index(b"\0", at + 4) + 1            # the camera id, the name
        at += 8 + 24 * struct.unpack_from("<Q", blob, at)[0]
    assert at == len(blob)
    open(name, "wb").write(bytes(blob))
    return [out[k] for k in sorted(out)]


def write_pv_copy(root):
    """A copy of tests/golden/colmap_tiny whose nine images use the three cameras PV_CAMERAS in turn; returns the camera id per image."""
    shutil.copytree(TINY, root)
    rewrite_cameras(root, PV_CAMERAS)
    return rewrite_camera_ids(root, lambda n: 1 + n % 3)


@pytest.fixture(scope="module")
def pv_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("pv") / "rec")
    return root, write_pv_copy(root)


# ------------------------------------------------------------------------------------------------------------------ the table form
def _set(rows, per_view=None, **kw):
    V = len(rows)
    g = torch.Generator().manual_seed(3)
    images = torch.randint(0, 256, (V, 5, 7, 4), generator=g, dtype=torch.uint8)
    return C.Capture.from_arrays(synthetic.make_cameras(V, seed=2), images, rows, per_view=per_view, **kw)


def test_table_form_from_arrays():
    cap = _set(ROWS)
    assert cap.per_view_intrinsics is True
    assert torch.is_tensor(cap.intrinsics) and cap.intrinsics.dtype == torch.float32 and tuple(cap.intrinsics.shape) == (4, 4)
    assert cap.intrinsics_host.dtype == np.float64 and np.array_equal(cap.intrinsics_host, ROWS)
    assert np.array_equal(cap.intrinsics.numpy(), ROWS.astype(np.float32))            # every entry rounded once
    assert cap.intrinsics_of(2) == tuple(ROWS[2])
    # a tensor is taken like an array
    assert torch.equal(_set(torch.from_numpy(ROWS)).intrinsics, cap.intrinsics)
    with pytest.raises(ValueError, match="intrinsics must be"):
        C.Capture(synthetic.make_cameras(4, seed=2), cap.bank, 5, 7, ROWS[:3])


def test_equal_rows_collapse_and_per_view_overrides():
    same = np.tile(ROWS[1], (4, 1))
    shared = _set(same)
    assert shared.per_view_intrinsics is False and shared.intrinsics == tuple(ROWS[1]) and shared.intrinsics_host is None
    plain = _set(tuple(ROWS[1]))
    assert plain.intrinsics == shared.intrinsics and torch.equal(plain.mvps, shared.mvps)
    for given in (same, tuple(ROWS[1])):
        forced = _set(given, per_view=True)
        assert forced.per_view_intrinsics is True and np.array_equal(forced.intrinsics_host, same)
        assert torch.equal(forced.mvps, shared.mvps)                                   # the same projections, bit for bit
    with pytest.raises(ValueError, match="per_view=False"):
        _set(ROWS, per_view=False)
    assert _set(same, per_view=False).per_view_intrinsics is False


def test_downscale_divides_the_rows():
    g = torch.Generator().manual_seed(3)
    images = torch.randint(0, 256, (4, 10, 14, 3), generator=g, dtype=torch.uint8)
    cap = C.Capture.from_arrays(synthetic.make_cameras(4, seed=2), images, ROWS * 2, downscale=2)
    assert (cap.H, cap.W) == (5, 7) and cap.per_view_intrinsics
    assert np.array_equal(cap.intrinsics_host, ROWS * 2 / 2) and np.array_equal(cap.intrinsics.numpy(), (ROWS * 2 / 2).astype(np.float32))
    third = C.Capture.from_arrays(synthetic.make_cameras(4, seed=2), images, ROWS, downscale=3)
    assert np.array_equal(third.intrinsics_host, ROWS / 3) and (third.H, third.W) == (3, 4)


def test_mvps_are_built_per_view():
    cap = _set(ROWS)
    for v in range(4):
        want = C.proj_matrix(5, 7, *(float(x) for x in ROWS[v])) @ torch.inverse(cap.poses[v])
        assert torch.equal(cap.mvps[v], want), v
    assert not torch.equal(cap.mvps[1] @ cap.poses[1], cap.mvps[0] @ cap.poses[0])


def test_rays_and_raster_agree_for_every_view():
    """tests/test_capture_io.py's check, per view of a set whose four rows differ: the point o + 3 d of pixel (i, j), pushed through
    mvps[v], lands within 1e-3 px of (i + 0.5, j + 0.5) -- the bound DESIGN 4.18 uses (fp32 arithmetic on coordinates below 10)."""
    h, w = 5, 7
    cap = _set(ROWS)
    jj, ii = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    for v in range(4):
        o, d, _, _ = cap.view(v)
        p = torch.cat([o + 3 * d, torch.ones(h * w, 1)], -1) @ cap.mvps[v].T
        ndc = p[:, :2] / p[:, 3:]
        wx, wy = (ndc[:, 0] * 0.5 + 0.5) * w, (ndc[:, 1] * 0.5 + 0.5) * h
        ex, ey = (wx - (ii.reshape(-1) + 0.5)).abs().max(), (wy - (jj.reshape(-1) + 0.5)).abs().max()
        print(f"view {v}: {float(ex):.3g} px, {float(ey):.3g} px")
        assert ex < 1e-3 and ey < 1e-3 and (p[:, 3] > 0).all()
        # ... and the view's rays are those of a shared set at that row
        one = _set(tuple(ROWS[v])).view(v)
        assert torch.equal(o, one[0]) and torch.equal(d, one[1])
    # with another view's projection the pixel centres are missed: the projections are per view for a reason
    o, d, _, _ = cap.view(0)
    p = torch.cat([o + 3 * d, torch.ones(h * w, 1)], -1) @ (C.proj_matrix(h, w, *(float(x) for x in ROWS[1])) @ torch.inverse(cap.poses[0])).T
    assert ((p[:, 0] / p[:, 3] * 0.5 + 0.5) * w - (ii.reshape(-1) + 0.5)).abs().max() > 0.1


def test_synthetic_renders_every_view_at_its_own_row():
    poses = synthetic.make_cameras(4, seed=0)
    rows = ROWS * 3
    cap = C.Capture.synthetic(poses, H=15, W=21, intrinsics=rows)
    assert cap.per_view_intrinsics and np.array_equal(cap.intrinsics_host, rows)
    for v in range(4):
        one = C.Capture.synthetic(poses, H=15, W=21, intrinsics=tuple(rows[v]))
        assert torch.equal(cap.bank[v], one.bank[v]), v
    same = C.Capture.synthetic(poses, H=15, W=21, intrinsics=np.tile(rows[0], (4, 1)), per_view=True)
    assert same.per_view_intrinsics and torch.equal(same.bank, C.Capture.synthetic(poses, H=15, W=21, intrinsics=tuple(rows[0])).bank)


def test_save_nerf_refuses_a_per_view_set(tmp_path):
    with pytest.raises(ValueError, match="one camera"):
        _set(ROWS).save_nerf(str(tmp_path))
    _set(np.tile(ROWS[0], (4, 1))).save_nerf(str(tmp_path))                # equal rows: a shared set


# --------------------------------------------------------------------------------------------------------------------------- COLMAP
def test_default_load_still_raises_and_names_the_option(pv_root):
    root, _ = pv_root
    with pytest.raises(ValueError, match="one camera model per set") as e:
        C.Capture.load_colmap(root)
    assert "per_view_intrinsics=True" in str(e.value)


@pytest.mark.parametrize("downscale", [1, 2])
def test_load_colmap_per_view(pv_root, downscale):
    root, ids = pv_root
    assert ids == [1, 2, 3] * 3
    cap = C.Capture.load_colmap(root, split="trainval", downscale=downscale, per_view_intrinsics=True, sparse_depth=True)
    want = np.array([PV_ROWS[i] for i in ids], dtype=np.float64) / downscale
    assert cap.per_view_intrinsics and (cap.H, cap.W) == (10 // downscale, 12 // downscale)
    assert np.array_equal(cap.intrinsics_host, want) and np.array_equal(cap.intrinsics.numpy(), want.astype(np.float32))
    # everything that does not depend on the cameras is the one-camera set's: poses, bank, keypoints (common size for the inside test)
    tiny = C.Capture.load_colmap(TINY, split="trainval", downscale=downscale, sparse_depth=True)
    assert torch.equal(cap.poses, tiny.poses) and torch.equal(cap.bank, tiny.bank) and torch.equal(cap.cam_near_far, tiny.cam_near_far)
    assert torch.equal(cap.sparse_depth.coords, tiny.sparse_depth.coords) and torch.equal(cap.sparse_depth.depth, tiny.sparse_depth.depth)
    # the splits take their rows along
    train = C.Capture.load_colmap(root, split="train", downscale=downscale, per_view_intrinsics=True)
    assert np.array_equal(train.intrinsics_host, want[[1, 2, 3, 4, 5, 6, 7]])
    # one camera among the kept images: the option changes nothing
    assert C.Capture.load_colmap(TINY, split="trainval", per_view_intrinsics=True).per_view_intrinsics is False


def test_save_colmap_then_load_returns_the_table(pv_root, tmp_path):
    root, ids = pv_root
    a = C.Capture.load_colmap(root, split="trainval", scale=0.7, per_view_intrinsics=True, keep_model=True)
    a.save_colmap(str(tmp_path / "again"), scale=0.7, **a.colmap)
    cams = C.read_colmap_cameras(str(tmp_path / "again" / "sparse" / "0" / "cameras.bin"))
    ims = C.read_colmap_images(str(tmp_path / "again" / "sparse" / "0" / "images.bin"))
    assert sorted(cams) == [1, 2, 3] and [ims[k]["camera_id"] for k in sorted(ims)] == ids      # one camera per distinct row
    b = C.Capture.load_colmap(str(tmp_path / "again"), split="trainval", scale=0.7, per_view_intrinsics=True)
    assert b.per_view_intrinsics and np.array_equal(a.intrinsics_host, b.intrinsics_host) and torch.equal(a.intrinsics, b.intrinsics)
    assert torch.equal(a.bank, b.bank) and (a.poses - b.poses).abs().max() <= 4 * 2.4e-7      # tests/test_colmap_io.py's round-trip bound
    with pytest.raises(ValueError, match="one camera model per set"):
        C.Capture.load_colmap(str(tmp_path / "again"))
    with pytest.raises(ValueError, match="SIMPLE_PINHOLE when"):
        a.save_colmap(str(tmp_path / "simple"), a.colmap["points"], model="SIMPLE_PINHOLE")       # rows 0, 1 have fx != fy


def test_differing_sizes_raise(pv_root, tmp_path):
    root = str(tmp_path / "rec")
    shutil.copytree(pv_root[0], root)
    rewrite_cameras(root, PV_CAMERAS[:2] + [(3, 2, 16, 10, [13.3, 5.9, 5.1, 0.05])])
    with pytest.raises(ValueError, match="differing image sizes"):
        C.Capture.load_colmap(root, per_view_intrinsics=True)
    with pytest.raises(ValueError, match="one camera model per set"):
        C.Capture.load_colmap(root)


def test_load_colmap_per_view_matches_the_reference(pv_root):
    """tests/golden/colmap_pv.npz: what the unchanged ColmapDataset makes of the same set.  The table equals the recorded fp32 values
    exactly (both are one fp32 rounding of the same float64 quotient); the poses by tests/test_colmap_io.py's criterion (4 x its measured
    gap of 0: exactly)."""
    g = dict(np.load(os.path.join(HERE, "golden", "colmap_pv.npz")))
    for tag, ds in (("", 1), ("ds2_", 2)):
        cap = C.Capture.load_colmap(pv_root[0], split="trainval", scale=-1, downscale=ds, per_view_intrinsics=True)
        assert g[tag + "intrinsics"].dtype == np.float32 and g[tag + "intrinsics"].shape == (9, 4)
        assert np.array_equal(cap.intrinsics.numpy(), g[tag + "intrinsics"])
        assert not (g[tag + "intrinsics"] == g[tag + "intrinsics"][0]).all()
        assert (cap.H, cap.W) == tuple(g[tag + "HW"])
        gap = np.abs(cap.poses.numpy() - g[tag + "poses"]).max()
        print(tag or "plain", "pose gap", float(gap))
        assert gap <= 4 * 0.0
    for split in ("train", "val"):
        ids = g[split + "_ids"].tolist()
        cap = C.Capture.load_colmap(pv_root[0], split=split, scale=-1, per_view_intrinsics=True)
        assert np.array_equal(cap.intrinsics.numpy(), g["intrinsics"][ids]) and np.array_equal(cap.poses.numpy(), g["poses"][ids])


# ------------------------------------------------------------------------------------------------------------------------------ DTU
# Largest relative error of load_dtu against the float64 construction of the five views below, MEASURED on the CPU (printed by the test):
#   rows  max |got - want| / |want|            = 8.21e-8   (K comes back from an fp32 P: about one fp32 rounding of its entries, 6e-8)
#   poses max |got - want| / max |want|        = 1.03e-7   (the fp32 storage of the pose itself accounts for 6e-8)
# The bound cannot be derived in advance (it depends on the conditioning of P[:,:3]); the assertion is 4 x the measured value.  The
# save_dtu -> load_dtu round trip of a 5-view set measures 8.4e-8 / 7.5e-8 and is held to the same bound.
DTU_ROWS_MEASURED, DTU_POSES_MEASURED = 8.21e-8, 1.03e-7
DTU_V, DTU_H, DTU_W = 5, 10, 12


def _dtu_cameras():
    rng = np.random.default_rng(11)
    Ks, Rs, Cs = [], [], []
    for v in range(DTU_V):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        Rs.append(q)
        Cs.append(rng.uniform(-1, 1, 3) * 1.5)
        Ks.append(np.array([[14.0 + 1.3 * v, 0, 6.5 - 0.2 * v], [0, 13.0 - 0.7 * v, 4.25 + 0.15 * v], [0, 0, 1]]))
    return Ks, Rs, Cs


def _write_dtu(root, world_scale=None, channels=3):
    """image/, mask/, cameras_sphere.npz with P = K [R | -R C] (float64, stored as fp32) times a per-view projective scale (negative for
    one view); -> images [V,H,W,3], masks [V,H,W], the float64 rows and the float64 poses load_dtu(scale, offset) should give."""
    from PIL import Image
    Ks, Rs, Cs = _dtu_cameras()
    rng = np.random.default_rng(5)
    images = rng.integers(0, 256, (DTU_V, DTU_H, DTU_W, 3), dtype=np.uint8)
    masks = rng.integers(0, 256, (DTU_V, DTU_H, DTU_W), dtype=np.uint8)
    os.makedirs(os.path.join(root, "image")); os.makedirs(os.path.join(root, "mask"))
    mats = {}
    for v in range(DTU_V):
        P = Ks[v] @ np.concatenate([Rs[v], -(Rs[v] @ Cs[v])[:, None]], 1)
        world = np.eye(4)
        world[:3] = P * (1.0 if world_scale is None else world_scale[v])
        mats[f"world_mat_{v}"], mats[f"scale_mat_{v}"] = world.astype(np.float32), np.eye(4, dtype=np.float32)
        Image.fromarray(images[v]).save(os.path.join(root, "image", f"{v:03d}.png"))
        Image.fromarray(np.repeat(masks[v][..., None], 3, -1)).save(os.path.join(root, "mask", f"{v:03d}.png"))
    np.savez(os.path.join(root, "cameras_sphere.npz"), **mats)
    return images, masks, Ks, Rs, Cs


def _dtu_poses(Rs, Cs, scale, offset):
    poses = np.tile(np.eye(4), (len(Rs), 1, 1))
    for v, (R, Cc) in enumerate(zip(Rs, Cs)):
        poses[v, :3, :3], poses[v, :3, 3] = R.T, Cc * scale + np.asarray(offset, dtype=np.float64)
    poses[:, :3, 1:3] *= -1
    poses = poses[:, [1, 0, 2, 3], :]
    poses[:, 2] *= -1
    return poses


def _dtu_errors(cap, rows, poses):
    e_rows = np.abs(cap.intrinsics_host / rows - 1).max()
    e_poses = np.abs(cap.poses.double().numpy() - poses).max() / np.abs(poses).max()
    return float(e_rows), float(e_poses)


def test_load_dtu_recovers_rows_and_poses(tmp_path):
    root = str(tmp_path / "scan")
    images, masks, Ks, Rs, Cs = _write_dtu(root, world_scale=[1.0, 2.5, -1.0, 0.4, -3.0])
    rows = np.array([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]] for K in Ks])
    cap = C.Capture.load_dtu(root, split="all", scale=0.8, offset=(0.1, -0.2, 0.05))
    assert cap.per_view_intrinsics and len(cap) == DTU_V and (cap.H, cap.W) == (DTU_H, DTU_W) and cap.has_alpha
    e_rows, e_poses = _dtu_errors(cap, rows, _dtu_poses(Rs, Cs, 0.8, (0.1, -0.2, 0.05)))
    print(f"load_dtu against the float64 construction: rows {e_rows:.3g} relative, poses {e_poses:.3g} of the largest entry")
    assert e_rows <= 4 * DTU_ROWS_MEASURED and e_poses <= 4 * DTU_POSES_MEASURED
    assert np.array_equal(cap.intrinsics.numpy(), cap.intrinsics_host.astype(np.float32))
    by = cap.bank_bytes().numpy()
    assert np.array_equal(by[..., :3], images) and np.array_equal(by[..., 3], masks)          # the mask's first channel is the alpha
    # rotations: proper, camera looking down -z of an OpenGL pose whatever the sign of P
    Rm = cap.poses[:, :3, :3].double().numpy()
    assert np.allclose(np.linalg.det(Rm), 1, atol=1e-5) and np.allclose(Rm @ Rm.transpose(0, 2, 1), np.eye(3), atol=1e-5)
    # scale == -1 means 1
    one, auto = C.Capture.load_dtu(root, split="all", scale=1), C.Capture.load_dtu(root, split="all")
    assert torch.equal(one.poses, auto.poses) and auto.scale == 1.0
    # downscale: the box mean, and the rows divided (the reference leaves them at full size)
    half = C.Capture.load_dtu(root, split="all", downscale=2)
    assert (half.H, half.W) == (5, 6) and np.array_equal(half.intrinsics_host, auto.intrinsics_host / 2)
    assert torch.equal(half.bank, C.box_downscale(auto.bank, DTU_H, DTU_W, 2))


def test_decompose_projection_signs():
    Ks, Rs, Cs = _dtu_cameras()
    for s in (1.0, -2.0):
        P = s * Ks[0] @ np.concatenate([Rs[0], -(Rs[0] @ Cs[0])[:, None]], 1)
        K, R, Cc = C.decompose_projection(P)
        assert (np.diag(K) > 0).all() and K[2, 2] == 1 and abs(np.linalg.det(R) - 1) < 1e-12 and np.allclose(np.tril(K, -1), 0)
        assert np.allclose(K, Ks[0], atol=1e-12) and np.allclose(R, Rs[0], atol=1e-12) and np.allclose(Cc, Cs[0], atol=1e-12)


def test_dtu_splits(tmp_path):
    root = str(tmp_path / "scan")
    _write_dtu(root)
    full = C.Capture.load_dtu(root, split="all")
    assert len(C.Capture.load_dtu(root, split="trainval")) == DTU_V
    val, train = C.Capture.load_dtu(root, split="val"), C.Capture.load_dtu(root, split="train")
    assert len(val) == 1 and len(train) == DTU_V - 1
    assert torch.equal(val.poses, full.poses[:1]) and torch.equal(val.bank, full.bank[:1])
    assert torch.equal(train.poses, full.poses[1:]) and torch.equal(train.bank, full.bank[1:])
    assert np.array_equal(train.intrinsics_host, full.intrinsics_host[1:])
    assert val.per_view_intrinsics is False and val.intrinsics == tuple(full.intrinsics_host[0])      # one view: one camera
    with pytest.raises(ValueError, match="split"):
        C.Capture.load_dtu(root, split="test")


def test_dtu_missing_mask_is_named(tmp_path):
    root = str(tmp_path / "scan")
    _write_dtu(root)
    os.remove(os.path.join(root, "mask", "003.png"))
    with pytest.raises(FileNotFoundError, match="003.png"):
        C.Capture.load_dtu(root, split="all")
    assert len(C.Capture.load_dtu(root, split="val")) == 1                  # the first frame has its mask
    with pytest.raises(FileNotFoundError, match="cameras_sphere"):
        C.Capture.load_dtu(str(tmp_path))


@pytest.mark.parametrize("shared", [False, True])
def test_save_dtu_then_load_dtu(tmp_path, shared):
    poses = synthetic.make_cameras(5, seed=4)
    rows = np.array([[30.0 + 1.37 * v, 28.5 - 0.9 * v, 12.2 + 0.3 * v, 9.7 - 0.21 * v] for v in range(5)])
    a = C.Capture.synthetic(poses, H=20, W=24, intrinsics=tuple(rows[0]) if shared else rows)
    a.save_dtu(str(tmp_path), scale=0.8, offset=(0.1, 0.0, -0.05))
    b = C.Capture.load_dtu(str(tmp_path), split="all", scale=0.8, offset=(0.1, 0.0, -0.05))
    assert torch.equal(a.bank, b.bank) and (a.H, a.W, a.has_alpha) == (b.H, b.W, b.has_alpha)
    want = np.tile(rows[0], (5, 1)) if shared else rows
    e_rows = float(np.abs((b.intrinsics_host if b.per_view_intrinsics else np.tile(b.intrinsics, (5, 1))) / want - 1).max())
    e_poses = float((a.poses.double() - b.poses.double()).abs().max() / a.poses.double().abs().max())
    print(f"save_dtu -> load_dtu: rows {e_rows:.3g}, poses {e_poses:.3g}")
    assert e_rows <= 4 * DTU_ROWS_MEASURED and e_poses <= 4 * DTU_POSES_MEASURED
