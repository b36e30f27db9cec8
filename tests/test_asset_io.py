"""Readers of the stage-1 export (export.read_obj / read_mlp_json / read_jpg: the inverses of the writers) and the float64
restatement of the asset's shader (tests/asset_ref.py) on cases small enough to work out by hand.  No GPU."""
import os

import numpy as np
import pytest

from nerf2mesh_amd import export
from nerf2mesh_amd.export import read_jpg, read_mlp_json, read_obj

import asset_ref


def _mesh(n_faces, seed):
    rng = np.random.default_rng(seed)
    nv = max(4, n_faces // 2 + 2)
    v = (rng.random((nv, 3)) * 2 - 1).astype(np.float32)
    f = rng.integers(0, nv, size=(n_faces, 3)).astype(np.int32)
    vt = rng.random((3 * n_faces, 2)).astype(np.float32)
    vt[0] = (0.0, 1.0)                                                 # the ends of the range go through the flip too
    vt[1] = (1.0, 0.0)
    ft = rng.permutation(3 * n_faces).astype(np.int32).reshape(n_faces, 3)
    return v, f, vt, ft


@pytest.mark.parametrize("n_faces", [2, 300])
def test_obj_round_trip(tmp_path, n_faces):
    v, f, vt, ft = _mesh(n_faces, seed=n_faces)
    path = export.write_obj(str(tmp_path), 3, v, f, vt, ft)
    assert os.path.basename(path) == "mesh_3.obj"
    rv, rf, rvt, rft = read_obj(path)
    assert rv.dtype == np.float32 and rf.dtype == np.int32 and rvt.dtype == np.float32 and rft.dtype == np.int32
    assert rv.shape == v.shape and rf.shape == f.shape and rvt.shape == vt.shape and rft.shape == ft.shape
    assert np.array_equal(rv, v) and np.array_equal(rf, f) and np.array_equal(rft, ft)
    assert np.array_equal(rvt[:, 0], vt[:, 0])
    # the flip 1 - v is done in float32 on the way out and undone in float32 on the way in: two float32 ulp at 1
    assert float(np.abs(rvt.astype(np.float64) - vt.astype(np.float64)).max()) <= 2.4e-7
    # the file itself holds the flipped value
    first_vt = [l for l in open(path).read().splitlines() if l.startswith("vt ")][0].split()
    assert float(first_vt[1]) == 0.0 and float(first_vt[2]) == 0.0     # vt[0] = (0, 1) -> "0.0 0.0"


def test_read_obj_rejects_faces_without_uv_indices(tmp_path):
    p = tmp_path / "bare.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    with pytest.raises(ValueError):
        read_obj(str(p))


def test_mlp_json_round_trip(tmp_path):
    import torch
    from nerf2mesh_amd.network import MLP

    class M:
        pass
    torch.manual_seed(5)
    m = M()
    m.specular_net = MLP(6, 3, 32, 2, bias=False)
    m.bound, m.cascade = 2, 2
    path = str(tmp_path / "mlp.json")
    export.write_mlp_json(path, m)
    got = read_mlp_json(path)
    w0, w1 = (p.detach().numpy() for p in m.specular_net.parameters())
    assert got["w0"].shape == (32, 6) and got["w1"].shape == (3, 32)
    assert got["w0"].dtype == np.float32 and got["w1"].dtype == np.float32
    assert np.array_equal(got["w0"].view(np.uint32), w0.view(np.uint32))          # bit-exact
    assert np.array_equal(got["w1"].view(np.uint32), w1.view(np.uint32))
    assert got["bound"] == 2 and got["cascade"] == 2


def test_jpg_round_trip_is_the_decoders_image(tmp_path):
    from PIL import Image
    yy, xx = np.mgrid[0:40, 0:56]
    x = np.stack([yy * 6, xx * 4, (yy + xx) * 2], axis=-1).astype(np.uint8)      # a gradient: row 0 is dark, the last row bright
    path = str(tmp_path / "t.jpg")
    export.write_jpg(path, x)
    got = read_jpg(path)
    assert got.dtype == np.uint8 and got.shape == (40, 56, 3)
    assert np.array_equal(got, np.asarray(Image.open(path)))
    assert got[:4].mean() < got[-4:].mean()                                      # row 0 first
    assert np.abs(got.astype(int) - x.astype(int)).mean() < 3                     # and it is the image that was written


# ---------------------------------------------------------------------------------------------- asset_ref by hand
def _one_triangle(uv):
    """A 1-pixel 'view' whose pixel sits at vertex-weighted uv `uv` of one triangle with uvs (0,0), (1,0), (0,1)."""
    vt = np.array([[0, 0], [1, 0], [0, 1]], np.float64)
    ft = np.array([[0, 1, 2]], np.int32)
    u, v = uv
    rast = np.array([[[1 - u - v, u, 0.5, 1.0]]])                                  # b0 (vertex 0), b1 (vertex 1); vertex 2 gets v
    return rast, ft, vt


TEX = np.array([[[10, 20, 30], [50, 60, 70]],
                [[90, 100, 110], [200, 220, 240]]], np.uint8)                        # [row][col]


def test_ref_nearest_returns_the_texel_at_each_texel_centre():
    z0, z1 = np.zeros((32, 6)), np.zeros((3, 32))
    for row in (0, 1):
        for col in (0, 1):
            rast, ft, vt = _one_triangle(((col + 0.5) / 2, (row + 0.5) / 2))
            for filt in ("nearest", "linear"):                                     # at a texel centre linear has weight 1 on that texel
                out = asset_ref.shade(rast, ft, vt, np.array([[0, 0, 2.0]]), [TEX], [TEX], [0], z0, z1, "diffuse", filt)
                assert np.allclose(out["rgb"][0] * 255, TEX[row, col], atol=1e-9), (row, col, filt)
                assert out["covered"][0] and out["cascade"][0] == 0
                assert np.isclose(out["x"][0], col + 0.5) and np.isclose(out["y"][0], row + 0.5)


def test_ref_linear_at_the_common_corner_is_the_mean_of_the_four():
    rast, ft, vt = _one_triangle((0.5, 0.5))
    out = asset_ref.shade(rast, ft, vt, np.array([[1.0, 0, 0]]), [TEX], [TEX], [0], np.zeros((32, 6)), np.zeros((3, 32)), "diffuse", "linear")
    assert np.allclose(out["rgb"][0] * 255, TEX.reshape(4, 3).astype(np.float64).mean(0), atol=1e-9)
    # and outside the outermost centres the border texel is repeated
    rast, ft, vt = _one_triangle((0.01, 0.02))
    out = asset_ref.shade(rast, ft, vt, np.array([[1.0, 0, 0]]), [TEX], [TEX], [0], np.zeros((32, 6)), np.zeros((3, 32)), "diffuse", "linear")
    assert np.allclose(out["rgb"][0] * 255, TEX[0, 0], atol=1e-9)


def test_ref_zero_weights_give_half_and_modes_combine():
    rast, ft, vt = _one_triangle((0.75, 0.25))                                     # texel row 0, col 1
    z0, z1 = np.zeros((32, 6)), np.zeros((3, 32))
    d = np.array([[0.0, 3.0, 4.0]])
    spec = asset_ref.shade(rast, ft, vt, d, [TEX], [TEX], [0], z0, z1, "specular")["rgb"][0]
    assert np.array_equal(spec, [0.5, 0.5, 0.5])
    full = asset_ref.shade(rast, ft, vt, d, [TEX], [TEX], [0], z0, z1, "full")["rgb"][0]
    assert np.allclose(full, np.clip(TEX[0, 1] / 255 + 0.5, 0, 1))
    # one hidden unit that reads the direction's z and the specular texel's red: the direction is normalised (4 / 5) and comes first
    w0, w1 = np.zeros((32, 6)), np.zeros((3, 32))
    w0[7, 2], w0[7, 3], w1[1, 7] = 2.0, 1.0, 3.0
    spec = asset_ref.shade(rast, ft, vt, d, [TEX], [TEX], [0], w0, w1, "specular")["rgb"][0]
    pre = 3.0 * (2.0 * 0.8 + TEX[0, 1, 0] / 255)
    assert np.allclose(spec, [0.5, 1 / (1 + np.exp(-pre)), 0.5])
    w0[7, 2] = -2.0                                                                  # relu: a negative pre-activation contributes nothing
    spec = asset_ref.shade(rast, ft, vt, d, [TEX], [TEX], [0], w0, w1, "specular")["rgb"][0]
    assert np.array_equal(spec, [0.5, 0.5, 0.5])


def test_ref_empty_pixels_and_cascades():
    vt = np.array([[0, 0], [1, 0], [0, 1], [0.2, 0.2], [0.9, 0.2], [0.2, 0.9]], np.float64)
    ft = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    rast = np.array([[[0.25, 0.5, 0.1, 0.0], [0.25, 0.5, 0.1, 1.0], [1.0, 0.0, 0.1, 2.0]]])       # empty, face 0, face 1 at its vertex 0
    other = (255 - TEX.astype(int)).astype(np.uint8)
    out = asset_ref.shade(rast, ft, vt, np.ones((3, 3)), [TEX, other], [TEX, other], [0, 1], np.zeros((32, 6)), np.zeros((3, 32)), "diffuse")
    assert list(out["covered"]) == [False, True, True] and list(out["cascade"]) == [-1, 0, 1]
    assert np.array_equal(out["rgb"][0], [0, 0, 0])
    assert np.allclose(out["rgb"][1] * 255, TEX[0, 1])                               # uv (0.5, 0.25)
    assert np.allclose(out["rgb"][2] * 255, other[0, 0])                             # uv (0.2, 0.2), second cascade's texture
    assert asset_ref.near_texel_boundary(np.array([1.00005, 0.5]), np.array([0.5, 0.5])).tolist() == [True, False]
