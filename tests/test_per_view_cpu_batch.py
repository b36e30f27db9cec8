"""The torch statements of a set with per-view intrinsics, on the CPU: capture.batch_from_uniforms_u8 with the table [V,4] against the same
statement called with each view's tuple, and NeRFRenderer.mark_untrained_grid with [B,4] against the tuple form called one view at a time.
Bit for bit: the table's fp32 entries are the roundings torch applies to the tuple's Python floats."""
import numpy as np
import pytest
import torch

from nerf2mesh_amd import synthetic
from nerf2mesh_amd.capture import Capture, batch_from_uniforms_u8, batch_sparse_u8, SparseDepth

V, H, W, N = 3, 5, 7, 1000
ROWS = np.array([[9.5, 7.25, 3.3, 2.85], [8.7, 8.1, 3.9, 2.2], [10.2, 6.9, 3.05, 2.65]])       # all different, some no fp32 numbers
NAMES = ("rays_o", "rays_d", "rgba", "nears", "fars", "noises", "bg", "gt_depth")


def _capture(cnf):
    g = torch.Generator().manual_seed(5)
    images = torch.randint(0, 256, (V, H, W, 4), generator=g, dtype=torch.uint8)
    poses = synthetic.make_cameras(V, seed=1)
    near_far = synthetic.cam_near_far(poses, "lego", H, W, float(ROWS[0, 0])) if cnf else None
    cap = Capture.from_arrays(poses, images, ROWS, cam_near_far=near_far)
    cap.dense_depth = torch.rand(V, H * W, generator=g) * 3 + 0.5
    return cap


def _uniforms():
    """tests/test_capture_kernels_gpu.py's uniforms: the four edge rows (first / last view and pixel) in front of random ones."""
    u = torch.rand(N, 6, generator=torch.Generator().manual_seed(9))
    below_one = torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))
    u[0, :2] = 0.0
    u[1, :2] = below_one
    u[2, 0], u[2, 1] = 0.0, below_one
    u[3, 0], u[3, 1] = below_one, 0.0
    return u


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("cnf", [False, True])
def test_table_equals_the_tuple_of_each_view(cnf, dense):
    cap = _capture(cnf)
    u = _uniforms()
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1])
    kw = dict(cam_near_far=cap.cam_near_far, dense_depth=cap.dense_depth if dense else None)
    assert cap.per_view_intrinsics and tuple(cap.intrinsics.shape) == (V, 4)
    counter = torch.full((1,), 5, dtype=torch.int32)
    got = batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, aabb, 0.05, H, W, cap.intrinsics, counter=counter, **kw)
    assert len(got) == (8 if dense else 7) and int(counter) == 0
    cam = (u[:, 0] * V).long().clamp(max=V - 1)
    assert cam[:4].tolist() == [0, V - 1, 0, V - 1] and all((cam == v).sum() > 100 for v in range(V))
    for v in range(V):
        want = batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, aabb, 0.05, H, W, cap.intrinsics_of(v), **kw)
        other = batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, aabb, 0.05, H, W, cap.intrinsics_of((v + 1) % V), **kw)
        m = cam == v
        for a, b, name in zip(got, want, NAMES):
            assert torch.equal(a[m], b[m]), (v, name)
        assert not torch.equal(got[1][m], other[1][m])                  # the rows matter
    # the host array is taken like the device table
    again = batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, aabb, 0.05, H, W, cap.intrinsics_host, **kw)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="per-view intrinsics must be"):
        batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, aabb, 0.05, H, W, cap.intrinsics[:2], **kw)


def test_sparse_batch_takes_the_row_of_its_view():
    cap = _capture(True)
    g = torch.Generator().manual_seed(2)
    counts = [6, 9, 4]
    K = sum(counts)
    coords = torch.stack([torch.randint(0, H, (K,), generator=g), torch.randint(0, W, (K,), generator=g)], -1)
    sd = SparseDepth(np.concatenate([[0], np.cumsum(counts)]), coords, torch.rand(K, generator=g) + 1, torch.rand(K, generator=g))
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1])
    for v in range(V):
        u = torch.rand(counts[v], 6, generator=g)
        for table in (cap.intrinsics, cap.intrinsics_host):
            got = batch_sparse_u8(cap.poses, cap.bank, cap.lut, u, v, sd, aabb, 0.05, H, W, table, cam_near_far=cap.cam_near_far)
            want = batch_sparse_u8(cap.poses, cap.bank, cap.lut, u, v, sd, aabb, 0.05, H, W, cap.intrinsics_of(v), cam_near_far=cap.cam_near_far)
            for a, b in zip(got, want):
                assert torch.equal(a, b)


def test_mark_untrained_grid_with_a_table_is_the_or_over_views():
    """[B,4] against the tuple form one view at a time: a cell is kept when ANY camera sees it, so the kept cells of the table form are the
    union of the kept cells of the single-view calls (inside the training box in both).  grid_size 16, two cascades, every row different,
    narrow lenses so that no view sees everything."""
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    B = 5
    opt = make_options(bound=2, grid_size=16, min_near=0.05)
    poses = synthetic.make_cameras(B, seed=3)
    rows = torch.tensor([[60.0 + 7.3 * v, 55.0 - 4.1 * v, 10.0 + 0.7 * v, 8.0 - 0.45 * v] for v in range(B)])      # 20 x 16 px views
    cnf = torch.stack([torch.full((B,), 0.3), torch.full((B,), 6.0)], -1) + torch.arange(B).float().unsqueeze(1) * 0.05

    c = torch.arange(16)
    cells = 2 * torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3).float() / 15 - 1

    def kept(p, intr, near_far):
        torch.manual_seed(0)
        m = NeRFNetwork(opt)
        assert m.cascade == 2 and m.density_grid.shape == (2, 16 ** 3)
        m._cell_unit = cells             # the Morton walk is a device kernel; which order the cells come in does not matter to this test
        m.mark_untrained_grid(p, intr, cam_near_far=near_far)
        return m.density_grid != -1

    for near_far in (None, cnf):
        got = kept(poses, rows, near_far)
        union = torch.zeros_like(got)
        singles = []
        for v in range(B):
            one = kept(poses[v:v + 1], tuple(float(x) for x in rows[v]), None if near_far is None else near_far[v:v + 1])
            singles.append(one)
            union |= one
        assert torch.equal(got, union)
        assert 0 < int(got.sum()) < got.numel() and all(int(s.sum()) < int(got.sum()) for s in singles)
        assert len({int(s.sum()) for s in singles}) > 1
        # the numpy host copy is taken like the tensor; S smaller than B walks more than one chunk
        torch.manual_seed(0)
        m = NeRFNetwork(opt)
        m._cell_unit = cells
        m.mark_untrained_grid(poses, rows.double().numpy(), cam_near_far=near_far, S=2)
        assert torch.equal(m.density_grid != -1, got)
    with pytest.raises(ValueError, match="per-view intrinsics must be"):
        NeRFNetwork(opt).mark_untrained_grid(poses, rows[:3])
