"""Stage-1 raster operators (include/n2m_raster.h) against the float64 restatement in tests/raster_ref.py.

CPU part (unmarked): the float64 reference is first checked against its own central differences and against the float32 C oracle
(oracle/n2m_raster_oracle.c), so that it can be trusted as the yardstick.
GPU part: rasterize / interpolate / antialias, forward and backward, on the HIP kernels -- welded perspective mesh, camera inside a closed
surface (w <= 0, the float path, a face beyond 2^20 px), slivers, an open patch with a three-face (fin) edge, and the stage-1 geometry
chain at 512 x 512 -- within the tolerance rule of raster_ref (derived from float32 conditioning and the atomic-sum bound, not tuned).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_simplify_ref as MR  # noqa: E402
import raster_ref as R  # noqa: E402

RESOLUTIONS = [(96, 128), (203, 117), (1, 64), (64, 1), (2, 2)]
SCENES = ["welded", "inside", "slivers", "fin"]


# ------------------------------------------------------------------------------------------------ scenes (clip-space meshes, fixed seeds)

def _mvp(eye, target, focal=1.4, near=0.05, far=100.0):
    """OpenGL projection @ view for a camera at `eye` looking at `target` (float64, resolution independent)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    up = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, up); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = right, up, -fwd
    view[:3, 3] = -view[:3, :3] @ eye
    proj = np.array([[focal, 0, 0, 0], [0, focal, 0, 0], [0, 0, -(far + near) / (far - near), -2 * far * near / (far - near)], [0, 0, -1, 0]])
    return proj @ view


def _clip(v, mvp):
    v = np.asarray(v, np.float64)
    return (np.concatenate([v, np.ones((len(v), 1))], 1) @ mvp.T).astype(np.float32)


def _floaters(rng, n, w_lo=0.7, w_hi=2.5):
    c = rng.uniform(-1.0, 1.0, (n, 1, 2))
    xy = (c + rng.normal(0, 0.15, (n, 3, 2))).reshape(-1, 2)
    z = np.repeat(rng.uniform(-0.9, 0.9, (n, 1)), 3, 1).reshape(-1, 1) + rng.normal(0, 0.03, (n * 3, 1))
    w = rng.uniform(w_lo, w_hi, (n * 3, 1))
    return np.concatenate([xy * w, z * w, w], 1).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


def _concat(*meshes):
    pos, tri, base = [], [], 0
    for p, t in meshes:
        pos.append(p); tri.append(t + base); base += len(p)
    return np.concatenate(pos).astype(np.float32), np.concatenate(tri).astype(np.int32)


def scene_welded():
    """(a) A jittered icosphere(3) -- every vertex shared by ~6 faces, so every gradient is a sum of atomics -- with w in [0.7, 2.5],
    plus floating triangles."""
    rng = np.random.default_rng(11)
    v, f = MR.icosphere(3)
    v = v.astype(np.float64) + rng.normal(0, 0.01, v.shape)
    w = 1.6 + 0.9 * v[:, 2] / np.abs(v[:, 2]).max()
    pos = np.stack([0.75 * v[:, 0] * w, 0.75 * v[:, 1] * w, 0.5 * v[:, 2] * w, w], 1).astype(np.float32)
    return _concat((pos, f), _floaters(rng, 60))


def scene_inside():
    """(b) The camera inside a closed sphere: faces behind the eye (w < 0), faces crossing w = 0, one extra face with every w < 0, and
    one face with a vertex at w = 1e-4 that projects beyond 2^20 px (float path although every w > 0)."""
    rng = np.random.default_rng(12)
    v, f = MR.icosphere(2, radius=2.0)
    v = v.astype(np.float64) + rng.normal(0, 0.02, v.shape)
    pos = _clip(v, _mvp([0.1, -0.2, 0.05], [1.0, 0.3, 0.2]))
    behind = np.array([[0.2, 0.1, -0.5, -0.9], [-0.4, 0.3, -0.6, -1.2], [0.1, -0.5, -0.4, -0.7]], np.float32)
    # x / w = 3e6: beyond 2^20 px at every resolution of RESOLUTIONS, W = 1 included; z / w = 0.4 on the whole face
    far = np.array([[-0.3 * 0.8, -0.2 * 0.8, 0.4 * 0.8, 0.8], [300.0, 1e-5, 0.4e-4, 1e-4], [-0.1, 0.5, 0.4, 1.0]], np.float32)
    return _concat((pos, f), (behind, np.array([[0, 1, 2]], np.int32)), (far, np.array([[0, 1, 2]], np.int32)))


def scene_slivers():
    """(c) Slivers: about 1:1000 on screen (100 px x 0.1 px at 128 px), non-degenerate in clip space, perspective w, over a welded
    background quad."""
    rng = np.random.default_rng(13)
    pos, tri = [], []
    for i in range(24):
        c = rng.uniform(-0.6, 0.6, 2)
        ang = rng.uniform(0, np.pi)
        d = np.array([np.cos(ang), np.sin(ang)])
        nrm = np.array([-d[1], d[0]])
        L = rng.uniform(1.2, 1.6)
        xy = np.stack([c - 0.5 * L * d, c + 0.5 * L * d, c + rng.uniform(-0.3, 0.3) * L * d + 1.6e-3 * nrm])
        w = rng.uniform(0.7, 2.5, 3)
        z = rng.uniform(-0.5, 0.3)
        pos += [[xy[k, 0] * w[k], xy[k, 1] * w[k], z * w[k], w[k]] for k in range(3)]
        tri.append([3 * i, 3 * i + 1, 3 * i + 2] if i % 2 else [3 * i, 3 * i + 2, 3 * i + 1])
    bg = np.array([[-0.9, -0.8, 0.6, 1], [0.85, -0.9, 0.6, 1], [0.9, 0.9, 0.6, 1], [-0.8, 0.85, 0.6, 1]], np.float32) * 1.3
    return _concat((np.asarray(pos, np.float32), np.asarray(tri, np.int32)), (bg, np.array([[0, 1, 2], [0, 2, 3]], np.int32)))


FIN_EYE = (0.013, 0.9, 1.1)
FIN_TARGET = (0.007, 0.011, 0.0)


def fin_mesh():
    """(d) world-space open patch (boundary edges) with a fin: a third face on an interior edge (MR.with_fin).  The fin face is the last
    face; face 0 is the fin's base face.  Returns (v, f, (a, b, c, d, tip)) with d the neighbour's opposite vertex."""
    v, f = MR.grid_patch(8, 1.0 / 8)
    v = v.astype(np.float64) - np.array([0.5, 0.5, 0.0])
    k = int(np.nonzero((f == 4 * 9 + 4).any(1) & (f == 5 * 9 + 4).any(1))[0][0])       # a face on the interior edge (4,4)-(5,4)
    a, b = 4 * 9 + 4, 5 * 9 + 4
    c = int(next(x for x in f[k] if x not in (a, b)))
    f = np.concatenate([f[k:k + 1], np.delete(f, k, 0)])
    f[0] = [a, b, c]
    v2, f2 = MR.with_fin(v.astype(np.float32), f)
    nb = [i for i in range(1, len(f)) if a in f[i] and b in f[i]]
    d = int(next(x for x in f[nb[0]] if x not in (a, b)))
    return v2, f2, (a, b, c, d, len(v2) - 1)


def scene_fin():
    v, f, _ = fin_mesh()
    return _clip(v, _mvp(FIN_EYE, FIN_TARGET)), f


BUILDERS = {"welded": scene_welded, "inside": scene_inside, "slivers": scene_slivers, "fin": scene_fin}
_SCENES = {}


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = BUILDERS[name]()
    return _SCENES[name]


def oracle_rast(name, H, W):
    from oracle import oracle as orc
    pos, tri = scene(name)
    return orc.rasterize(pos, tri, H, W)


# ================================================================================================ CPU: the reference itself

def _fd(fn, x, i, h):
    xp, xm = x.clone(), x.clone()
    xp.view(-1)[i] += h; xm.view(-1)[i] -= h
    return (fn(xp) - fn(xm)) / (2 * h)


def test_reference_autograd_matches_central_differences():
    """float64 autograd of (u, v), interpolate and the antialias blend against float64 central differences, ~1e-7 relative, on a few
    hundred random pixels / pixel pairs of the welded, camera-inside and sliver scenes (ambiguous pairs skipped; the camera-inside scene
    has no pair that float32 decides, its silhouette belongs to the face beyond 2^20 px)."""
    rng = np.random.default_rng(5)
    for name in ("welded", "inside", "slivers"):
        H, W = 96, 128
        pos, tri = scene(name)
        rast = oracle_rast(name, H, W)
        ids = torch.as_tensor(rast[..., 3]).long() - 1
        p, f, c = R.covered_corners(pos, tri, ids)
        sel = torch.as_tensor(rng.choice(len(p), 300, replace=False))
        p, c = p[sel], c[sel]
        fx, fy = R.pixel_ndc(p % W, p // W, H, W)
        wts = torch.as_tensor(rng.normal(size=(len(p), 2)))
        g = lambda cc: (R.uvz(cc, fx, fy)[:, :2] * wts).sum()          # noqa: E731
        cc = c.clone().requires_grad_(True)
        (ga,) = torch.autograd.grad(g(cc), cc)
        for i in rng.choice(c.numel(), 60, replace=False):
            if i % 4 == 2:
                continue
            h = 1e-6 * max(1.0, float(c.view(-1)[i].abs()))
            fd = float(_fd(g, c.detach(), int(i), h))
            assert abs(fd - float(ga.view(-1)[i])) <= 1e-7 * max(1.0, abs(fd)), (name, i, fd, float(ga.view(-1)[i]))
        # interpolate: out = u a0 + v a1 + (1 - u - v) a2, gradients w.r.t. (u, v) and the attributes
        attr = torch.as_tensor(rng.normal(size=(len(pos), 3)))
        vid = torch.as_tensor(tri).long()[f[sel]]
        uv = torch.as_tensor(rast.reshape(-1, 4)[p.numpy(), :2]).double()
        wo = torch.as_tensor(rng.normal(size=(len(p), 3)))

        def interp(uv_, at):
            b = torch.stack([uv_[:, 0], uv_[:, 1], 1 - uv_[:, 0] - uv_[:, 1]], 1)
            return ((b[..., None] * at[vid]).sum(1) * wo).sum()
        u1, a1 = uv.clone().requires_grad_(True), attr.clone().requires_grad_(True)
        gu, gat = torch.autograd.grad(interp(u1, a1), [u1, a1])
        for i in rng.choice(uv.numel(), 30, replace=False):
            fd = float(_fd(lambda x: interp(x, attr), uv, int(i), 1e-6))
            assert abs(fd - float(gu.view(-1)[i])) <= 1e-7 * max(1.0, abs(fd))
        used = torch.unique(vid).numpy()
        for v in rng.choice(used, 20, replace=False):
            i = int(v) * 3 + int(rng.integers(3))
            fd = float(_fd(lambda x: interp(uv, x), attr, i, 1e-6))
            assert abs(fd - float(gat.view(-1)[i])) <= 1e-7 * max(1.0, abs(fd))
        # antialias blend: d of the crossing edge w.r.t. its two clip-space end points
        color = rng.random((H, W, 3))
        _, _, _, pr = R.antialias_ref(color, rast, pos, tri)
        keep = ~pr["amb_found"]
        n = int(keep.sum())
        if name == "inside":
            continue
        assert n > 20
        k = torch.as_tensor(rng.choice(n, min(n, 200), replace=False))
        P, O = pr["P"][keep][k], pr["O"][keep][k]
        pos64 = torch.as_tensor(pos).double()
        ab = torch.stack([pos64[pr["va"][keep][k]], pos64[pr["vb"][keep][k]]], 1)
        Pxy = torch.stack([(P % W).double() + 0.5, (P // W).double() + 0.5], 1)
        Oxy = torch.stack([(O % W).double() + 0.5, (O // W).double() + 0.5], 1)
        wd = torch.as_tensor(rng.normal(size=len(P)))
        blend = lambda x: ((0.5 - R._pair_d(x, Pxy, Oxy, W, H)).abs() * wd).sum()    # noqa: E731
        x1 = ab.clone().requires_grad_(True)
        (gab,) = torch.autograd.grad(blend(x1), x1)
        for i in rng.choice(ab.numel(), 60, replace=False):
            if i % 4 == 2:
                continue
            h = 1e-7 * max(1.0, float(ab.view(-1)[i].abs()))
            fd = float(_fd(blend, ab, int(i), h))
            assert abs(fd - float(gab.view(-1)[i])) <= 1e-7 * max(1.0, abs(fd)), (name, i, fd, float(gab.view(-1)[i]))


def test_inside_scene_takes_the_float_path():
    """Scene (b) holds what it claims at every resolution: faces with a vertex at w <= 0 and faces crossing w = 0, and one face (the
    last) with every w > 0 that still takes the float path because a vertex projects beyond 2^20 px; that face covers pixels at the full
    resolutions."""
    pos, tri = scene("inside")
    w = torch.as_tensor(pos)[torch.as_tensor(tri).long()][..., 3]
    assert bool(((w > 0).any(1) & (w <= 0).any(1)).any()) and bool((w < 0).all(1).any())
    far = len(tri) - 1
    assert bool((w[far] > 0).all())
    for H, W in RESOLUTIONS:
        fixed = R.fixed_path(pos, tri, H, W)
        assert not bool(fixed[far]), (H, W)
        assert not bool((fixed | ~(w > 1e-12).all(1))[:far].logical_not().any())        # the only all-positive face off the fixed path
        if H * W > 1000:
            ids, _ = R.rasterize_truth(pos, tri, H, W)
            assert int((ids == far).sum()) > 0, (H, W)


@pytest.mark.parametrize("name", SCENES)
def test_oracle_rasterize_matches_float64_truth(name):
    """The C oracle's ids equal the float64 coverage truth on every pixel outside the decision margin; the margin stays below 1 % of the
    covered pixels at the two full resolutions."""
    pos, tri = scene(name)
    for H, W in RESOLUTIONS:
        ids, amb = R.rasterize_truth(pos, tri, H, W)
        got = torch.as_tensor(oracle_rast(name, H, W)[..., 3]).long() - 1
        bad = (got != ids) & ~amb
        assert not bool(bad.any()), f"{name} {H}x{W}: {int(bad.sum())} pixels with another id outside the margin"
        if H * W > 1000:
            assert int(amb.sum()) < 0.01 * max(int((ids >= 0).sum()), 1), (name, H, W, int(amb.sum()))


@pytest.mark.parametrize("name", SCENES)
def test_oracle_interpolate_and_antialias_within_the_rule(name):
    """The oracle's (u, v, z/w), interpolate and antialias forward against float64 under the tolerance rule."""
    from oracle import oracle as orc
    pos, tri = scene(name)
    rng = np.random.default_rng(3)
    for H, W in RESOLUTIONS[:3]:
        rast = oracle_rast(name, H, W)
        ids = torch.as_tensor(rast[..., 3]).long() - 1
        vals, _ = R.rasterize_fields(pos, tri, ids, H, W)
        R.check(rast[..., :3].reshape(-1, 3), vals, f"{name} {H}x{W} oracle (u, v, z/w)", mask=(ids >= 0))
        attr = rng.normal(size=(len(pos), 4)).astype(np.float32)
        out, _, _ = R.interpolate_ref(attr, rast, tri)
        R.check(orc.interpolate(attr, rast, tri), out, f"{name} {H}x{W} oracle interpolate")
        color = rng.random((H, W, 3)).astype(np.float32)
        aa, _, _, pr = R.antialias_ref(color, rast, pos, tri)
        R.check(orc.antialias(color, rast, pos, tri), aa, f"{name} {H}x{W} oracle antialias", mask=~R.ambiguous_pixels(pr, H * W))


def _remap(rast, perm):
    """rast of the faces tri[perm]: the same image with every id renamed."""
    inv = np.empty_like(perm); inv[perm] = np.arange(len(perm))
    r = rast.copy()
    ids = r[..., 3].astype(np.int64) - 1
    r[..., 3] = np.where(ids >= 0, inv[np.maximum(ids, 0)] + 1, 0).astype(np.float32)
    return r


def _fin_orders(F):
    rng = np.random.default_rng(9)
    return {"identity": np.arange(F), "reversed": np.arange(F)[::-1].copy(), "fin_first": np.r_[F - 1, np.arange(F - 1)],
            "random": rng.permutation(F)}


def test_fin_view_decides_on_the_fin_edge():
    """Scene (d) is a real test of the non-manifold rule: on screen the fin tip lies on one side of the shared edge and one of the two
    patch faces' opposite vertices on the other, so the image depends on which two of the three faces an edge table keeps; the rule
    (an edge with more than two faces is a silhouette) removes that choice, and the C oracle follows it whatever the order of the faces."""
    from oracle import oracle as orc
    v, f, (a, b, c, d, tip) = fin_mesh()
    pos, tri = scene("fin")
    H, W = 96, 128
    px = lambda i: ((pos[i, 0] / pos[i, 3] * 0.5 + 0.5) * W, (pos[i, 1] / pos[i, 3] * 0.5 + 0.5) * H)     # noqa: E731
    A, B = np.array(px(a)), np.array(px(b))
    side = lambda i: np.sign(np.cross(B - A, np.array(px(i)) - A))     # noqa: E731
    assert side(c) != side(d) and side(tip) in (side(c), side(d))        # the tip on one face's side: its edge is a 'fold' for that face
    rast = oracle_rast("fin", H, W)
    color = np.random.default_rng(0).random((H, W, 3)).astype(np.float32)
    rule, _, _, _ = R.antialias_ref(color, rast, pos, tri)
    F = len(tri)
    base = R.opposite_table(tri, len(pos))
    nb = [i for i in range(1, F - 1) if a in tri[i] and b in tri[i]][0]
    kof = lambda fi: next(k for k in range(3) if {tri[fi][k], tri[fi][(k + 1) % 3]} == {a, b})     # noqa: E731
    images = []
    for keep in ((0, nb), (0, F - 1), (nb, F - 1)):                   # the two faces an insertion race could have kept
        oth = base.copy()
        for fi in (0, nb, F - 1):
            others = [g for g in keep if g != fi]
            oth[fi, kof(fi)] = next(x for x in tri[others[0]] if x not in (a, b)) if fi in keep else \
                next(x for x in tri[keep[0]] if x not in (a, b))
        two, _, _, _ = R.antialias_ref(color, rast, pos, tri, other=oth)
        images.append(two.ref)
    assert any(bool((x != images[0]).any()) for x in images[1:]), "which two faces the table keeps does not matter in this view"
    ref = orc.antialias(color, rast, pos, tri)
    for nm, perm in _fin_orders(F).items():
        got = orc.antialias(color, _remap(rast, perm), pos, tri[perm])
        np.testing.assert_array_equal(got, ref, err_msg=nm)


# ================================================================================================ GPU: the HIP kernels

class Dev:
    """The raw C entries of include/n2m_raster.h on one scene (device tensors; every call on torch's current stream)."""

    def __init__(self, pos, tri):
        from nerf2mesh_amd import _lib as L
        from nerf2mesh_amd import raster
        self.L, self.raster = L, raster
        self.pos = torch.as_tensor(np.asarray(pos, np.float32)).cuda().contiguous()
        self.tri = torch.as_tensor(np.asarray(tri, np.int32)).cuda().contiguous()
        self.V, self.F = self.pos.shape[0], self.tri.shape[0]
        self.table = raster.antialias_construct_topology_hash(self.tri)

    def c(self, name, *args):
        self.L.call(name, *args, self.L.stream())

    def rasterize(self, H, W):
        rast = torch.empty(H, W, 4, device="cuda")
        zbuf = torch.empty(H * W, dtype=torch.int64, device="cuda")
        self.c("n2m_rasterize_forward", self.pos.data_ptr(), self.tri.data_ptr(), self.V, self.F, H, W, zbuf.data_ptr(), rast.data_ptr())
        return rast

    def rasterize_backward(self, rast, d_rast):
        gp = torch.zeros(self.V, 4, device="cuda")
        H, W = rast.shape[:2]
        self.c("n2m_rasterize_backward", self.pos.data_ptr(), self.tri.data_ptr(), rast.data_ptr(), d_rast.data_ptr(), self.V, self.F, H, W,
               gp.data_ptr())
        return gp

    def interpolate(self, attr, rast):
        H, W = rast.shape[:2]
        out = torch.empty(H, W, attr.shape[1], device="cuda")
        self.c("n2m_interpolate_forward", attr.data_ptr(), rast.data_ptr(), self.tri.data_ptr(), self.V, self.F, attr.shape[1], H, W, out.data_ptr())
        return out

    def interpolate_backward(self, attr, rast, d_out, stride=None, offset=0, with_attr=True):
        H, W = rast.shape[:2]
        A = attr.shape[1]
        ga = torch.zeros_like(attr) if with_attr else None
        gr = torch.full((H, W, 4), float("nan"), device="cuda")
        args = (attr.data_ptr(), rast.data_ptr(), self.tri.data_ptr(), d_out.data_ptr() + 4 * offset)
        tail = (self.V, self.F, A, H, W, ga.data_ptr() if with_attr else None, gr.data_ptr())
        if stride is None:
            self.c("n2m_interpolate_backward", *args, *tail)
        else:
            self.c("n2m_interpolate_backward_strided", *args, stride, *tail)
        return ga, gr

    def antialias(self, color, rast, table=None, tri=None):
        H, W, C = color.shape
        tri = self.tri if tri is None else tri
        table = self.table if table is None else table
        out = torch.empty_like(color)
        self.c("n2m_antialias_forward", color.data_ptr(), rast.data_ptr(), self.pos.data_ptr(), tri.data_ptr(), table.data_ptr(), table.shape[0],
               self.V, self.F, C, H, W, out.data_ptr())
        return out

    def antialias_backward(self, color, rast, d_out, boost=1.0, seeded=False, table=None, tri=None):
        H, W, C = color.shape
        tri = self.tri if tri is None else tri
        table = self.table if table is None else table
        gc = d_out.clone() if seeded else torch.full_like(color, float("nan"))
        gp = torch.zeros(self.V, 4, device="cuda")
        self.c("n2m_antialias_backward_seeded" if seeded else "n2m_antialias_backward", color.data_ptr(), rast.data_ptr(), self.pos.data_ptr(),
               tri.data_ptr(), table.data_ptr(), table.shape[0], d_out.data_ptr(), self.V, self.F, C, H, W, float(boost), gc.data_ptr(), gp.data_ptr())
        return gc, gp


_DEV = {}


def dev_scene(name, H, W):
    """(Dev, device rast) of a scene at a resolution, computed once per session."""
    if (name, H, W) not in _DEV:
        d = _DEV.get(name) or Dev(*scene(name))
        _DEV[name] = d
        _DEV[(name, H, W)] = d.rasterize(H, W)
    return _DEV[name], _DEV[(name, H, W)]


def _atomic_only(sc):
    """|a - b| bound for two device results that sum the same terms in different orders: twice the any-order bound."""
    return 2 * sc.cnt * R.U32 * sc.abs + 2.0 ** -30


def _same_terms(a, b, sc, what, mask=None):
    err = (torch.as_tensor(np.asarray(a)).double().reshape(sc.n, sc.k) - torch.as_tensor(np.asarray(b)).double().reshape(sc.n, sc.k)).abs()
    bad = ~(err <= _atomic_only(sc))
    if mask is not None:
        bad &= torch.as_tensor(np.asarray(mask)).reshape(-1, 1).bool()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ beyond the atomic-sum bound (max {float(err.max()):.3g})"


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", RESOLUTIONS)
@pytest.mark.parametrize("name", SCENES)
def test_rasterize_forward_backward_f64(name, H, W):
    """Device ids equal the float64 truth outside the margin; (u, v, z/w) on the device ids and grad_pos of sum(d_rast * rast) within the
    rule; the z column of grad_pos and the rows of vertices no covered pixel references are exactly 0."""
    d, rast = dev_scene(name, H, W)
    pos, tri = scene(name)
    ids64, amb = R.rasterize_truth(pos, tri, H, W)
    got = rast.cpu()
    ids = got[..., 3].long() - 1
    bad = (ids != ids64) & ~amb
    assert not bool(bad.any()), f"{int(bad.sum())} pixels with another id outside the margin"
    if name == "inside" and H * W > 1000:
        assert int((ids == len(tri) - 1).sum()) > 0, "the face beyond 2^20 px (float path) owns no pixel"
    rng = np.random.default_rng(H * 7 + W)
    d_rast = torch.as_tensor(rng.normal(size=(H, W, 4)).astype(np.float32))
    vals, grads = R.rasterize_fields(pos, tri, ids, H, W, d_rast=d_rast)
    R.check(got[..., :3].reshape(-1, 3), vals, "(u, v, z/w)", mask=(ids >= 0))
    gp = d.rasterize_backward(rast, d_rast.cuda()).cpu()
    R.check(gp.reshape(-1, 1), grads, "rasterize grad_pos")
    assert bool((gp[:, 2] == 0).all())
    used = torch.zeros(len(pos), dtype=torch.bool)
    used[torch.as_tensor(tri).long()[ids[ids >= 0]].reshape(-1)] = True
    assert bool((gp[~used] == 0).all())
    if (ids >= 0).sum() > 100:
        assert float(gp.abs().sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", RESOLUTIONS)
@pytest.mark.parametrize("name", SCENES)
def test_interpolate_f64(name, H, W):
    """out, grad_attr and grad_rast (channels 0, 1) within the rule for A in {1, 3, 4, 7}; channels 2, 3 exactly 0; the strided entry on
    one channel of an RGBA gradient, and the entry without grad_attr, give grad_rast bit for bit."""
    d, rast = dev_scene(name, H, W)
    pos, tri = scene(name)
    rng = np.random.default_rng(H + 3 * W)
    rast_c = rast.cpu()
    for A in (1, 3, 4, 7):
        attr = torch.as_tensor(rng.normal(size=(len(pos), A)).astype(np.float32))
        d_out = torch.as_tensor(rng.normal(size=(H, W, A)).astype(np.float32))
        out_ref, ga_ref, gr_ref = R.interpolate_ref(attr, rast_c, tri, d_out)
        a_d, g_d = attr.cuda(), d_out.cuda()
        R.check(d.interpolate(a_d, rast).cpu().reshape(-1, A), out_ref, f"interpolate out A={A}")
        ga, gr = d.interpolate_backward(a_d, rast, g_d)
        R.check(ga.cpu().reshape(-1, 1), ga_ref, f"interpolate grad_attr A={A}")
        gr = gr.cpu()
        R.check(gr[..., :2].reshape(-1, 2), gr_ref, f"interpolate grad_rast A={A}")
        assert bool((gr[..., 2:] == 0).all())
        _, gr_noattr = d.interpolate_backward(a_d, rast, g_d, with_attr=False)
        assert torch.equal(gr_noattr.cpu(), gr)
    attr1 = torch.as_tensor(rng.normal(size=(len(pos), 1)).astype(np.float32)).cuda()
    rgba = torch.as_tensor(rng.normal(size=(H, W, 4)).astype(np.float32)).cuda()
    _, g_plain = d.interpolate_backward(attr1, rast, rgba[..., 3].contiguous(), with_attr=False)
    _, g_str = d.interpolate_backward(attr1, rast, rgba, stride=4, offset=3, with_attr=False)
    assert torch.equal(g_plain, g_str)
    if int((rast_c[..., 3] > 0).sum()) > 0:
        assert float(g_plain[..., :2].abs().sum()) > 0
    attr3 = torch.as_tensor(rng.normal(size=(len(pos), 3)).astype(np.float32)).cuda()
    _, g_p = d.interpolate_backward(attr3, rast, rgba[..., :3].contiguous())
    _, g_s = d.interpolate_backward(attr3, rast, rgba, stride=4)
    assert torch.equal(g_p, g_s)


def _aa_case(name, H, W, C, seed):
    """color, d_out (zeroed on both pixels of every ambiguous pair) and the float64 reference at boost 1."""
    d, rast = dev_scene(name, H, W)
    pos, tri = scene(name)
    rng = np.random.default_rng(seed)
    color = torch.as_tensor(rng.random((H, W, C)).astype(np.float32))
    d_out = torch.as_tensor(rng.normal(size=(H, W, C)).astype(np.float32))
    _, _, _, pr = R.antialias_ref(color, rast.cpu(), pos, tri)
    amb_px = R.ambiguous_pixels(pr, H * W)
    d_out.reshape(-1, C)[amb_px] = 0
    out, gc, gp, _ = R.antialias_ref(color, rast.cpu(), pos, tri, d_out)
    return d, rast, color, d_out, out, gc, gp, amb_px


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", RESOLUTIONS)
@pytest.mark.parametrize("name", SCENES)
def test_antialias_f64(name, H, W):
    """out (pixels no ambiguous pair touches), grad_color and grad_pos within the rule for C in {1, 3, 4, 5}; the seeded entry equals
    the plain one within the atomic-sum bound; grad_pos scales with pos_gradient_boost, grad_color does not."""
    for C in (1, 3, 4, 5):
        d, rast, color, d_out, out, gc, gp, amb_px = _aa_case(name, H, W, C, seed=H * W + C)
        c_d, g_d = color.cuda(), d_out.cuda()
        R.check(d.antialias(c_d, rast).cpu().reshape(-1, C), out, f"antialias out C={C}", mask=~amb_px)
        gcol, gpos = d.antialias_backward(c_d, rast, g_d)
        R.check(gcol.cpu().reshape(-1, C), gc, f"antialias grad_color C={C}")
        R.check(gpos.cpu().reshape(-1, 1), gp, f"antialias grad_pos C={C}")
        assert bool((gpos[:, 2] == 0).all())
        gcol_s, gpos_s = d.antialias_backward(c_d, rast, g_d, seeded=True)
        _same_terms(gcol_s.cpu(), gcol.cpu(), gc, "seeded grad_color")
        _same_terms(gpos_s.cpu(), gpos.cpu(), gp, "seeded grad_pos")
        gcol3, gpos3 = d.antialias_backward(c_d, rast, g_d, boost=3.0)
        _same_terms(gcol3.cpu(), gcol.cpu(), gc, "grad_color at boost 3")
        gp3 = R.Scatter(gp.n, 1)
        gp3.abs, gp3.cnt = 3 * gp.abs, gp.cnt
        _same_terms(gpos3.cpu(), 3 * gpos.cpu().double(), gp3, "grad_pos at boost 3")


@pytest.mark.gpu
def test_fin_edge_antialias_is_order_independent():
    """Scene (d): antialias forward, grad_color and grad_pos do not change when the faces are permuted (ids remapped) or the edge table
    is rebuilt, and agree with the float64 reference, which applies the rule (an edge with more than two faces is a silhouette)."""
    H, W, C = 96, 128, 3
    d, rast, color, d_out, out, gc, gp, amb_px = _aa_case("fin", H, W, C, seed=17)
    pos, tri = scene("fin")
    c_d, g_d = color.cuda(), d_out.cuda()
    base_out = d.antialias(c_d, rast).cpu()
    base_gc, base_gp = (t.cpu() for t in d.antialias_backward(c_d, rast, g_d))
    R.check(base_out.reshape(-1, C), out, "fin antialias out", mask=~amb_px)
    R.check(base_gc.reshape(-1, C), gc, "fin grad_color")
    R.check(base_gp.reshape(-1, 1), gp, "fin grad_pos")
    for nm, perm in _fin_orders(len(tri)).items():
        tri_p = torch.as_tensor(tri[perm]).cuda().contiguous()
        rast_p = torch.as_tensor(_remap(rast.cpu().numpy(), perm)).cuda()
        for rebuild in range(2):
            table = d.raster.antialias_construct_topology_hash(tri_p)
            o = d.antialias(c_d, rast_p, table=table, tri=tri_p).cpu()
            g1, g2 = d.antialias_backward(c_d, rast_p, g_d, table=table, tri=tri_p)
            _same_terms(o, base_out, out, f"fin out, faces {nm}, table {rebuild}")
            _same_terms(g1.cpu(), base_gc, gc, f"fin grad_color, faces {nm}, table {rebuild}")
            _same_terms(g2.cpu(), base_gp, gp, f"fin grad_pos, faces {nm}, table {rebuild}")


# ------------------------------------------------------------------------------------------------ the stage-1 geometry chain

def _stage1_mesh(decimated):
    from nerf2mesh_amd import synthetic as S
    v, f = S.scene_mesh(20000)
    if decimated:
        from nerf2mesh_amd import mesh_simplify
        v, f, _ = mesh_simplify.decimate(v.cuda(), f.cuda(), 8000)
        v, f = v.cpu(), f.cpu()
    pose = S.make_cameras(4, seed=1)[2]
    mvp = S.mvp_matrix(pose, 512, 512, S.LEGO_FOCAL * 512 / S.LEGO_HW)
    return v.float(), f.int(), mvp.float()


@pytest.mark.gpu
@pytest.mark.parametrize("decimated", [False, True])
def test_stage1_chain_f64(decimated):
    """L(v) = sum W * antialias([interpolate(rgb), interpolate(1)], rasterize(to_clip(v, mvp))) -- the geometry path of render_stage1 with
    a fixed per-vertex colour -- at 512 x 512: dL/dv through the device chain (antialias backward, interpolate backward, rasterize
    backward, to_clip backward) against float64 autograd of the same chain with the device's ids held fixed."""
    from nerf2mesh_amd import _lib as L
    H = W = 512
    v, f, mvp = _stage1_mesh(decimated)
    V, F = v.shape[0], f.shape[0]
    rng = np.random.default_rng(23)
    rgb = torch.as_tensor(rng.random((V, 3)).astype(np.float32))
    attr4 = torch.cat([rgb, torch.ones(V, 1)], 1)
    s = L.stream()
    vd, md = v.cuda().contiguous(), mvp.cuda().contiguous()
    clip = torch.empty(V, 4, device="cuda")
    L.call("n2m_to_clip", vd.data_ptr(), md.data_ptr(), V, clip.data_ptr(), s)
    d = Dev(clip.cpu().numpy(), f.numpy())
    rast = d.rasterize(H, W)
    ids = rast[..., 3].long().cpu() - 1
    assert 0.05 < float((ids >= 0).float().mean()) < 0.9
    rgb_d, ones_d = rgb.cuda(), torch.ones(V, 1, device="cuda")
    color = torch.cat([d.interpolate(rgb_d, rast), d.interpolate(ones_d, rast)], -1).contiguous()
    # float64 chain with the device ids held fixed; pairs whose decision is ambiguous get no upstream weight
    clip64 = torch.cat([v.double(), torch.ones(V, 1, dtype=torch.float64)], 1) @ mvp.double().T
    pr = R.antialias_pairs(rast.cpu(), clip64.numpy(), f.numpy())
    Wt = torch.as_tensor(rng.normal(size=(H * W, 4)))
    Wt[R.ambiguous_pixels(pr, H * W)] = 0
    p = torch.nonzero(ids.reshape(-1) >= 0)[:, 0]
    vid = f.long()[ids.reshape(-1)[p]]
    keep = ~pr["amb_found"]
    P, O, d_ = pr["P"][keep], pr["O"][keep], pr["d"][keep]
    va, vb = pr["va"][keep], pr["vb"][keep]
    dst, src = torch.where(d_ < 0.5, P, O), torch.where(d_ < 0.5, O, P)
    Pxy = torch.stack([(P % W).double() + 0.5, (P // W).double() + 0.5], 1)
    Oxy = torch.stack([(O % W).double() + 0.5, (O // W).double() + 0.5], 1)

    def chain(vv, mm, at):
        cl = torch.cat([vv, torch.ones_like(vv[:, :1])], 1) @ mm.T
        fx, fy = R.pixel_ndc(p % W, p // W, H, W, vv.dtype)
        uv = R.uvz(cl[vid], fx, fy)[:, :2]
        b = torch.stack([uv[:, 0], uv[:, 1], 1 - uv[:, 0] - uv[:, 1]], 1)
        col = torch.zeros(H * W, 4, dtype=vv.dtype).index_add(0, p, (b[..., None] * at[vid]).sum(1))
        dd = R._pair_d(torch.stack([cl[va], cl[vb]], 1), Pxy.to(vv.dtype), Oxy.to(vv.dtype), W, H)
        out = col.index_add(0, dst, (0.5 - dd).abs()[:, None] * (col[src] - col[dst]))
        return (out * Wt.to(vv.dtype)).sum()
    [(g64, g32), _, _], _ = R.contributions(chain, [v.double(), mvp.double(), attr4.double()], torch.ones((), dtype=torch.float64), seed=7)
    # atomic terms per vertex: the rasterize-backward pixels and antialias pairs that reach it, mapped through the 4-term d_clip @ mvp
    Wimg = Wt.float().reshape(H, W, 4)
    aa_ref, gc, gp, _ = R.antialias_ref(color.cpu(), rast.cpu(), clip64.numpy(), f.numpy(), d_out=Wimg)
    _, _, gr = R.interpolate_ref(attr4, rast.cpu(), f.numpy(), gc.ref.reshape(H, W, 4))
    _, gpr = R.rasterize_fields(clip64.numpy(), f.numpy(), ids, H, W, d_rast=torch.cat([gr.ref, torch.zeros(H * W, 2, dtype=torch.float64)], 1).reshape(H, W, 4))
    absc = (gp.abs + gpr.abs).reshape(V, 4)
    cnt = (gp.cnt + gpr.cnt).reshape(V, 4).amax(1, keepdim=True) + 4
    M = mvp.double().abs()[:, :3]
    sc = R.Scatter(V * 3, 1)
    sc.ref = g64.reshape(-1, 1)
    sc.cond = (g32 - g64).abs().reshape(-1, 1)
    sc.abs = (absc @ M).reshape(-1, 1)
    sc.cnt = cnt.expand(V, 3).reshape(-1, 1).double()
    # the device chain
    Wd = Wimg.cuda().contiguous()
    gcol, gpos = d.antialias_backward(color, rast, Wd)
    _, gr_rgb = d.interpolate_backward(rgb_d, rast, gcol, stride=4, with_attr=False)
    _, gr_one = d.interpolate_backward(ones_d, rast, gcol, stride=4, offset=3, with_attr=False)
    d_rast = (gr_rgb + gr_one).contiguous()
    L.call("n2m_rasterize_backward", d.pos.data_ptr(), d.tri.data_ptr(), rast.data_ptr(), d_rast.data_ptr(), V, F, H, W, gpos.data_ptr(), s)
    dv = torch.empty(V, 3, device="cuda")
    L.call("n2m_to_clip_backward", gpos.data_ptr(), md.data_ptr(), V, dv.data_ptr(), s)
    assert float(g64.abs().max()) > 0
    R.check(dv.cpu().reshape(-1, 1), sc, f"stage-1 chain dL/dv ({'decimated' if decimated else 'box mesh'})")


# ------------------------------------------------------------------------------------------------ the nvdiffrast-style wrapper

def _merged(*scs):
    """The atomic-sum bound of terms from several Scatters summed into the same elements."""
    m = R.Scatter(scs[0].n, scs[0].k)
    for sc in scs:
        m.abs, m.cnt = m.abs + sc.abs, m.cnt + sc.cnt
    return m


@pytest.mark.gpu
def test_wrapper_minibatch_two_equals_two_single_calls():
    """raster.py with B = 2 against two B = 1 calls.  rasterize and interpolate outputs bit for bit; antialias output and the gradients of
    each operator (taken one operator at a time, so that every gradient sums exact inputs) within the atomic-sum bound of the float64
    reference's terms; a broadcast attr (Ba = 1) accumulates grad_attr from both images; Ba not in {1, B} raises ValueError."""
    from nerf2mesh_amd import raster as dr
    pos0, tri = scene("welded")
    H, W, A = 96, 128, 3
    rng = np.random.default_rng(31)
    pos = torch.as_tensor(np.stack([pos0, pos0 * np.float32(1.02) + np.float32(0.01)])).cuda()
    T = torch.as_tensor(tri).cuda()
    attr = torch.as_tensor(rng.normal(size=(1, len(pos0), A)).astype(np.float32)).cuda()
    wr = torch.as_tensor(rng.normal(size=(2, H, W, 4)).astype(np.float32)).cuda()
    wo = torch.as_tensor(rng.normal(size=(2, H, W, A)).astype(np.float32)).cuda()
    wa = torch.as_tensor(rng.normal(size=(2, H, W, A)).astype(np.float32)).cuda()
    ctx = dr.RasterizeGLContext(output_db=False)
    rast0, _ = dr.rasterize(ctx, pos, T, (H, W))
    for b in range(2):                                          # no upstream weight on pairs whose decision float32 may flip
        pr = R.antialias_pairs(rast0[b].cpu(), pos[b].cpu().numpy(), tri)
        wa[b].reshape(-1, A)[R.ambiguous_pixels(pr, H * W).cuda()] = 0

    def run(P, At, Wr, Wo, Wa):
        P1 = P.clone().requires_grad_(True)
        rast, _ = dr.rasterize(ctx, P1, T, (H, W))
        (rast * Wr).sum().backward()
        rast = rast.detach()
        A1 = At.clone().requires_grad_(True)
        out, _ = dr.interpolate(A1, rast, T)
        (out * Wo).sum().backward()
        out = out.detach()
        C1, P2 = out.clone().requires_grad_(True), P.clone().requires_grad_(True)
        aa = dr.antialias(C1, rast, P2, T)
        (aa * Wa).sum().backward()
        return dict(rast=rast, out=out, aa=aa.detach(), gp_r=P1.grad, ga=A1.grad, gc=C1.grad, gp_a=P2.grad)
    both = run(pos, attr, wr, wo, wa)
    one = [run(pos[b:b + 1], attr, wr[b:b + 1], wo[b:b + 1], wa[b:b + 1]) for b in range(2)]
    ga_terms = []
    for b in range(2):
        x, y = {k: v[b] for k, v in both.items() if k != "ga"}, {k: v[0] for k, v in one[b].items() if k != "ga"}
        assert torch.equal(x["rast"], y["rast"])
        assert torch.equal(x["out"], y["out"])
        pb, rast_c = pos[b].cpu().numpy(), y["rast"].cpu()
        ids = rast_c[..., 3].long() - 1
        _, gp_r = R.rasterize_fields(pb, tri, ids, H, W, d_rast=wr[b].cpu())
        _same_terms(x["gp_r"].cpu(), y["gp_r"].cpu(), gp_r, f"rasterize grad_pos, image {b}")
        _, ga, _ = R.interpolate_ref(attr[0].cpu(), rast_c, tri, wo[b].cpu())
        ga_terms.append(ga)
        aa, gc, gp_a, pr = R.antialias_ref(y["out"].cpu(), rast_c, pb, tri, d_out=wa[b].cpu())
        amb = R.ambiguous_pixels(pr, H * W)
        _same_terms(x["aa"].cpu(), y["aa"].cpu(), aa, f"antialias out, image {b}", mask=~amb)
        _same_terms(x["gc"].cpu(), y["gc"].cpu(), gc, f"antialias grad_color, image {b}")
        _same_terms(x["gp_a"].cpu(), y["gp_a"].cpu(), gp_a, f"antialias grad_pos, image {b}")
        assert float(y["gp_a"].abs().sum()) > 0 and float(y["gp_r"].abs().sum()) > 0
    ga_sum = one[0]["ga"] + one[1]["ga"]
    _same_terms(both["ga"].cpu(), ga_sum.cpu(), _merged(*ga_terms), "broadcast grad_attr")
    assert float((both["ga"] - one[0]["ga"]).abs().max()) > 0                  # the second image's share is there
    with pytest.raises(ValueError):
        dr.interpolate(attr.expand(3, -1, -1).contiguous(), both["rast"], T)
