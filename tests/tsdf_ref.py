"""Float64 numpy model of the TSDF integration rule, written from the comment on n2m_tsdf_integrate in include/n2m_hip.h (not from the
kernel), and the fixtures the TSDF tests share.

Per lattice point x = lo + index * (hi - lo) / (R - 1) and per view, views in order:
    p = R^T (x - c), zc = -p_z                       skip unless zc > min_depth
    col = fx p_x / zc + cx, row = cy - fy p_y / zc   skip unless 0 <= col < W and 0 <= row < H;  i = floor(col), j = floor(row)
    d = depth[v, j, i]                               skip unless d > 0 (0, negatives, NaN: no information; +inf is a depth)
    sdf = d - zc                                     skip if sdf < -trunc
    s = min(1, sdf / trunc);  tsdf = (tsdf w + s) / (w + 1);  w = min(w + 1, w_max)

Next to the result the model returns the NEAR-DECISION (point, view) pairs: the ones where fp32 rounding may take the other side of a
test, so that a correct fp32 implementation may differ there by more than rounding:
    |zc - min_depth| < 1e-4;  col or row within 1e-3 px of an integer (0, W and H are integers) while the pixel is within 1e-3 px of the
    image;  |sdf + trunc| < 1e-4 trunc;  d exactly at its skip boundary (d == 0)."""
import numpy as np

PX_EPS, Z_EPS, TRUNC_EPS = 1e-3, 1e-4, 1e-4


def look_at(centre, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """Camera-to-world [4,4] float64 of a camera at `centre` looking at `target`: it looks down its -z axis, y up (the engines' convention)."""
    c = np.asarray(centre, np.float64)
    z = c - np.asarray(target, np.float64)
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, c
    return P


def camera_rows(poses, intrinsics):
    """[n,16] float32: rotation row-major, centre, fx, fy, cx, cy -- the values the kernel is handed (the model reads them back as float64)."""
    poses = np.asarray(poses, np.float64)
    n = poses.shape[0]
    intr = np.broadcast_to(np.asarray(intrinsics, np.float64), (n, 4))
    return np.concatenate([poses[:, :3, :3].reshape(n, 9), poses[:, :3, 3], intr], axis=1).astype(np.float32)


def lattice(R, lo, hi):
    """[R0,R1,R2,3] float64: linspace(lo, hi, R) per axis, indexed [x,y,z]."""
    ax = [np.float64(lo[k]) + np.arange(R[k], dtype=np.float64) * (np.float64(hi[k]) - np.float64(lo[k])) / (R[k] - 1) for k in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)


def project(cam, X):
    """(zc, col, row) of the points X [...,3] in the camera `cam` [16], float64; col and row are NaN where zc == 0."""
    cam = np.asarray(cam, np.float64)
    Rm, c = cam[:9].reshape(3, 3), cam[9:12]
    fx, fy, cx, cy = cam[12:]
    p = (np.asarray(X, np.float64) - c) @ Rm                  # p = R^T (x - c)
    zc = -p[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        col = fx * p[..., 0] / zc + cx
        row = cy - fy * p[..., 1] / zc
    return zc, col, row


def integrate(tsdf, weight, lo, hi, cams, depth, trunc, min_depth, w_max):
    """The rule in float64.  tsdf, weight [R0,R1,R2] (any float type; not modified), cams [n,16], depth [n,H,W].  Returns
    (tsdf', weight', near [n,R0,R1,R2] bool, used [n,R0,R1,R2] bool): near = the near-decision pairs, used = the pairs that updated."""
    t, w = np.array(tsdf, np.float64), np.array(weight, np.float64)
    R = t.shape
    X = lattice(R, lo, hi)
    cams, depth = np.asarray(cams, np.float64), np.asarray(depth, np.float64)
    n, H, W = depth.shape
    trunc, min_depth, w_max = np.float64(trunc), np.float64(min_depth), np.float64(w_max)
    near, used = np.zeros((n,) + R, bool), np.zeros((n,) + R, bool)
    for v in range(n):
        zc, col, row = project(cams[v], X)
        front = zc > min_depth
        near_v = np.abs(zc - min_depth) < Z_EPS
        colf, rowf = np.where(front, col, -1.0), np.where(front, row, -1.0)
        inside = front & (colf >= 0) & (colf < W) & (rowf >= 0) & (rowf < H)
        around = front & (colf > -PX_EPS) & (colf < W + PX_EPS) & (rowf > -PX_EPS) & (rowf < H + PX_EPS)
        near_v |= around & ((np.abs(colf - np.round(colf)) < PX_EPS) | (np.abs(rowf - np.round(rowf)) < PX_EPS))
        i = np.clip(np.floor(colf), 0, W - 1).astype(np.int64)
        j = np.clip(np.floor(rowf), 0, H - 1).astype(np.int64)
        d = depth[v][j, i]
        near_v |= inside & (d == 0)
        with np.errstate(invalid="ignore"):
            valid = inside & (d > 0)
            sdf = np.where(valid, d, 1.0) - zc
            near_v |= valid & (np.abs(sdf + trunc) < TRUNC_EPS * trunc)
            upd = valid & ~(sdf < -trunc)
            s = np.minimum(1.0, sdf / trunc)
        t = np.where(upd, (t * w + np.where(upd, s, 0.0)) / (w + 1.0), t)
        w = np.where(upd, np.minimum(w + 1.0, w_max), w)
        near[v], used[v] = near_v, upd
    return t, w, near, used


# ------------------------------------------------------------------------------------------------ fixtures
def sphere_depth(pose, intr, H, W, radius):
    """(z-depth [H,W] float64 of the sphere |x| = radius through every pixel centre, hit [H,W] bool) for a camera outside or inside it: the
    first intersection in front of the camera, closed form.  The ray of pixel (j, i) is c + t R ((i + .5 - cx) / fx, -(j + .5 - cy) / fy, -1):
    |z| = 1, so t is the depth along the optical axis."""
    fx, fy, cx, cy = intr
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dirs = np.stack([(ii + 0.5 - cx) / fx, -(jj + 0.5 - cy) / fy, -np.ones_like(ii)], -1) @ pose[:3, :3].T
    o = pose[:3, 3]
    a, b, c = (dirs * dirs).sum(-1), 2.0 * (dirs @ o), o @ o - radius * radius
    disc = b * b - 4 * a * c
    hit = disc >= 0
    sq = np.sqrt(np.where(hit, disc, 0.0))
    t0, t1 = (-b - sq) / (2 * a), (-b + sq) / (2 * a)
    t = np.where(t0 > 0, t0, t1)
    hit &= t > 0
    return np.where(hit, t, 0.0), hit


R_SMALL, HW_SMALL = (9, 12, 17), (13, 19)
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
SMALL = dict(trunc=0.3, min_depth=0.05, w_max=3.0)


def small_fixture():
    """The kernel-against-model case: R = (9, 12, 17), maps of 13 x 19 pixels, four cameras at radius 3 and one at radius 0.3 inside the
    box, every view with intrinsics of its own (fx 11 .. 15, fy 8.5 .. 12.5).  The maps hold the radius-0.6 sphere's depth, +inf where a
    ray misses it, and a few pixels each of exact zeros, negatives and NaN.  Returns (cams [5,16] f32, depth [5,13,19] f32)."""
    H, W = HW_SMALL
    centres = [(2.7, 0.9, -0.95), (-1.5, 2.4, 1.0), (0.3, -2.0, 2.2), (-1.2, -1.6, -2.2), (0.18, -0.12, 0.2078)]      # the last: radius 0.3
    intr = np.array([[11.0 + v, 8.5 + v, W / 2 + 0.3 * v, H / 2 - 0.2 * v] for v in range(5)])
    poses = np.stack([look_at(c, target=(0.1 * k, -0.05 * k, 0.0)) for k, c in enumerate(centres)])
    depth = np.empty((5, H, W), np.float32)
    for v in range(5):
        z, hit = sphere_depth(poses[v], intr[v], H, W, 0.6)
        depth[v] = np.where(hit, z, np.inf)
    depth[0, 2, 3] = depth[1, 2, 12] = depth[4, 5, 5] = 0.0
    depth[0, 10, 15] = depth[2, 6, 10] = depth[4, 8, 12] = -1.5
    depth[1, 7, 8] = depth[3, 6, 9] = depth[4, 6, 9] = np.nan
    return camera_rows(poses, intr), depth


R_SPHERE, HW_SPHERE, F_SPHERE, RADIUS = 32, 128, 150.0, 0.6


def sphere_fixture(blob=False):
    """The analytic sphere: radius 0.6, 8 cameras on the radius-3 sphere (the corners of a cube), maps of 128 x 128 at focal 150.  Returns
    (cams [8,16] f32, z [8,128,128] f32 the depth where a ray hits, hit [8,128,128] bool).  blob=True adds to view 0 a 12 x 12-pixel patch of
    depth 2.3 beside the sphere: a floater at radius ~0.9 that no other view confirms."""
    H = W = HW_SPHERE
    intr = (F_SPHERE, F_SPHERE, W / 2, H / 2)
    corners = [(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    poses = np.stack([look_at(np.array(c, np.float64) * 3.0 / np.sqrt(3.0)) for c in corners])
    z, hit = np.empty((8, H, W), np.float32), np.empty((8, H, W), bool)
    for v in range(8):
        z[v], hit[v] = sphere_depth(poses[v], intr, H, W, RADIUS)
    if blob:
        assert not hit[0, 58:70, 103:115].any()
        z[0, 58:70, 103:115], hit[0, 58:70, 103:115] = 2.3, True
    return camera_rows(poses, intr), z, hit


def zero_crossings(tsdf, weight, lo, hi):
    """Points [K,3] where the tsdf changes sign along a lattice edge whose two endpoints are observed (weight > 0), by linear interpolation."""
    X = lattice(tsdf.shape, lo, hi)
    out = []
    for ax in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[ax], b[ax] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        ta, tb = tsdf[a], tsdf[b]
        m = (weight[a] > 0) & (weight[b] > 0) & ((ta < 0) != (tb < 0))
        f = (ta[m] / (ta[m] - tb[m]))[:, None]
        out.append(X[a][m] * (1 - f) + X[b][m] * f)
    return np.concatenate(out, axis=0)
