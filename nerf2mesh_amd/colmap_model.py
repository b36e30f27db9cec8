"""COLMAP's binary model files (reader and writer) and the pose algebra the loaders of capture.py share.

Written from COLMAP's published format description (https://colmap.github.io/format.html, "Binary File Format"; the camera model ids and
their parameter counts are those of src/colmap/sensor/models.h), little endian throughout:
  cameras.bin   u64 count; per camera: i32 id, i32 model, u64 width, u64 height, f64 params[n(model)]
  images.bin    u64 count; per image: i32 id, f64 q[4] (w, x, y, z), f64 t[3], i32 camera id, name (zero-terminated), u64 n2d,
                n2d x (f64 x, f64 y, i64 point3D id or -1)
  points3D.bin  u64 count; per point: u64 id, f64 xyz[3], u8 rgb[3], f64 error, u64 track length, length x (i32 image id, i32 point2D idx)
"""
import math
import struct

import numpy as np

COLMAP_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8), 5: ("OPENCV_FISHEYE", 8),
                 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
COLMAP_DIRS = (("colmap_sparse", "0"), ("sparse", "0"), ("colmap",))
_POINT2D = np.dtype([("xy", "<f8", 2), ("id", "<i8")])


class _Reader:
    def __init__(self, name):
        with open(name, "rb") as f:
            self.buf, self.pos, self.name = f.read(), 0, name

    def take(self, fmt):
        n = struct.calcsize(fmt)
        if self.pos + n > len(self.buf):
            raise ValueError(f"{self.name}: truncated at byte {self.pos}")
        out = struct.unpack_from(fmt, self.buf, self.pos)
        self.pos += n
        return out

    def array(self, dtype, count):
        dt = np.dtype(dtype)
        if self.pos + dt.itemsize * count > len(self.buf):
            raise ValueError(f"{self.name}: truncated at byte {self.pos}")
        out = np.frombuffer(self.buf, dt, count, self.pos)
        self.pos += dt.itemsize * count
        return out

    def cstring(self):
        end = self.buf.find(b"\0", self.pos)
        if end < 0:
            raise ValueError(f"{self.name}: unterminated name at byte {self.pos}")
        out = self.buf[self.pos:end].decode()
        self.pos = end + 1
        return out


def read_colmap_cameras(name):
    """{camera id: dict(model, width, height, params [n] f64)}."""
    r = _Reader(name)
    cams = {}
    for _ in range(r.take("<Q")[0]):
        cid, model, w, h = r.take("<iiQQ")
        if model not in COLMAP_MODELS:
            raise ValueError(f"{name}: unknown camera model id {model}")
        mname, npar = COLMAP_MODELS[model]
        cams[cid] = dict(model=mname, width=int(w), height=int(h), params=r.array("<f8", npar).copy())
    return cams


def read_colmap_images(name):
    """{image id: dict(q [4] (w, x, y, z), t [3], camera_id, name, xys [n,2] f64, point3D_ids [n] i64)}."""
    r = _Reader(name)
    ims = {}
    for _ in range(r.take("<Q")[0]):
        iid = r.take("<i")[0]
        qt = r.array("<f8", 7).copy()
        cam = r.take("<i")[0]
        fname = r.cstring()
        p2d = r.array(_POINT2D, r.take("<Q")[0])
        ims[iid] = dict(q=qt[:4], t=qt[4:], camera_id=cam, name=fname, xys=p2d["xy"].copy().reshape(-1, 2), point3D_ids=p2d["id"].copy())
    return ims


def read_colmap_points(name):
    """(ids [M] i64 ascending, xyz [M,3] f64, error [M] f64)."""
    r = _Reader(name)
    ids, xyz, err = [], [], []
    for _ in range(r.take("<Q")[0]):
        pid, x, y, z, _r, _g, _b, e, track = r.take("<QdddBBBdQ")
        r.array("<i4", 2 * track)
        ids.append(pid); xyz.append((x, y, z)); err.append(e)
    order = np.argsort(np.asarray(ids, dtype=np.int64), kind="stable")
    return (np.asarray(ids, dtype=np.int64)[order], np.asarray(xyz, dtype=np.float64).reshape(-1, 3)[order],
            np.asarray(err, dtype=np.float64)[order])


def write_colmap_cameras(name, model_id, width, height, params):
    """cameras.bin: one camera of model `model_id` and size width x height per parameter vector of `params`, ids from 1."""
    with open(name, "wb") as f:
        f.write(struct.pack("<Q", len(params)))
        for n, p in enumerate(params):
            f.write(struct.pack("<iiQQ", n + 1, model_id, width, height))
            f.write(np.asarray(p, dtype="<f8").tobytes())


def write_colmap_images(name, qt, camera_ids, names, keypoints):
    """images.bin: image v + 1 with qt[v] [7] (q then t), its camera id, name and keypoints (xy [n,2], point3D id [n] or -1).  Returns the
    tracks {point3D id: [(image id, keypoint index)]} that write_colmap_points takes."""
    tracks = {}
    with open(name, "wb") as f:
        f.write(struct.pack("<Q", len(names)))
        for v, (xy, pid) in enumerate(keypoints):
            f.write(struct.pack("<i", v + 1))
            f.write(np.asarray(qt[v]).astype("<f8").tobytes())
            f.write(struct.pack("<i", camera_ids[v]))
            f.write(names[v].encode() + b"\0")
            rec = np.empty(len(pid), dtype=_POINT2D)
            rec["xy"], rec["id"] = xy, pid
            f.write(struct.pack("<Q", len(pid)))
            f.write(rec.tobytes())
            for j, p in enumerate(pid):
                if p != -1:
                    tracks.setdefault(int(p), []).append((v + 1, j))
    return tracks


def write_colmap_points(name, ids, xyz, errors, tracks):
    """points3D.bin: ids [M], xyz [M,3], errors [M], every point grey, with its track from write_colmap_images."""
    with open(name, "wb") as f:
        f.write(struct.pack("<Q", len(ids)))
        for m, pid in enumerate(ids):
            tr = tracks.get(int(pid), [])
            f.write(struct.pack("<QdddBBBdQ", int(pid), *xyz[m], 128, 128, 128, float(errors[m]), len(tr)))
            f.write(np.asarray(tr, dtype="<i4").tobytes())


def quat_to_rotmat(q):
    """Rotation matrix of a unit quaternion (w, x, y, z)."""
    w, x, y, z = (float(a) for a in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def rotmat_to_quat(R):
    """Unit quaternion (w, x, y, z), w >= 0, of a rotation matrix (the branch with the largest pivot)."""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        q = (0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s)
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = ((R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s)
    elif R[1, 1] > R[2, 2]:
        s = math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = ((R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s)
    else:
        s = math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = ((R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s)
    q = np.asarray(q, dtype=np.float64)
    q /= np.linalg.norm(q)
    return -q if q[0] < 0 else q


def decompose_projection(P):
    """P [3,4] = s K [R | -R C] (any scale s, either sign) -> K [3,3] upper triangular with a positive diagonal and K[2,2] = 1, R [3,3]
    world-to-camera with det R = +1, C [3] the camera centre; float64 throughout.  What nerf/dtu_provider.py:49-63 takes from
    cv2.decomposeProjectionMatrix, by an RQ decomposition of M = P[:,:3] (a QR factorisation of the row-reversed transpose); the signs are
    fixed afterwards: columns of K / rows of R flipped until K's diagonal is positive, and R negated when its determinant is -1 (that
    is P -> -P, the same camera).  C = -inv(M) P[:,3] does not depend on either."""
    P = np.asarray(P, dtype=np.float64)
    M = P[:3, :3]
    J = np.eye(3)[::-1]
    q, r = np.linalg.qr((J @ M).T)                 # J M = r^T q^T  ->  M = (J r^T J) (J q^T)
    K, R = J @ r.T @ J, J @ q.T
    S = np.diag(np.where(np.diag(K) < 0, -1.0, 1.0))
    K, R = K @ S, S @ R
    if np.linalg.det(R) < 0:
        R = -R
    C = -np.linalg.solve(M, P[:3, 3])
    return K / K[2, 2], R, C


def _rotation_between(a, b):
    """The rotation that takes direction a to direction b (Rodrigues; nerf/colmap_provider.py:18-27 `rotmat`, whose random retry for
    opposite directions is replaced by a fixed perpendicular axis)."""
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    v, c = np.cross(a, b), float(np.dot(a, b))
    if c < -1 + 1e-10:
        axis = np.cross(a, [1.0, 0.0, 0.0] if abs(a[0]) < 0.9 else [0.0, 1.0, 0.0])
        axis /= np.linalg.norm(axis)
        return 2 * np.outer(axis, axis) - np.eye(3)
    s = np.linalg.norm(v)
    k = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + k + k.dot(k) * ((1 - c) / (s ** 2 + 1e-10))


def center_poses(poses, pts3d, enable_cam_center=False):
    """nerf/colmap_provider.py:30-54: move the point centroid (or the camera centroid) to the origin and rotate the mean of the cameras'
    second axis onto +z.  poses [V,4,4], pts3d [M,3], float64; returns new arrays."""
    center = poses[:, :3, 3].mean(0) if enable_cam_center else pts3d.mean(0)
    up = poses[:, :3, 1].mean(0)
    R = np.eye(4)
    R[:3, :3] = _rotation_between(up / (np.linalg.norm(up) + 1e-10), np.array([0.0, 0.0, 1.0]))
    poses = poses.copy()
    poses[:, :3, 3] -= center
    return R @ poses, (pts3d - center) @ R[:3, :3].T


def _world_flip(poses, pts):
    """The convention change of nerf/colmap_provider.py:205-211, its own inverse on the world side: camera axes y, z negated (OpenCV ->
    OpenGL), world (x, y, z) -> (y, x, -z) for poses and points."""
    poses = poses.copy()
    poses[:, :3, 1:3] *= -1
    poses = poses[:, [1, 0, 2, 3], :]
    poses[:, 2] *= -1
    pts = pts[:, [1, 0, 2]].copy()
    pts[:, 2] *= -1
    return poses, pts
