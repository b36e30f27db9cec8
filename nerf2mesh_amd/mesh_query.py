"""Closest-point queries on a triangle mesh and the mesh-to-mesh distance built on them (include/n2m_hip.h, csrc/meshquery.hip).

`MeshIndex` is a linear bounding-volume hierarchy (Karras 2012) over the mesh's faces, built on the device; `MeshIndex.closest` returns, for
every query point, the lexicographic minimum of (squared distance, face id) over the faces and the closest point itself.  The rule does not
depend on the tree: the traversal only skips what cannot win, and returns what the exhaustive scan returns bit for bit (DESIGN.md section
4.15; tests/mesh_query_ref.py restates the scan in numpy).  Keys, boxes and the traversal are HIP; sorting the keys, sorting the queries
along their own Morton curve and the surface sampling are torch plumbing, as in mesh_simplify.py.
"""
import torch

from . import _lib as L

_p = L.ptr

SLACK = 2.0 ** -40            # of the squared box diagonal (absolute) and of the best squared distance (relative): DESIGN 4.15


def _check_mesh(name, vertices, triangles):
    """mesh_simplify._check_mesh, except that a face with a repeated vertex index is allowed (the index leaves it out)."""
    if not (torch.is_tensor(vertices) and vertices.is_cuda and torch.is_tensor(triangles) and triangles.is_cuda):
        raise RuntimeError(f"{name}: vertices and triangles must be CUDA tensors (the mesh passes run on the device; there is no host path)")
    if vertices.device != triangles.device:
        raise RuntimeError(f"{name}: vertices and triangles must be on the same device")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise ValueError(f"{name}: vertices must be float32 [V, 3], got {vertices.dtype} {tuple(vertices.shape)}")
    if triangles.dim() != 2 or triangles.shape[1] != 3 or triangles.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name}: triangles must be int32 or int64 [F, 3], got {triangles.dtype} {tuple(triangles.shape)}")
    V, F = int(vertices.shape[0]), int(triangles.shape[0])
    if V >= 1 << 31 or 3 * F >= 1 << 31:
        raise ValueError(f"{name}: {V} vertices / {F} faces exceed the 31-bit ids")
    if F:
        lo, hi = (int(x) for x in torch.stack([triangles.min(), triangles.max()]).tolist())
        if lo < 0 or hi >= V:
            raise ValueError(f"{name}: triangle indices must lie in [0, {V}), got [{lo}, {hi}]")
    return vertices.detach().contiguous(), triangles.detach().to(torch.int32).contiguous()


def _spread3(x):
    x = (x | (x << 16)) & 0xFF0000FF
    x = (x | (x << 8)) & 0x0F00F00F
    x = (x | (x << 4)) & 0xC30C30C3
    return (x | (x << 2)) & 0x49249249


class MeshIndex:
    """Spatial index of a triangle mesh for closest-point queries; built once, immutable.

    vertices float32 [V, 3], triangles int32/int64 [F, 3], CUDA.  A face with a repeated vertex index is left out.  Building reads the
    mesh's bounding box and the number of indexed faces back to the host (two reads)."""

    def __init__(self, vertices, triangles):
        self.vertices, self.faces = _check_mesh("MeshIndex", vertices, triangles)
        dev = self.device = self.vertices.device
        V, F = int(self.vertices.shape[0]), int(self.faces.shape[0])
        self.lo, self.scale, self.diag2 = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.0
        self.n = 0
        self.leaf_face = self.children = self.boxes = None
        if F == 0:
            return
        with torch.cuda.device(dev):
            s = L.stream()
            used = self.vertices[self.faces.reshape(-1).long()].double()
            box = torch.stack([used.amin(0), used.amax(0)]).tolist()      # host read: the box the Morton cells divide
            self.lo = tuple(box[0])
            ext = [h - l for l, h in zip(*box)]
            self.scale = tuple(1024.0 / e if e > 0.0 and e < float("inf") else 0.0 for e in ext)
            self.diag2 = ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2]
            keys = torch.empty(F, dtype=torch.int64, device=dev)
            L.call("n2m_mesh_bvh_morton", _p(self.vertices), _p(self.faces), F, *self.lo, *self.scale, _p(keys), s)
            keys, _ = torch.sort(keys)
            n = self.n = int((keys != torch.iinfo(torch.int64).max).sum())   # host read: the faces with three distinct indices
            if n == 0:
                return
            keys = keys[:n].contiguous()
            self.leaf_face = (keys & 0xFFFFFFFF).to(torch.int32).contiguous()
            self.children = torch.empty(max(n - 1, 1), 2, dtype=torch.int32, device=dev)
            parent = torch.empty(2 * n - 1, dtype=torch.int32, device=dev)
            self.boxes = torch.empty(2 * n - 1, 6, dtype=torch.float32, device=dev)
            counters = torch.empty(max(n - 1, 1), dtype=torch.int32, device=dev)
            L.call("n2m_mesh_bvh_hierarchy", _p(keys), n, _p(self.children), _p(parent), s)
            L.call("n2m_mesh_bvh_refit", _p(self.vertices), _p(self.faces), _p(self.leaf_face), n, _p(self.children), _p(parent), _p(self.boxes),
                   _p(counters), s)

    def _query_order(self, pts):
        """The queries sorted along their own Morton curve in the mesh's box, so that a wave's 64 queries walk the same nodes."""
        lo = torch.tensor(self.lo, dtype=torch.float64, device=pts.device)
        scale = torch.tensor(self.scale, dtype=torch.float64, device=pts.device)
        q = torch.nan_to_num((pts - lo) * scale, nan=0.0).clamp_(0.0, 1023.0).long()
        code = _spread3(q[:, 0]) | (_spread3(q[:, 1]) << 1) | (_spread3(q[:, 2]) << 2)
        return torch.sort(code).indices

    def closest(self, points, prune=True, sort_queries=True):
        """points float32 or float64 [N, 3], CUDA -> (d2 float64 [N], face int32 [N], point float64 [N, 3]).

        d2 is the squared distance (fp64) to the closest point of the closest face, face the lowest id among the faces at that
        distance, point that face's closest point, unrounded.  An empty index gives d2 = inf, face = -1, point = NaN.
        prune=False visits every face (the exhaustive device scan, slow); sort_queries=False launches the queries in their own order.
        Neither changes a result."""
        if not (torch.is_tensor(points) and points.is_cuda and points.device == self.device):
            raise RuntimeError("MeshIndex.closest: points must be a CUDA tensor on the mesh's device")
        if points.dim() != 2 or points.shape[1] != 3 or points.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"MeshIndex.closest: points must be float32 or float64 [N, 3], got {points.dtype} {tuple(points.shape)}")
        N = int(points.shape[0])
        if N >= 1 << 31:
            raise ValueError(f"MeshIndex.closest: {N} points exceed the 31-bit ids")
        dev = self.device
        pts = points.detach().double().contiguous()
        d2 = torch.empty(N, dtype=torch.float64, device=dev)
        face = torch.empty(N, dtype=torch.int32, device=dev)
        hit = torch.empty(N, 3, dtype=torch.float64, device=dev)
        if N == 0:
            return d2, face, hit
        with torch.cuda.device(dev):
            order = self._query_order(pts) if sort_queries and self.n > 1 else None
            src = pts if order is None else pts[order].contiguous()
            L.call("n2m_mesh_closest", _p(self.vertices), _p(self.faces), _p(self.leaf_face), self.n, _p(self.children), _p(self.boxes), _p(src), N,
                   1 if prune else 0, SLACK * self.diag2, SLACK, _p(d2), _p(face), _p(hit), L.stream())
            if order is not None:
                inv = torch.empty_like(order)
                inv[order] = torch.arange(N, device=dev)
                d2, face, hit = d2[inv], face[inv], hit[inv]
        return d2, face, hit


def sample_surface(vertices, triangles, n, generator=None):
    """n points on the surface, uniform by area: -> (points float64 [n, 3], face int64 [n]).  Faces are drawn from the cumulative fp64
    areas, the point inside a face by the square-root barycentric map.  generator: a torch.Generator on the mesh's device."""
    vertices, faces = _check_mesh("sample_surface", vertices, triangles)
    dev = vertices.device
    n = int(n)
    if n < 0:
        raise ValueError("sample_surface: n must be >= 0")
    if faces.shape[0] == 0:
        if n:
            raise ValueError("sample_surface: a mesh without faces has no surface to sample")
        return torch.empty(0, 3, dtype=torch.float64, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
    p = vertices.double()[faces.long()]
    a, b, c = p[:, 0], p[:, 1], p[:, 2]
    cum = torch.cumsum(torch.linalg.cross(b - a, c - a).norm(dim=1), 0)
    if not float(cum[-1]) > 0.0:
        raise ValueError("sample_surface: the mesh has no area")
    r = torch.rand(n, 3, dtype=torch.float64, device=dev, generator=generator)
    f = torch.searchsorted(cum, r[:, 0] * cum[-1], right=True).clamp_(max=faces.shape[0] - 1)
    s = torch.sqrt(r[:, 1])
    w0, w1, w2 = (1.0 - s)[:, None], (s * (1.0 - r[:, 2]))[:, None], (s * r[:, 2])[:, None]
    return w0 * a[f] + w1 * b[f] + w2 * c[f], f


def mesh_distance(va, fa, vb, fb, n=100000, generator=None):
    """Sampled distance between the meshes A = (va, fa) and B = (vb, fb): n area-weighted samples of each surface against the other mesh.

    -> {"mean_ab", "max_ab": mean and maximum distance of A's samples to B; "mean_ba", "max_ba": of B's samples to A;
        "chamfer": (mean_ab + mean_ba) / 2; "hausdorff": max(max_ab, max_ba) (floats);
        "samples_a", "samples_b": the samples, float64 [n, 3]; "d_ab", "d_ba": their distances, float64 [n]}."""
    if int(n) < 1:
        raise ValueError("mesh_distance: n must be >= 1")
    sa, _ = sample_surface(va, fa, n, generator)
    sb, _ = sample_surface(vb, fb, n, generator)
    d_ab = torch.sqrt(MeshIndex(vb, fb).closest(sa)[0])
    d_ba = torch.sqrt(MeshIndex(va, fa).closest(sb)[0])
    mean_ab, max_ab, mean_ba, max_ba = torch.stack([d_ab.mean(), d_ab.max(), d_ba.mean(), d_ba.max()]).tolist()
    return {"mean_ab": mean_ab, "max_ab": max_ab, "mean_ba": mean_ba, "max_ba": max_ba, "chamfer": 0.5 * (mean_ab + mean_ba),
            "hausdorff": max(max_ab, max_ba), "samples_a": sa, "samples_b": sb, "d_ab": d_ab, "d_ba": d_ba}
