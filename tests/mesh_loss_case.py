"""Shared by tests/test_mesh_losses.py (CPU) and tests/test_mesh_losses_gpu.py: the test meshes, a brute-force topology, the float64 yardstick
(the definitions of the normal-consistency and edge-length losses written out here, independently of nerf2mesh_amd.trainer.MeshEdgeTerms)
and the tolerance every float32 evaluation of them is held to."""
import functools
import itertools

import numpy as np
import torch

# The yardstick is the float64 evaluation of the definitions on the same float32 inputs.  Distances to it of the plain float32 torch form
# (MeshEdgeTerms on CPU tensors, its autograd gradient), measured on the CPU over every mesh and weight setting of cases():
#   value:    |value - yardstick|                                largest 1.3e-07 (triangle, weights (0.37, 2.5))
#   gradient: max |grad - grad_ref| / max |grad_ref| per mesh    largest 1.3e-05 (flat grid, weights (0.37, 2.5): the normal term's rounding noise
#             against the small gradient of the edge term; 3.7e-06 on the tetrahedron, at most 1.2e-06 on the noisy grids)
# A float32 evaluation -- the HIP kernels above all -- gets 8 x the largest such distance (1.04e-06 and 1.04e-04): the margin covers another
# summation order.
FP32_VALUE_DIST, FP32_GRAD_DIST = 1.3e-07, 1.3e-05
VALUE_BOUND, GRAD_BOUND = 8 * FP32_VALUE_DIST, 8 * FP32_GRAD_DIST

WEIGHTS = ((1.0, 0.0), (0.0, 1.0), (0.37, 2.5))        # (lambda_normal, lambda_edgelen): each loss alone, then both with non-unit weights
UPSTREAM = 3.5                                          # non-unit gradient flowing into the loss


def tetrahedron():
    v = [[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.3, 0.9, 0.1], [0.4, 0.3, 0.8]]
    return np.array(v, np.float32), np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)


def triangle():
    return np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.2], [0.2, 1.0, 0.0]], np.float32), np.array([[0, 1, 2]], np.int32)


def book():
    """Three faces on the edge (0, 1): a non-manifold edge, 3 pairs."""
    v = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 1.0, 0.0], [0.4, -0.2, 0.9], [0.6, -0.7, -0.5]]
    return np.array(v, np.float32), np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)


def grid(n=21, noise=0.0, seed=0):
    """n x n vertices on the unit square in the plane z = 0, every cell split into two triangles; `noise` is added to all three coordinates."""
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([x / (n - 1), y / (n - 1), np.zeros_like(x, dtype=np.float64)], -1).reshape(-1, 3)
    if noise:
        v = v + noise * np.random.default_rng(seed).standard_normal(v.shape)
    i = (y[:-1, :-1] * n + x[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([i, i + 1, i + n + 1], 1), np.stack([i, i + n + 1, i + n], 1)])
    return v.astype(np.float32), f.astype(np.int32)


def concat(*meshes):
    """Meshes concatenated with an index offset, as model.triangles holds the cascades' meshes."""
    vs, fs, o = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + o)
        o += v.shape[0]
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def zero_area():
    """Two faces on the edge (0, 1); the second face's opposite vertex lies ON the edge's line: a zero-area face, n1 = 0 exactly."""
    v = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 1.0, 0.25], [2.0, 0.0, 0.0]]
    return np.array(v, np.float32), np.array([[0, 1, 2], [1, 0, 3]], np.int32)


def cases():
    """name -> (verts, faces, weight settings).  The flat grid's normal term is 0 with a gradient of exactly 0 in exact arithmetic: alone it
    has no largest gradient to normalise by, so the flat grid runs with the two settings in which the edge term gives the gradient a scale
    (with both terms on it is the case that sets GRAD_BOUND)."""
    return {
        "tetrahedron": (*tetrahedron(), WEIGHTS),
        "triangle": (*triangle(), WEIGHTS),
        "book": (*book(), WEIGHTS),
        "grid": (*grid(), WEIGHTS[1:]),
        "grid noise 0.1": (*grid(noise=0.1, seed=1), WEIGHTS),
        "grid noise 0.01": (*grid(noise=0.01, seed=2), WEIGHTS),
        "grid noise 0.001": (*grid(noise=0.001, seed=3), WEIGHTS),
        "two cascades": (*concat(grid(noise=0.02, seed=4), grid(9, noise=0.05, seed=5)), WEIGHTS),
    }


def brute_topology(faces):
    """Plain Python: edges (sorted, v0 < v1) and the pair records (v0, v1, a, b) of every two faces on an edge, faces in ascending order."""
    on_edge = {}
    for fi, f in enumerate(np.asarray(faces).tolist()):
        for k in range(3):
            a, b, c = f[k], f[(k + 1) % 3], f[(k + 2) % 3]
            on_edge.setdefault((min(a, b), max(a, b)), []).append(c)
    edges = sorted(on_edge)
    pairs = [(v0, v1, a, b) for (v0, v1) in edges for a, b in itertools.combinations(on_edge[(v0, v1)], 2)]
    return np.array(edges, np.int64).reshape(-1, 2), np.array(pairs, np.int64).reshape(-1, 4)


def defined_losses(verts, edges, pairs):
    """(normal consistency, edge length) of `verts` (a torch tensor of any float dtype) by the definitions:
    c = n0 . n1 / (max(|n0|, 1e-8) max(|n1|, 1e-8)), mean of 1 - c over the pairs; mean of |v0 - v1|^2 over the edges; 0 where there is none."""
    zero = verts.sum() * 0
    normal = edge = zero
    if len(pairs):
        v0, v1, a, b = (verts[torch.as_tensor(pairs[:, k])] for k in range(4))
        e = v1 - v0
        n0 = torch.linalg.cross(e, a - v0)
        n1 = -torch.linalg.cross(e, b - v0)
        eps = torch.full((), 1e-8, dtype=verts.dtype)
        c = (n0 * n1).sum(-1) / (torch.maximum(n0.norm(dim=-1), eps) * torch.maximum(n1.norm(dim=-1), eps))
        normal = (1 - c).mean()
    if len(edges):
        d = verts[torch.as_tensor(edges[:, 0])] - verts[torch.as_tensor(edges[:, 1])]
        edge = (d * d).sum(-1).mean()
    return normal, edge


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """{weights: (value, gradient [V, 3])} in float64 of the case's float32 vertices, computed once per process; the gradient carries UPSTREAM."""
    v, f, settings = cases()[name]
    edges, pairs = brute_topology(f)
    out = {}
    for lam_n, lam_e in settings:
        x = torch.from_numpy(v).double().requires_grad_()
        n, e = defined_losses(x, edges, pairs)
        val = lam_n * n + lam_e * e
        (val * UPSTREAM).backward()
        out[(lam_n, lam_e)] = (float(val.detach()), x.grad.clone())
    return out


def distances(name, weights, value, grad):
    """(|value - yardstick|, max |grad - grad_ref| / max |grad_ref|) of one float32 evaluation; a gradient that is exactly 0 in the yardstick (no
    term at all) must be exactly 0."""
    ref_val, ref_grad = yardstick(name)[weights]
    dv = abs(float(value) - ref_val)
    scale = float(ref_grad.abs().max())
    err = float((grad.detach().cpu().double() - ref_grad).abs().max())
    return dv, (err / scale if scale > 0 else (0.0 if err == 0 else float("inf")))
