"""Mesh cleaning on the device (include/n2m_hip.h, csrc/meshclean.hip): what the reference does with pymeshlab in `clean_mesh`
(meshutils.py:146-188; nerf/renderer.py:537 for the inner mesh, :653 for the outer cascades).

The per-element work (grid cells, the vertex-merge rounds, face re-pointing, duplicate / null flags, union-find components and their
statistics, the non-manifold-edge rounds, the fan walk and split) is HIP; sorting keys, unique-ing edges and the CSR offsets are torch
plumbing, as in mesh_simplify.py.  The rule, and why it does not depend on thread timing: DESIGN.md section 4.12.
tests/mesh_clean_ref.py restates it sequentially in numpy.
"""
import math

import torch

from . import _lib as L
from .mesh_simplify import _compact, _edges, _offsets

_p = L.ptr

CELL_MARGIN = 1.0 + 2.0 ** -10   # merge grid: cells a little larger than r, so the cell rounding cannot lose a pair
MAX_CELLS = 1 << 24              # merge grid: the cell edge doubles until the dense cell offsets stay below this
STAT_KEYS = ("unreferenced", "merged", "degenerate", "duplicate", "null", "components", "diameter_components", "diameter_faces",
             "size_components", "size_faces", "nonmanifold_faces", "split_vertices", "merge_rounds", "nonmanifold_rounds")


def _check_input(name, vertices, triangles):
    """mesh_simplify._check_mesh without the distinct-corner check: a cleaner takes raw input (such faces leave in step 2 or 4)."""
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


def box_diagonal(lo, hi):
    """Diagonal of the box [lo, hi] (fp32 corners as Python floats): sqrt((dx*dx + dy*dy) + dz*dz) in fp64."""
    dx, dy, dz = (float(h) - float(l) for l, h in zip(lo, hi))
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def merge_grid(lo, hi, r):
    """(cell edge, [nx, ny, nz]) of the merge grid: the edge starts at r * CELL_MARGIN and doubles while the grid has > MAX_CELLS cells."""
    h = r * CELL_MARGIN
    ext = [float(b) - float(a) for a, b in zip(lo, hi)]
    while True:
        n = [int(math.floor(e / h)) + 1 for e in ext]
        if n[0] * n[1] * n[2] <= MAX_CELLS:
            return h, n
        h *= 2.0


def _bbox(v, live=None):
    """(lo, hi) as Python floats (one host read); live: optional bool [V] -- the box of those rows only."""
    if live is not None:
        inf = torch.tensor(float("inf"), device=v.device)
        lo, hi = torch.where(live[:, None], v, inf).amin(0), torch.where(live[:, None], v, -inf).amax(0)
    else:
        lo, hi = v.amin(0), v.amax(0)
    vals = torch.cat([lo, hi]).tolist()
    return vals[:3], vals[3:]


def _keep(rows, keep):
    """Stable compaction of several row tensors by one uint8 mask -> (rows', removed count)."""
    n = int(keep.shape[0])
    scan = torch.cumsum(keep, 0, dtype=torch.int32)
    n_out = int(scan[-1]) if n else 0
    return [_compact(r, keep, scan, n_out) for r in rows], n - n_out


def _drop_unreferenced(v, f, s):
    V = int(v.shape[0])
    if V == 0:
        return v, f, 0
    ref = torch.empty(V, dtype=torch.uint8, device=v.device)
    L.call("n2m_mesh_mark_referenced", _p(f), int(f.shape[0]), V, _p(ref), s)
    vscan = torch.cumsum(ref, 0, dtype=torch.int32)
    n_v = int(vscan[-1])
    v = _compact(v, ref, vscan, n_v)
    f = f.contiguous()
    L.call("n2m_mesh_reindex", _p(f), f.numel(), _p(vscan), s)
    return v, f, V - n_v


def _merge(v, lo, hi, r, s, st):
    """Seeds of the greedy sweep -> dest [V] i32 (a seed's own id, else the id of the seed that claims it)."""
    dev = v.device
    V = int(v.shape[0])
    h, (nx, ny, nz) = merge_grid(lo, hi, r)
    keys = torch.empty(V, dtype=torch.int64, device=dev)
    L.call("n2m_mesh_clean_cell_keys", _p(v), V, float(lo[0]), float(lo[1]), float(lo[2]), h, nx, ny, nz, _p(keys), s)
    skeys, order = torch.sort(keys, stable=True)
    order = order.to(torch.int32).contiguous()
    cell_off = _offsets(skeys, nx * ny * nz)
    st_a = torch.full((V,), -1, dtype=torch.int32, device=dev)
    st_b = torch.empty_like(st_a)
    blocker = torch.full((V,), -1, dtype=torch.int32, device=dev)
    undecided = torch.empty(1, dtype=torch.int32, device=dev)
    r2 = r * r
    for rnd in range(V):                                     # the lowest undecided vertex decides in every round
        L.call("n2m_mesh_clean_merge_round", _p(v), V, _p(order), _p(keys), _p(cell_off), nx, ny, nz, r2, _p(st_a), _p(st_b), _p(blocker),
               _p(undecided), s)
        st_a, st_b = st_b, st_a
        if int(undecided.item()) == 0:                       # the round's one host read
            st["merge_rounds"] = rnd + 1
            return st_a
    raise RuntimeError("clean_mesh: the vertex merge did not converge")   # unreachable by the argument above


def clean_mesh(vertices, triangles, v_pct=1, min_f=8, min_d=5, repair=True, remesh=False, stats=None):
    """pymeshlab `clean_mesh` (meshutils.py:146-188) on the device, with its arguments and defaults.

    vertices float32 [V, 3], triangles int32/int64 [F, 3], CUDA; faces with a repeated corner are accepted.  In order:
    1. unreferenced vertices are dropped;  2. (v_pct > 0) every vertex closer than r = v_pct / 100 * the box diagonal to a seed of the
    greedy index-order sweep is merged into it, degenerate faces are dropped;  3. duplicate faces (same vertex set, either orientation) keep
    the lowest id;  4. faces of exactly zero fp64 area are dropped;  5. edge-connected components with a box diagonal below min_d / 100 *
    the mesh's (min_d > 0), then those with fewer than min_f faces (min_f > 0), are dropped;  6. (repair) faces on edges with > 2 faces
    are deleted in ascending (double area, id) order while one of their edges still has > 2 faces;  7. (repair) every vertex with more
    than one fan gets one new vertex, for the fan of its first (face, corner).  Unreferenced vertices are then dropped.

    Returns (v [V', 3] float32, f [F', 3] int32, face_src [F'] int64): surviving faces and input vertices keep their relative order,
    the step-7 vertices follow them, face_src is each face's index in the input.  remesh=True is not wired in here and raises
    NotImplementedError: the isotropic re-meshing itself is mesh_remesh.remesh_isotropic.
    stats: optional dict, filled with the counts of STAT_KEYS."""
    if remesh:
        raise NotImplementedError("clean_mesh: remesh=True (isotropic explicit re-meshing) is not wired into clean_mesh; call mesh_remesh.remesh_isotropic")
    if not (v_pct >= 0 and min_f >= 0 and min_d >= 0):
        raise ValueError(f"clean_mesh: v_pct, min_f and min_d must be >= 0, got {v_pct}, {min_f}, {min_d}")
    vertices, faces = _check_input("clean_mesh", vertices, triangles)
    dev = vertices.device
    st = dict.fromkeys(STAT_KEYS, 0)
    with torch.cuda.device(dev):
        s = L.stream()
        f = faces.clone()
        src = torch.arange(int(f.shape[0]), dtype=torch.int32, device=dev)
        totals = torch.empty(5, dtype=torch.int64, device=dev)
        # 1. unreferenced vertices
        v, f, st["unreferenced"] = _drop_unreferenced(vertices, f, s)
        V = int(v.shape[0])
        live = None                                          # vertices not merged away (the step-5 box); None: all of them
        # 2. merge close vertices
        if v_pct > 0 and V:
            lo, hi = _bbox(v)
            r = float(v_pct) / 100.0 * box_diagonal(lo, hi)
            if r * r > 0:
                dest = _merge(v, lo, hi, r, s, st)
                live = dest == torch.arange(V, dtype=torch.int32, device=dev)
                st["merged"] = V - int(live.sum())
                F = int(f.shape[0])
                alive = torch.empty(F, dtype=torch.uint8, device=dev)
                L.call("n2m_mesh_clean_repoint", _p(f), F, _p(dest), _p(alive), s)
                (f, src), st["degenerate"] = _keep([f, src], alive)
        # 3 + 4. duplicate faces, then null faces
        F = int(f.shape[0])
        if F:
            t = torch.sort(f, dim=1).values.long()
            o1 = torch.sort(t[:, 2], stable=True).indices
            o2 = torch.sort(t[o1, 0] * V + t[o1, 1], stable=True).indices
            order = o1[o2].to(torch.int32).contiguous()         # by sorted triple, ties in ascending face id
            alive = torch.empty(F, dtype=torch.uint8, device=dev)
            L.call("n2m_mesh_clean_dup_null", _p(v), _p(f), F, _p(order), _p(alive), _p(totals), s)
            st["duplicate"], st["null"] = (int(x) for x in totals[:2].tolist())
            (f, src), _ = _keep([f, src], alive)
        # 5. connected components: diameter, then face count
        F = int(f.shape[0])
        if F:
            min_diag = float(min_d) / 100.0 * box_diagonal(*_bbox(v, live)) if min_d > 0 else 0.0
            edges, _, c2e = _edges(f, V)
            E = int(edges.shape[0])
            ws = torch.empty(4 * E + 32 * F, dtype=torch.uint8, device=dev)
            label = torch.empty(F, dtype=torch.int32, device=dev)
            L.call("n2m_mesh_clean_components", _p(v), _p(f), F, _p(c2e), E, _p(ws), ws.numel(), _p(label), s)
            alive = torch.empty(F, dtype=torch.uint8, device=dev)
            L.call("n2m_mesh_clean_component_filter", F, _p(label), _p(ws), E, int(min_d > 0), min_diag, int(math.ceil(min_f)), _p(alive),
                   _p(totals), s)
            (st["components"], st["diameter_components"], st["diameter_faces"], st["size_components"],
             st["size_faces"]) = (int(x) for x in totals.tolist())
            (f, src), _ = _keep([f, src], alive)
        # 6. non-manifold edges
        F = int(f.shape[0])
        if repair and F:
            edges, nf, c2e = _edges(f, V)
            da = torch.empty(F, dtype=torch.float64, device=dev)
            state = torch.empty(F, dtype=torch.uint8, device=dev)
            L.call("n2m_mesh_clean_nm_edge_init", _p(v), _p(f), F, _p(c2e), _p(nf), _p(da), _p(state), _p(totals), s)
            n_cand = int(totals[0])
            if n_cand:
                ekeys, eorder = torch.sort(c2e.reshape(-1).long(), stable=True)
                ef_faces = (eorder // 3).to(torch.int32).contiguous()
                ef_off = _offsets(ekeys, int(edges.shape[0]))
                other = torch.empty_like(state)
                for rnd in range(n_cand):                    # the smallest undecided candidate decides in every round
                    L.call("n2m_mesh_clean_nm_edge_round", F, _p(c2e), _p(nf), _p(ef_off), _p(ef_faces), _p(da), _p(state), _p(other),
                           _p(totals), s)
                    state, other = other, state
                    und, deleted = (int(x) for x in totals[:2].tolist())   # the round's one host read
                    st["nonmanifold_faces"] += deleted
                    if und == 0:
                        st["nonmanifold_rounds"] = rnd + 1
                        break
                (f, src), _ = _keep([f, src], (state != 2).to(torch.uint8))
        # 7. non-manifold vertices
        F = int(f.shape[0])
        if repair and F:
            ckeys, corder = torch.sort(f.reshape(-1).long(), stable=True)
            vf_corner = corder.to(torch.int32).contiguous()
            vf_off = _offsets(ckeys, V)
            visited = torch.empty(3 * F, dtype=torch.uint8, device=dev)
            stack = torch.empty(3 * F, dtype=torch.int32, device=dev)
            split = torch.empty(V, dtype=torch.uint8, device=dev)
            first = torch.empty(V, dtype=torch.int32, device=dev)
            L.call("n2m_mesh_clean_fan_walk", _p(f), F, V, _p(vf_off), _p(vf_corner), _p(visited), _p(stack), _p(split), _p(first), _p(totals), s)
            n_split = int(totals[0])
            st["split_vertices"] = n_split
            if n_split:
                if V + n_split >= 1 << 31:
                    raise RuntimeError("clean_mesh: the vertex count exceeds 31-bit ids")
                # split vertices in the order of their first corner (unique per vertex); the others sort after them (INT32_MAX)
                key = torch.where(split != 0, first, torch.full_like(first, torch.iinfo(torch.int32).max))
                split_ids = torch.sort(key).indices[:n_split].to(torch.int32).contiguous()
                v = torch.cat([v, torch.empty(n_split, 3, dtype=torch.float32, device=dev)]).contiguous()
                L.call("n2m_mesh_clean_fan_split", _p(v), V, _p(f), _p(vf_off), _p(vf_corner), _p(visited), _p(split_ids), n_split, s)
                V += n_split
        # drop unreferenced vertices, stably
        v, f, _ = _drop_unreferenced(v, f, s)
    if stats is not None:
        stats.update(st)
    return v, f, src.long()
