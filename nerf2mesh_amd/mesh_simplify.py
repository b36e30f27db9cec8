"""Mesh decimation and midpoint subdivision on the device (include/n2m_hip.h, csrc/meshsimplify.hip): what the reference does with
pymeshlab on the host (`meshing_decimation_quadric_edge_collapse`, `meshing_surface_subdivision_midpoint`; meshutils.py:191-231,
nerf/renderer.py:209-294, :540-541, :582-583, :658-659).

The per-element work (quadrics, edge costs and placement, validity, independent-set selection, collapse, subdivision emission,
compaction) is HIP; sorting and unique-ing edge keys and the CSR offsets are torch plumbing, as in UniformLaplacian (trainer.py).
The rule, and why it does not depend on thread timing: DESIGN.md section 4.11.  tests/mesh_simplify_ref.py restates it in numpy.
"""
import torch

from . import _lib as L

_p = L.ptr

BOUNDARY_WEIGHT = 1.0     # boundary constraint plane of edge e: weight BOUNDARY_WEIGHT * |e|^2 (a face's plane: its area)
MAX_ROUNDS = 512


def _check_mesh(name, vertices, triangles):
    if not (torch.is_tensor(vertices) and vertices.is_cuda and torch.is_tensor(triangles) and triangles.is_cuda):
        raise RuntimeError(f"{name}: vertices and triangles must be CUDA tensors (the mesh passes run on the device; there is no host path)")
    if vertices.device != triangles.device:
        raise RuntimeError(f"{name}: vertices and triangles must be on the same device")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise ValueError(f"{name}: vertices must be float32 [V, 3], got {vertices.dtype} {tuple(vertices.shape)}")
    if triangles.dim() != 2 or triangles.shape[1] != 3 or triangles.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name}: triangles must be int32 or int64 [F, 3], got {triangles.dtype} {tuple(triangles.shape)}")
    V, F = int(vertices.shape[0]), int(triangles.shape[0])
    if V >= 1 << 31 or 3 * F >= 1 << 31:          # V < 2^31 also keeps the edge key min * V + max below 2^62
        raise ValueError(f"{name}: {V} vertices / {F} faces exceed the 31-bit ids")
    if F:
        lo, hi = (int(x) for x in torch.stack([triangles.min(), triangles.max()]).tolist())
        if lo < 0 or hi >= V:
            raise ValueError(f"{name}: triangle indices must lie in [0, {V}), got [{lo}, {hi}]")
        t = triangles
        if bool(((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 2] == t[:, 0])).any()):
            raise ValueError(f"{name}: every triangle needs three distinct vertices")
    return vertices.detach().contiguous(), triangles.detach().to(torch.int32).contiguous()


def _check_mask(name, mask, F, dev):
    if mask is None:
        return None
    if not (torch.is_tensor(mask) and mask.is_cuda and mask.device == dev):
        raise RuntimeError(f"{name}: the face selection must be a CUDA tensor on the mesh's device")
    if mask.shape != (F,) or mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{name}: the face selection must be bool or uint8 [F], got {mask.dtype} {tuple(mask.shape)}")
    return (mask != 0).to(torch.uint8).contiguous()


def _edges(faces, V):
    """edges [E, 2] i32 (a < b, ascending), edge_nf [E] i32, c2e [F, 3] i32 (corner k -> the edge (v_k, v_k+1))."""
    f = faces.long()
    a, b = f, f.roll(-1, dims=1)
    key = (torch.minimum(a, b) * V + torch.maximum(a, b)).reshape(-1)
    uk, inv, cnt = torch.unique(key, sorted=True, return_inverse=True, return_counts=True)
    edges = torch.stack([uk // V, uk % V], 1).to(torch.int32).contiguous()
    return edges, cnt.to(torch.int32).contiguous(), inv.view(-1, 3).to(torch.int32).contiguous()


def _offsets(sorted_keys, V, scale=1):
    """CSR offsets [V + 1] of keys sorted ascending whose row is key // scale: a search, no host read (bincount would read back)."""
    bounds = torch.arange(V + 1, device=sorted_keys.device, dtype=torch.int64) * scale
    return torch.searchsorted(sorted_keys, bounds).to(torch.int32).contiguous()


def _topology(faces, V):
    """Edges plus the CSRs: vertex -> faces (ascending face id), vertex -> edges (ascending other endpoint)."""
    edges, nf, c2e = _edges(faces, V)
    cv = faces.reshape(-1).long()
    keys, order = torch.sort(cv, stable=True)
    vf_faces = (order // 3).to(torch.int32).contiguous()
    vf_off = _offsets(keys, V)
    E = edges.shape[0]
    el = edges.long()
    ends, other = torch.cat([el[:, 0], el[:, 1]]), torch.cat([el[:, 1], el[:, 0]])
    eid = torch.arange(E, device=faces.device, dtype=torch.int32).repeat(2)
    keys, order = torch.sort(ends * V + other)
    ve_edges = eid[order].contiguous()
    ve_off = _offsets(keys, V, V)
    return edges, nf, c2e, vf_off, vf_faces, ve_off, ve_edges


def _compact(src, keep, scan, n_out):
    """Rows of src with keep, in order (n_out rows are allocated for the sum of keep; src rows bound the writes)."""
    n = src.shape[0]
    width = src[0].numel() if n else 1
    dst = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    L.call("n2m_mesh_compact_rows", _p(src), n, width, src.element_size(), _p(keep), _p(scan), _p(dst), L.stream())
    return dst[:n_out]


def decimate(vertices, triangles, target, optimal_placement=True, selected=None, stats=None):
    """Quadric edge-collapse decimation (Garland-Heckbert) in parallel rounds of independent collapses.

    vertices float32 [V, 3], triangles int32/int64 [F, 3], CUDA.  Returns (v [V', 3] float32, f [F', 3] int32, face_src [F'] int64): the
    decimated mesh with unreferenced vertices dropped, and for every surviving face the index of its source face (surviving faces keep
    their relative order).  The faces are reduced to `target` (or one below it: an interior collapse removes two), unless the mesh runs out
    of valid collapses first.  `optimal_placement=False` places the surviving vertex at the cheapest of {a, b, midpoint} only (the
    reference's setting for the outer cascades).

    selected: optional bool/uint8 [F] face mask.  A vertex may move only if all of its faces are selected, so unselected faces and their
    vertices are never touched; `target` then counts the selected faces (MeshLab's selected-only target).

    Edges with more than two faces freeze their endpoints: they are kept, not repaired.  A collapse is refused when it breaks the link
    condition or flips or degenerates a face, so a manifold input stays manifold and the reference's
    `meshing_repair_non_manifold_*` calls after the decimation are not needed for manifold inputs.

    stats: optional dict, filled with {"rounds": n, "faces": [count after each round]}."""
    vertices, faces = _check_mesh("decimate", vertices, triangles)
    dev = vertices.device
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    sel = _check_mask("decimate", selected, F, dev)
    target = int(target)
    if target < 0:
        raise ValueError("decimate: target must be >= 0")
    with torch.cuda.device(dev):
        n_count = F if sel is None else int(sel.sum())
        if stats is not None:
            stats.update(rounds=0, faces=[])
        if target >= n_count or F == 0:
            return vertices.clone(), faces.clone(), torch.arange(F, dtype=torch.int64, device=dev)
        s = L.stream()
        v = vertices.clone()
        f = faces.clone()
        src = torch.arange(F, dtype=torch.int32, device=dev)
        edges, nf, c2e, vf_off, vf_faces, ve_off, ve_edges = _topology(f, V)
        Q = torch.empty(V, 10, dtype=torch.float64, device=dev)
        L.call("n2m_mesh_quadrics", _p(v), V, _p(f), _p(c2e), _p(nf), _p(vf_off), _p(vf_faces), BOUNDARY_WEIGHT, _p(Q), s)
        flags = torch.empty(V, dtype=torch.int32, device=dev)
        dest = torch.empty(V, dtype=torch.int32, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        ws = torch.empty(2 * V, dtype=torch.int64, device=dev)
        for r in range(MAX_ROUNDS):
            if r:
                edges, nf, c2e, vf_off, vf_faces, ve_off, ve_edges = _topology(f, V)
            F, E = int(f.shape[0]), int(edges.shape[0])
            L.call("n2m_mesh_vertex_flags", _p(f), F, _p(c2e), _p(nf), _p(sel), V, _p(flags), s)
            keys = torch.empty(E, dtype=torch.int64, device=dev)
            place = torch.empty(E, 3, dtype=torch.float32, device=dev)
            L.call("n2m_mesh_edge_collapse_cost", _p(v), _p(f), _p(edges), _p(nf), E, _p(flags), _p(Q), _p(vf_off), _p(vf_faces), _p(ve_off),
                   _p(ve_edges), int(bool(optimal_placement)), _p(keys), _p(place), s)
            pick = torch.empty(E, dtype=torch.uint8, device=dev)
            L.call("n2m_mesh_select_collapses", _p(edges), _p(nf), E, _p(keys), _p(ve_off), _p(ve_edges), V, _p(ws), ws.numel() * 8, _p(pick),
                   _p(totals), s)
            n_sel, removed = (int(x) for x in totals.tolist())       # the round's one host read
            if n_sel == 0:
                break
            budget = n_count - target
            if removed > budget:
                # last round: the cheapest selected edges (by key) while the faces removed before each one are still below the budget.
                # Selected keys are below 2^63, so the signed order is the unsigned one; unselected edges sort last.
                on = pick.bool()
                order = torch.argsort(torch.where(on, keys, torch.full_like(keys, torch.iinfo(torch.int64).max)))
                rem = nf[order].long() * on[order]
                keep = on[order] & ((torch.cumsum(rem, 0) - rem) < budget)
                pick.scatter_(0, order, keep.to(torch.uint8))
                removed = int((rem * keep).sum())                  # the last round's second host read
            alive = torch.empty(F, dtype=torch.uint8, device=dev)
            L.call("n2m_mesh_collapse_apply", _p(edges), E, _p(pick), _p(place), _p(v), _p(Q), V, _p(f), F, _p(dest), _p(alive), s)
            scan = torch.cumsum(alive, 0, dtype=torch.int32)
            n_out = F - removed
            f = _compact(f, alive, scan, n_out)
            src = _compact(src, alive, scan, n_out)
            if sel is not None:
                sel = _compact(sel, alive, scan, n_out)
            n_count -= removed
            if stats is not None:
                stats["rounds"] = r + 1
                stats["faces"].append(int(f.shape[0]))
            if n_count <= target:
                break
        # drop unreferenced vertices, stably
        ref = torch.empty(V, dtype=torch.uint8, device=dev)
        L.call("n2m_mesh_mark_referenced", _p(f), int(f.shape[0]), V, _p(ref), s)
        vscan = torch.cumsum(ref, 0, dtype=torch.int32)
        n_v = int(vscan[-1])
        v_out = _compact(v, ref, vscan, n_v)
        f = f.contiguous()
        L.call("n2m_mesh_reindex", _p(f), f.numel(), _p(vscan), s)
    return v_out, f, src.long()


def subdivide_midpoint(vertices, triangles, threshold, selected=None, iterations=3):
    """Midpoint subdivision of the selected faces (pymeshlab `meshing_surface_subdivision_midpoint(threshold=..., selected=True)`, with
    its default of 3 iterations).  Every iteration splits each edge longer than `threshold` that belongs to a selected face at its
    midpoint, then re-triangulates every face (selected or not) by its split pattern, so the mesh stays conforming; children of
    selected faces stay selected.  selected: bool/uint8 [F] (None: every face).  Returns (v [V', 3] float32, f [F', 3] int32); the input
    vertices keep their ids, new vertices follow them in edge order."""
    vertices, faces = _check_mesh("subdivide_midpoint", vertices, triangles)
    dev = vertices.device
    F = int(faces.shape[0])
    sel = _check_mask("subdivide_midpoint", selected, F, dev)
    if sel is None:
        sel = torch.ones(F, dtype=torch.uint8, device=dev)
    if not float(threshold) > 0:
        raise ValueError("subdivide_midpoint: threshold must be > 0")
    thr2 = float(threshold) * float(threshold)
    v, f = vertices.clone(), faces.clone()
    with torch.cuda.device(dev):
        s = L.stream()
        for _ in range(int(iterations)):
            V, F = int(v.shape[0]), int(f.shape[0])
            if F == 0:
                break
            edges, _, c2e = _edges(f, V)
            E = int(edges.shape[0])
            split = torch.empty(E, dtype=torch.uint8, device=dev)
            L.call("n2m_mesh_subdiv_mark", _p(v), _p(f), F, _p(c2e), _p(sel), thr2, E, _p(split), s)
            sscan = torch.cumsum(split, 0, dtype=torch.int32)
            n_new = int(sscan[-1])
            if n_new == 0:
                break
            if V + n_new >= 1 << 31:                              # the next iteration's ids and edge keys (below 2^62)
                raise RuntimeError("subdivide_midpoint: the vertex count exceeds 31-bit ids")
            v2 = torch.cat([v, torch.empty(n_new, 3, dtype=torch.float32, device=dev)]).contiguous()
            L.call("n2m_mesh_subdiv_midpoints", _p(v2), V, _p(edges), E, _p(split), _p(sscan), s)
            counts = torch.empty(F, dtype=torch.int32, device=dev)
            L.call("n2m_mesh_subdiv_count", _p(c2e), F, _p(split), _p(counts), s)
            fscan = torch.cumsum(counts, 0, dtype=torch.int64)     # up to 4 F: summed in 64 bits, checked before it becomes i32
            n_f = int(fscan[-1])
            if 3 * n_f >= 1 << 31:
                raise RuntimeError(f"subdivide_midpoint: {n_f} faces exceed the 31-bit corner ids")
            fscan = fscan.to(torch.int32)
            f2 = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
            sel2 = torch.empty(n_f, dtype=torch.uint8, device=dev)
            L.call("n2m_mesh_subdiv_emit", _p(v2), V, _p(f), F, _p(c2e), _p(split), _p(sscan), _p(fscan), _p(sel), _p(f2), _p(sel2), s)
            v, f, sel = v2, f2, sel2
    return v, f
