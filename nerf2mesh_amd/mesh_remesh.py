"""Isotropic explicit re-meshing on the device (include/n2m_hip.h, csrc/meshremesh.hip): what the reference does with pymeshlab on the
host (`meshing_isotropic_explicit_remeshing(iterations=3, targetlen=PureValue(refine_remesh_size), selectedonly=True)`,
meshutils.py:208-209) between the selected decimation and the selected subdivision of the stage-1 refinement.

Botsch & Kobbelt's loop -- split the long edges, collapse the short ones, flip towards regular valence, relax tangentially -- as the
project's own deterministic rule: DESIGN.md section 4.14.  It does not reproduce MeshLab's vertex positions or counts.  The per-element
work is HIP (csrc/meshremesh.hip, and the selection / collapse / compaction / subdivision entry points of csrc/meshsimplify.hip, unchanged);
sorting and unique-ing edge keys and the CSR offsets are torch plumbing, as in mesh_simplify.py.  tests/mesh_remesh_ref.py restates the rule in
numpy, bit for bit.
"""
import math

import torch

from . import _lib as L
from .mesh_query import MeshIndex
from .mesh_simplify import _check_mask, _check_mesh, _compact, _edges, _offsets, _topology

_p = L.ptr

MAX_SPLIT_ROUNDS = 32
MAX_COLLAPSE_ROUNDS = 128
MAX_FLIP_ROUNDS = 128


def _edge_corners(c2e, E):
    """Corner ids 3 f + k sorted (stably) by the edge the corner owns, and the offsets [E + 1] of every edge's run."""
    keys, order = torch.sort(c2e.reshape(-1).long(), stable=True)
    return _offsets(keys, E), order.to(torch.int32).contiguous()


class _Topo:
    """Edges, CSRs and the vertex / edge classes of the current mesh (rebuilt whenever the connectivity changed)."""

    def __init__(self, v, f, sel, cos_f):
        dev = v.device
        V, F = int(v.shape[0]), int(f.shape[0])
        s = L.stream()
        self.edges, self.nf, self.c2e, self.vf_off, self.vf_faces, self.ve_off, self.ve_edges = _topology(f, V)
        E = self.E = int(self.edges.shape[0])
        self.eoff, self.ecorn = _edge_corners(self.c2e, E)
        flags = torch.empty(V, dtype=torch.int32, device=dev)
        L.call("n2m_mesh_vertex_flags", _p(f), F, _p(self.c2e), _p(self.nf), _p(sel), V, _p(flags), s)
        self.efeat = torch.empty(E, dtype=torch.uint8, device=dev)
        self.vclass = torch.empty(V, dtype=torch.int32, device=dev)
        L.call("n2m_mesh_remesh_classify", _p(v), V, _p(f), _p(self.edges), E, _p(self.eoff), _p(self.ecorn), _p(self.ve_off), _p(self.ve_edges),
               _p(flags), cos_f, _p(self.efeat), _p(self.vclass), s)

    def valence_dev(self):
        """Sum over the vertices of (valence - target)^2, target 6, 4 on a boundary, 0-valence vertices left out: a device scalar."""
        val = (self.ve_off[1:] - self.ve_off[:-1]).long()
        d = val - torch.where((self.vclass & 2) != 0, 4, 6)
        return torch.where(val > 0, d * d, torch.zeros_like(d)).sum()


def _split_pass(v, f, sel, src, hi2):
    dev = v.device
    s = L.stream()
    for r in range(MAX_SPLIT_ROUNDS):
        V, F = int(v.shape[0]), int(f.shape[0])
        edges, _, c2e = _edges(f, V)
        E = int(edges.shape[0])
        split = torch.empty(E, dtype=torch.uint8, device=dev)
        L.call("n2m_mesh_remesh_split_mark", _p(v), _p(edges), E, F, _p(c2e), _p(sel), hi2, _p(split), s)
        sscan = torch.cumsum(split, 0, dtype=torch.int32)
        n_new = int(sscan[-1])
        if n_new == 0:
            return v, f, sel, src, r
        if V + n_new >= 1 << 31:
            raise RuntimeError("remesh_isotropic: the vertex count exceeds 31-bit ids")
        v2 = torch.cat([v, torch.empty(n_new, 3, dtype=torch.float32, device=dev)]).contiguous()
        L.call("n2m_mesh_subdiv_midpoints", _p(v2), V, _p(edges), E, _p(split), _p(sscan), s)
        counts = torch.empty(F, dtype=torch.int32, device=dev)
        L.call("n2m_mesh_subdiv_count", _p(c2e), F, _p(split), _p(counts), s)
        fscan = torch.cumsum(counts, 0, dtype=torch.int64)
        n_f = int(fscan[-1])
        if 3 * n_f >= 1 << 31:
            raise RuntimeError(f"remesh_isotropic: {n_f} faces exceed the 31-bit corner ids")
        f2 = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
        sel2 = torch.empty(n_f, dtype=torch.uint8, device=dev)
        L.call("n2m_mesh_subdiv_emit", _p(v2), V, _p(f), F, _p(c2e), _p(split), _p(sscan), _p(fscan.to(torch.int32)), _p(sel), _p(f2), _p(sel2), s)
        src = torch.repeat_interleave(src, counts.long(), output_size=n_f).contiguous()      # a child names its parent's source
        v, f, sel = v2, f2, sel2
    return v, f, sel, src, MAX_SPLIT_ROUNDS


def _collapse_pass(v, f, sel, src, lo2, hi2, cos_f):
    dev = v.device
    s = L.stream()
    V = int(v.shape[0])
    Q = torch.zeros(V, 10, dtype=torch.float64, device=dev)      # n2m_mesh_collapse_apply sums quadrics; this rule has none
    dest = torch.empty(V, dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    ws = torch.empty(2 * V, dtype=torch.int64, device=dev)
    for r in range(MAX_COLLAPSE_ROUNDS):
        F = int(f.shape[0])
        if F == 0:
            return f, sel, src, r
        t = _Topo(v, f, sel, cos_f)
        E = t.E
        keys = torch.empty(E, dtype=torch.int64, device=dev)
        place = torch.empty(E, 3, dtype=torch.float32, device=dev)
        L.call("n2m_mesh_remesh_collapse_cost", _p(v), _p(f), _p(t.edges), _p(t.nf), E, _p(t.vclass), _p(t.efeat), _p(t.vf_off), _p(t.vf_faces),
               _p(t.ve_off), _p(t.ve_edges), lo2, hi2, _p(keys), _p(place), s)
        pick = torch.empty(E, dtype=torch.uint8, device=dev)
        L.call("n2m_mesh_select_collapses", _p(t.edges), _p(t.nf), E, _p(keys), _p(t.ve_off), _p(t.ve_edges), V, _p(ws), ws.numel() * 8, _p(pick),
               _p(totals), s)
        n_sel, removed = (int(x) for x in totals.tolist())       # the round's host read
        if n_sel == 0:
            return f, sel, src, r
        alive = torch.empty(F, dtype=torch.uint8, device=dev)
        L.call("n2m_mesh_collapse_apply", _p(t.edges), E, _p(pick), _p(place), _p(v), _p(Q), V, _p(f), F, _p(dest), _p(alive), s)
        scan = torch.cumsum(alive, 0, dtype=torch.int32)
        n_out = F - removed
        f, src, sel = _compact(f, alive, scan, n_out), _compact(src, alive, scan, n_out), _compact(sel, alive, scan, n_out)
    return f, sel, src, MAX_COLLAPSE_ROUNDS


def _flip_pass(v, f, sel, src, cos_f, devs):
    dev = v.device
    s = L.stream()
    V = int(v.shape[0])
    total = torch.empty(1, dtype=torch.int64, device=dev)
    m1 = torch.empty(V, dtype=torch.int64, device=dev)
    rounds = MAX_FLIP_ROUNDS
    for r in range(MAX_FLIP_ROUNDS):
        t = _Topo(v, f, sel, cos_f)
        E = t.E
        if devs is not None:
            devs.append(t.valence_dev())
        keys = torch.empty(E, dtype=torch.int64, device=dev)
        quads = torch.empty(E, 6, dtype=torch.int32, device=dev)
        L.call("n2m_mesh_remesh_flip_round", _p(v), V, _p(f), _p(sel), _p(src), _p(t.edges), E, _p(t.eoff), _p(t.ecorn), _p(t.efeat), _p(t.vclass),
               _p(t.ve_off), _p(t.ve_edges), _p(keys), _p(quads), _p(m1), _p(total), s)
        if int(total) == 0:                                      # the round's host read
            rounds = r
            break
    else:
        if devs is not None:
            devs.append(_Topo(v, f, sel, cos_f).valence_dev())
    return rounds


def _relax_pass(v, f, sel, cos_f, index=None):
    dev = v.device
    s = L.stream()
    V, F = int(v.shape[0]), int(f.shape[0])
    t = _Topo(v, f, sel, cos_f)
    out = v.clone()
    moved = torch.empty(V, dtype=torch.uint8, device=dev)
    vnormal = torch.empty(V, 3, dtype=torch.float64, device=dev)      # written (and later read) for the moved vertices only
    L.call("n2m_mesh_remesh_relax", _p(v), V, _p(f), _p(t.edges), _p(t.vclass), _p(t.vf_off), _p(t.vf_faces), _p(t.ve_off), _p(t.ve_edges), _p(out),
           _p(moved), _p(vnormal), s)
    projected = 0
    if index is not None:                                        # every moved vertex onto the input surface, rounded to fp32 once
        ids = torch.nonzero(moved).reshape(-1)                   # host read: the number of moved vertices
        projected = int(ids.shape[0])
        if projected:
            _, face, hit = index.closest(out[ids])
            out[ids] = torch.where((face >= 0)[:, None], hit.float(), out[ids])
    revert = torch.empty(V, dtype=torch.uint8, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    reverted = 0
    while True:                                                  # ends: every pass with a non-zero total clears at least one moved flag
        L.call("n2m_mesh_remesh_relax_revert", _p(v), _p(out), V, _p(f), F, _p(moved), _p(vnormal), _p(revert), _p(total), s)
        n = int(total)                                           # the pass's host read
        if n == 0:
            return out, reverted, projected
        reverted += n


def remesh_isotropic(vertices, triangles, target_len, iterations=3, selected=None, feature_deg=30.0, stats=None, project=False):
    """Isotropic explicit re-meshing towards the edge length `target_len` (absolute; the reference's `PureValue`).

    vertices float32 [V, 3], triangles int32/int64 [F, 3], CUDA.  Returns (v [V', 3] float32, f [F', 3] int32, face_src [F'] int64).
    With L = target_len, every iteration (1) splits every edge longer than 4/3 L at its midpoint until none is left, (2) collapses the
    edges shorter than 4/5 L, shortest first, in rounds of independent collapses, where that keeps the surface valid (no face turned against its
    old normal or its vertex's normal) and makes no edge longer than 4/3 L, (3) flips edges while that lowers the squared deviation of the valences from 6 (4 on a boundary), in rounds of
    flips on disjoint vertex quadruples, (4) moves every free vertex to the mean of its neighbours, within its tangent plane and then
    back onto its own one-ring triangles, undoing moves that would flip a face.

    feature_deg: an edge whose face normals differ by more than this angle, a boundary edge and an edge with more than two faces are
    features.  They are never flipped; a vertex on a feature line only collapses along it and is not relaxed; a vertex where a feature
    line ends, branches or turns by more than the angle is frozen.

    selected: optional bool/uint8 [F] face mask (MeshLab's `selectedonly`, strict): only edges whose faces are all selected are split or
    flipped and only vertices whose faces are all selected move or collapse, so unselected faces and their vertices come out bit for bit,
    in their order.  face_src[i] of an unselected face is that input face; a selected face names a selected input face it descends from
    (split child -> parent, flipped pair -> the lower id of the two).

    Edges with more than two faces freeze their endpoints: non-manifold input is kept, not repaired.

    project: after every relaxation, replace every vertex it moved by the closest point of the *input* surface (all of its faces, through
    a mesh_query.MeshIndex built once per call) to its relaxed position, rounded to fp32 once; the undoing of moves that would flip a face
    runs after that, against the positions before the pass.  Without it the surface drifts inward a little with every iteration (DESIGN
    4.15).  Feature and frozen vertices never move, so they are never projected.  False leaves every output bit as it was.

    stats: optional dict, filled with {"iterations": [{"split_rounds", "collapse_rounds", "flip_rounds", "relax_reverts", "faces",
    "valence_dev": [before the first flip round, after every round]}, ...]}; with project=True every entry also has "projected", the
    number of vertices the pass projected."""
    vertices, faces = _check_mesh("remesh_isotropic", vertices, triangles)
    dev = vertices.device
    F = int(faces.shape[0])
    sel = _check_mask("remesh_isotropic", selected, F, dev)
    target_len, iterations, feature_deg = float(target_len), int(iterations), float(feature_deg)
    if not (target_len > 0 and math.isfinite(target_len)):
        raise ValueError("remesh_isotropic: target_len must be > 0")
    if iterations < 0:
        raise ValueError("remesh_isotropic: iterations must be >= 0")
    if not 0.0 <= feature_deg <= 180.0:
        raise ValueError("remesh_isotropic: feature_deg must lie in [0, 180]")
    hi, lo = (4.0 / 3.0) * target_len, (4.0 / 5.0) * target_len
    hi2, lo2 = hi * hi, lo * lo
    cos_f = math.cos(math.radians(feature_deg))                  # once, on the host: no device cos decides anything
    if stats is not None:
        stats["iterations"] = []
    with torch.cuda.device(dev):
        if sel is None:
            sel = torch.ones(F, dtype=torch.uint8, device=dev)
        if iterations == 0 or F == 0 or int(sel.sum()) == 0:
            return vertices.clone(), faces.clone(), torch.arange(F, dtype=torch.int64, device=dev)
        s = L.stream()
        v, f = vertices.clone(), faces.clone()
        src = torch.arange(F, dtype=torch.int32, device=dev)
        index = MeshIndex(vertices, faces) if project else None
        for _ in range(iterations):
            if int(f.shape[0]) == 0:
                break
            v, f, sel, src, n_split = _split_pass(v, f, sel, src, hi2)
            f, sel, src, n_collapse = _collapse_pass(v, f, sel, src, lo2, hi2, cos_f)
            devs = [] if stats is not None else None
            n_flip = _flip_pass(v, f, sel, src, cos_f, devs)
            v, n_revert, n_project = _relax_pass(v, f, sel, cos_f, index)
            if stats is not None:
                stats["iterations"].append({"split_rounds": n_split, "collapse_rounds": n_collapse, "flip_rounds": n_flip, "relax_reverts": n_revert,
                                            "faces": int(f.shape[0]), "valence_dev": [int(x) for x in torch.stack(devs).tolist()]})
                if project:
                    stats["iterations"][-1]["projected"] = n_project
        # drop the vertices the collapses left unreferenced, stably
        V = int(v.shape[0])
        ref = torch.empty(V, dtype=torch.uint8, device=dev)
        L.call("n2m_mesh_mark_referenced", _p(f), int(f.shape[0]), V, _p(ref), s)
        vscan = torch.cumsum(ref, 0, dtype=torch.int32)
        n_v = int(vscan[-1])
        v_out = _compact(v, ref, vscan, n_v)
        f = f.contiguous()
        L.call("n2m_mesh_reindex", _p(f), f.numel(), _p(vscan), s)
    return v_out, f, src.long()
