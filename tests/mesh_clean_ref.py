"""Sequential numpy restatement of the device mesh cleaning (nerf2mesh_amd/mesh_clean.py, csrc/meshclean.hip; rule in DESIGN.md section
4.12).

Written from the rule and sequential, as vcg is: the greedy vertex sweep over a grid, the area-ordered deletion loop and the per-vertex fan
walk visit one element after the other, so checking the device's parallel rounds against it is an independent check.  The round counts
the device reports follow from the same sequential pass (the round in which each element decides).  Inputs of up to ~100 k vertices run
in seconds.  No GPU and no torch needed."""
import itertools
import math

import numpy as np

from mesh_simplify_ref import edge_face_counts, edges_of, grid_patch, icosphere, torus, with_fin  # noqa: F401  (re-exported helpers)

CELL_MARGIN = 1.0 + 2.0 ** -10
STAT_KEYS = ("unreferenced", "merged", "degenerate", "duplicate", "null", "components", "diameter_components", "diameter_faces",
             "size_components", "size_faces", "nonmanifold_faces", "split_vertices", "merge_rounds", "nonmanifold_rounds")


def box_diagonal(lo, hi):
    dx, dy, dz = (float(h) - float(l) for l, h in zip(lo, hi))
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def _bbox(v):
    return [float(x) for x in v.min(0)], [float(x) for x in v.max(0)]


def _drop_unreferenced(v, f):
    ref = np.zeros(len(v), bool)
    ref[f.reshape(-1)] = True
    new_id = np.cumsum(ref) - 1
    return v[ref], new_id[f].reshape(-1, 3), int(len(v) - ref.sum())


def close_pairs(v, r2):
    """All (i, j), i != j, with (dx*dx + dy*dy) + dz*dz < r2 in fp64 of the fp32 coordinates, found through a uniform grid of cells
    larger than r (each point's 27 surrounding cells).  Sorted by (i, j)."""
    p = np.asarray(v, np.float64)
    V = len(p)
    h = math.sqrt(r2) * CELL_MARGIN
    c = np.floor((p - p.min(0)) / h).astype(np.int64)
    n = c.max(0) + 1
    key = (c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2]
    order = np.argsort(key, kind="stable")
    sk = key[order]
    I, J = [], []
    for d in itertools.product((-1, 0, 1), repeat=3):
        cc = c + np.asarray(d)
        ok = ((cc >= 0) & (cc < n)).all(1)
        k2 = (cc[:, 0] * n[1] + cc[:, 1]) * n[2] + cc[:, 2]
        lo, hi = np.searchsorted(sk, k2, "left"), np.searchsorted(sk, k2, "right")
        cnt = np.where(ok, hi - lo, 0)
        tot = int(cnt.sum())
        if tot == 0:
            continue
        I.append(np.repeat(np.arange(V), cnt))
        J.append(order[np.repeat(lo, cnt) + np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt)])
    if not I:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    I, J = np.concatenate(I), np.concatenate(J)
    d = p[J] - p[I]
    m = (I != J) & (((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < r2)
    I, J = I[m], J[m]
    o = np.lexsort((J, I))
    return I[o], J[o]


def merge_close(v, r2):
    """The greedy sweep (vcg ClusterVertex): vertices in index order; an unclaimed one becomes a seed and claims every unclaimed vertex
    closer than r.  -> (dest [V]: own id for a seed, the claiming seed otherwise; the device's round count)."""
    V = len(v)
    I, J = close_pairs(v, r2)
    off = np.searchsorted(I, np.arange(V + 1))
    dest = np.full(V, -1, np.int64)
    for i in range(V):
        if dest[i] >= 0:
            continue
        dest[i] = i
        nb = J[off[i]:off[i + 1]]
        dest[nb[dest[nb] < 0]] = i
    # the round in which the device decides each vertex: a seed once all its lower neighbours are decided, a claimed vertex once its seed
    # and all its lower neighbours below the seed are (a decision made in round t is seen in round t + 1)
    rnd = np.zeros(V, np.int64)
    for i in range(V):
        nb = J[off[i]:off[i + 1]]
        low = nb[nb < i]
        if dest[i] != i:
            s = int(dest[i])
            low = np.append(low[low < s], s)
        rnd[i] = 1 + (int(rnd[low].max()) if low.size else 0)
    return dest, int(rnd.max()) if V else 0


def _cross(v, f):
    p = np.asarray(v, np.float64)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    u, w = b - a, c - a
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)


def components(f, V):
    """Edge-connected components by a sequential union-find -> label [F] = the smallest face id of the component."""
    F = len(f)
    _, _, c2e = edges_of(f, V)
    rep = np.full(int(c2e.max()) + 1, F, np.int64)
    np.minimum.at(rep, c2e.reshape(-1), np.repeat(np.arange(F), 3))
    parent = list(range(F))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, e in enumerate(c2e.reshape(-1).tolist()):
        a, b = find(i // 3), find(int(rep[e]))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.asarray([find(x) for x in range(F)], np.int64)


def fans(f, V):
    """Per vertex, its corners (flat ids, ascending) split into fans: list over vertices of lists of sorted corner lists, the fan of the
    first corner first.  Sequential walk over the faces sharing an edge (v, w)."""
    flat = f.reshape(-1)
    order = np.argsort(flat, kind="stable")
    off = np.searchsorted(flat[order], np.arange(V + 1))
    out = []
    for v in range(V):
        corners = order[off[v]:off[v + 1]].tolist()
        left, groups = list(corners), []
        while left:
            fan, stack = {left[0]}, [left[0]]
            while stack:
                c = stack.pop()
                fc, kc = divmod(c, 3)
                ws = {int(f[fc, (kc + 1) % 3]), int(f[fc, (kc + 2) % 3])}
                for d in left:
                    if d not in fan:
                        fd, kd = divmod(d, 3)
                        if int(f[fd, (kd + 1) % 3]) in ws or int(f[fd, (kd + 2) % 3]) in ws:
                            fan.add(d)
                            stack.append(d)
            groups.append(sorted(fan))
            left = [d for d in left if d not in fan]
        out.append(groups)
    return out


def clean_mesh(v, f, v_pct=1, min_f=8, min_d=5, repair=True):
    """-> (v, f, face_src, stats) like nerf2mesh_amd.mesh_clean.clean_mesh (remesh is not part of the rule)."""
    v = np.asarray(v, np.float32).copy()
    f = np.asarray(f, np.int64).reshape(-1, 3).copy()
    src = np.arange(len(f))
    st = dict.fromkeys(STAT_KEYS, 0)
    # 1
    v, f, st["unreferenced"] = _drop_unreferenced(v, f)
    V = len(v)
    live = np.ones(V, bool)
    # 2
    if v_pct > 0 and V:
        r = float(v_pct) / 100.0 * box_diagonal(*_bbox(v))
        if r * r > 0:
            dest, st["merge_rounds"] = merge_close(v, r * r)
            live = dest == np.arange(V)
            st["merged"] = int(V - live.sum())
            f = dest[f]
            ok = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
            st["degenerate"] = int((~ok).sum())
            f, src = f[ok], src[ok]
    # 3, 4
    if len(f):
        _, first = np.unique(np.sort(f, 1), axis=0, return_index=True)
        keep = np.zeros(len(f), bool)
        keep[first] = True
        st["duplicate"] = int((~keep).sum())
        f, src = f[keep], src[keep]
        null = (_cross(v, f) == 0).all(1)
        st["null"] = int(null.sum())
        f, src = f[~null], src[~null]
    # 5
    if len(f):
        F = len(f)
        label = components(f, V)
        roots = np.unique(label)
        count = np.bincount(label, minlength=F)
        lo = np.full((F, 3), np.inf, np.float32)
        hi = np.full((F, 3), -np.inf, np.float32)
        np.minimum.at(lo, np.repeat(label, 3), v[f.reshape(-1)])
        np.maximum.at(hi, np.repeat(label, 3), v[f.reshape(-1)])
        dd = hi.astype(np.float64) - lo.astype(np.float64)
        with np.errstate(invalid="ignore"):
            diag = np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])
        if min_d > 0:
            min_diag = float(min_d) / 100.0 * box_diagonal(*_bbox(v[live]))
            by_d = diag[label] < min_diag
        else:
            by_d = np.zeros(F, bool)
        by_s = ~by_d & (count[label] < math.ceil(min_f)) if min_f > 0 else np.zeros(F, bool)
        st["components"] = len(roots)
        st["diameter_components"], st["diameter_faces"] = int(by_d[roots].sum()), int(by_d.sum())
        st["size_components"], st["size_faces"] = int(by_s[roots].sum()), int(by_s.sum())
        keep = ~(by_d | by_s)
        f, src = f[keep], src[keep]
    # 6 (vcg RemoveNonManifoldFace)
    if repair and len(f):
        _, nf, c2e = edges_of(f, V)
        cand = np.nonzero((nf[c2e] > 2).any(1))[0]
        if cand.size:
            n = _cross(v, f)
            da = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
            seq = cand[np.lexsort((cand, da[cand]))]
            live_nf = nf.copy()
            deleted = np.zeros(len(f), bool)
            rnd = {}
            on_edge = {}                                     # non-manifold edge -> candidates already visited (smaller keys)
            for c in seq.tolist():
                es = c2e[c]
                if (live_nf[es] > 2).any():
                    deleted[c] = True
                    live_nf[es] -= 1
                before = [g for e in es.tolist() if nf[e] > 2 for g in on_edge.get(e, [])]
                rnd[c] = 1 + max((rnd[g] for g in before), default=0)
                for e in es.tolist():
                    if nf[e] > 2:
                        on_edge.setdefault(e, []).append(c)
            st["nonmanifold_faces"] = int(deleted.sum())
            st["nonmanifold_rounds"] = max(rnd.values())
            f, src = f[~deleted], src[~deleted]
    # 7 (vcg SplitNonManifoldVertex, vertdispratio = 0)
    if repair and len(f):
        splits = [(groups[0][0], vid, groups[0]) for vid, groups in enumerate(fans(f, V)) if len(groups) > 1]
        splits.sort()
        st["split_vertices"] = len(splits)
        flat = f.reshape(-1)
        for k, (_, vid, fan) in enumerate(splits):
            flat[fan] = V + k
        f = flat.reshape(-1, 3)
        if splits:
            v = np.concatenate([v, v[[vid for _, vid, _ in splits]]])
    v, f, _ = _drop_unreferenced(v, f)
    return v, f.astype(np.int32), src, st


def fan_counts(f, V):
    """Fans per vertex (0 for an unreferenced vertex)."""
    return np.asarray([len(g) for g in fans(np.asarray(f, np.int64), V)])
