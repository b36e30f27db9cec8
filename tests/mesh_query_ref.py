"""numpy restatement of the closest-point query (nerf2mesh_amd/mesh_query.py, csrc/meshquery.hip; rule in DESIGN.md section 4.15) and of
the re-meshing with re-projection (`remesh_isotropic(project=True)`).

The query is the exhaustive scan: every face against every point, in fp64 with the device's operation order, the lexicographic minimum of
(d2, face id).  The device walks a hierarchy instead and must return the same bits.  The re-meshing runs mesh_remesh_ref's own split,
collapse and flip passes; only the relaxation is restated here, with the projection between the relaxation and the undoing of moves.
No GPU and no torch needed."""
import numpy as np

import mesh_remesh_ref as M
from mesh_simplify_ref import _dot

PAIRS = 1 << 18        # (point, face) pairs per chunk of the scan


def closest(v, f, points):
    """-> (d2 f64 [N], face i32 [N], point f64 [N, 3]): for every point the face with the lowest (d2, id), d2 = |c - p|^2 with c =
    mesh_remesh_ref.closest_on_triangle.  A face with a repeated vertex index does not count, a face whose d2 is not finite never wins
    (NaN is not < anything); no face at all: d2 = inf, face = -1, point = NaN."""
    p = np.asarray(v, np.float32).astype(np.float64)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    pts = np.asarray(points).astype(np.float64).reshape(-1, 3)
    N, F = len(pts), len(f)
    d2, face, hit = np.full(N, np.inf), np.full(N, -1, np.int32), np.full((N, 3), np.nan)
    if F == 0 or N == 0:
        return d2, face, hit
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    out = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])
    step = max(1, PAIRS // F)
    for s in range(0, N, step):
        q = pts[s:s + step]
        Q = len(q)
        qq = np.repeat(q, F, axis=0)
        cc = M.closest_on_triangle(qq, np.tile(a, (Q, 1)), np.tile(b, (Q, 1)), np.tile(c, (Q, 1)))
        d = cc - qq
        with np.errstate(invalid="ignore", over="ignore"):
            dd = _dot(d, d).reshape(Q, F)
        dd = np.where(np.isnan(dd) | out[None, :], np.inf, dd)
        j = np.argmin(dd, axis=1)                                # the first minimum: the lowest face id on a tie
        best = dd[np.arange(Q), j]
        won = best < np.inf
        d2[s:s + step] = best
        face[s:s + step] = np.where(won, j, -1)
        hit[s:s + step] = np.where(won[:, None], cc.reshape(Q, F, 3)[np.arange(Q), j], np.nan)
    return d2, face, hit


def relax_project(v, f, sel, cos_f, v0, f0):
    """mesh_remesh_ref.relax with the projection: every vertex the relaxation moved is replaced by the closest point of (v0, f0) to its
    relaxed (fp32) position, rounded to fp32 once, before the moves that would turn a face are undone.
    -> (new vertices f32, vertices put back, vertices projected, mask of the vertices moved and not put back)."""
    t = M.Topo(v, f, sel, cos_f)
    p, V = t.p, t.V
    deg, degf = t.valence, np.diff(t.vf_off)
    q, n = np.zeros((V, 3)), t.vertex_normals()
    for j in range(int(deg.max()) if V else 0):
        vs = np.nonzero(deg > j)[0]
        q[vs] = q[vs] + p[t.ve_other[t.ve_off[vs] + j]]
    nn = _dot(n, n)
    movable = (t.vclass == 0) & (deg > 0) & (nn > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = q / deg[:, None].astype(np.float64)
        r = q + n * (_dot(n, p - q) / nn)[:, None]
    best = np.full(V, np.inf)
    hit = p.copy()
    for j in range(int(degf.max()) if V else 0):
        vs = np.nonzero(movable & (degf > j))[0]
        tri = f[t.vf_faces[t.vf_off[vs] + j]]
        c = M.closest_on_triangle(r[vs], p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]])
        d = c - r[vs]
        dd = _dot(d, d)
        up = dd < best[vs]
        best[vs[up]] = dd[up]
        hit[vs[up]] = c[up]
    moved = movable & (best < np.inf)
    out = v.copy()
    out[moved] = hit[moved].astype(np.float32)
    ids = np.nonzero(moved)[0]
    if len(ids):
        _, face, c = closest(v0, f0, out[ids])
        out[ids] = np.where((face >= 0)[:, None], c.astype(np.float32), out[ids])
    reverted = 0
    while True:
        touched = moved[f].any(1)
        g = M._normals(out.astype(np.float64), f)
        ok = _dot(g, t.fn) > 0
        for k in range(3):
            ok &= ~moved[f[:, k]] | (_dot(g, n[f[:, k]]) > 0)
        bad = touched & ~ok
        back = np.zeros(V, bool)
        back[f[bad].reshape(-1)] = True
        back &= moved
        if not back.any():
            return out, reverted, len(ids), moved
        out[back] = v[back]
        moved &= ~back
        reverted += int(back.sum())


def remesh_isotropic(v, faces, target_len, iterations=3, selected=None, feature_deg=30.0, stats=None, hook=None, info=None):
    """nerf2mesh_amd.mesh_remesh.remesh_isotropic(project=True): mesh_remesh_ref.remesh_isotropic's loop with relax_project in the place
    of relax.  info: optional dict; info["on_surface"] <- mask over the output vertices of those the last relaxation moved, projected
    and did not put back."""
    v = np.asarray(v, np.float32).copy()
    f = np.asarray(faces, np.int64).copy()
    v0, f0 = v.copy(), f.copy()
    F = f.shape[0]
    sel = np.ones(F, np.uint8) if selected is None else (np.asarray(selected) != 0).astype(np.uint8)
    src = np.arange(F)
    if stats is not None:
        stats["iterations"] = []
    if iterations == 0 or F == 0 or sel.sum() == 0:
        if info is not None:
            info["on_surface"] = np.zeros(len(v), bool)
        return v, f.astype(np.int32), src
    lo2, hi2 = M.thresholds(target_len)
    cos_f = M.cos_feature(feature_deg)
    kept = np.zeros(len(v), bool)
    for it in range(iterations):
        if f.shape[0] == 0:
            break
        n_split = M.MAX_SPLIT_ROUNDS
        for r in range(M.MAX_SPLIT_ROUNDS):
            v, f, sel, src, n = M.split_round(v, f, sel, src, hi2)
            if n == 0:
                n_split = r
                break
        if hook:
            hook("split", it, v, f, sel)
        n_collapse = M.MAX_COLLAPSE_ROUNDS
        for r in range(M.MAX_COLLAPSE_ROUNDS):
            f, sel, src, n = M.collapse_round(v, f, sel, src, lo2, hi2, cos_f)
            if n == 0:
                n_collapse = r
                break
        if hook:
            hook("collapse", it, v, f, sel)
        n_flip, devs = M.MAX_FLIP_ROUNDS, []
        for r in range(M.MAX_FLIP_ROUNDS):
            n, dev = M.flip_round(v, f, sel, src, cos_f)
            devs.append(dev)
            if n == 0:
                n_flip = r
                break
        else:
            devs.append(M.Topo(v, f, sel, cos_f).valence_dev())
        if hook:
            hook("flip", it, v, f, sel)
        v, n_revert, n_project, kept = relax_project(v, f, sel, cos_f, v0, f0)
        if hook:
            hook("relax", it, v, f, sel)
        if stats is not None:
            stats["iterations"].append({"split_rounds": n_split, "collapse_rounds": n_collapse, "flip_rounds": n_flip, "relax_reverts": n_revert,
                                        "faces": int(f.shape[0]), "valence_dev": devs, "projected": n_project})
    ref = np.zeros(v.shape[0], bool)
    ref[f.reshape(-1)] = True
    new_id = np.cumsum(ref) - 1
    if info is not None:
        info["on_surface"] = kept[ref] if len(kept) == len(ref) else np.zeros(int(ref.sum()), bool)
    return v[ref], new_id[f].astype(np.int32), src
