"""numpy restatement of the device mesh passes (nerf2mesh_amd/mesh_simplify.py, csrc/meshsimplify.hip; rule in DESIGN.md section 4.11).

Written from the rule, not from the kernels: whole-array numpy in fp64, the same operation order wherever a value feeds a comparison, so
the device results are reproduced bit for bit (same faces in the same order, same vertex bits).  Fast enough for meshes of a few thousand
faces.  No GPU and no torch needed."""
import numpy as np

BOUNDARY_WEIGHT = 1.0
MAX_ROUNDS = 512
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def mix_id(h):
    """The key's tie-break: murmur3's 32-bit finaliser of the edge id (a bijection, so keys stay unique)."""
    h = np.asarray(h, np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _plane_terms(n, d, s):
    """[N, 10] terms of s * p p^T, p = (n, d), each rounded as (n_i * n_j) * s."""
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    return np.stack([(x * x) * s, (x * y) * s, (x * z) * s, (x * d) * s, (y * y) * s, (y * z) * s, (y * d) * s, (z * z) * s, (z * d) * s,
                     (d * d) * s], 1)


def _cost(q, p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    r0 = q[:, 0] * x + q[:, 1] * y + q[:, 2] * z + q[:, 3]
    r1 = q[:, 1] * x + q[:, 4] * y + q[:, 5] * z + q[:, 6]
    r2 = q[:, 2] * x + q[:, 5] * y + q[:, 7] * z + q[:, 8]
    r3 = q[:, 3] * x + q[:, 6] * y + q[:, 8] * z + q[:, 9]
    return x * r0 + y * r1 + z * r2 + r3


def edges_of(faces, V):
    """(edges [E, 2] a < b ascending, nf [E], c2e [F, 3]); corner k owns the edge (v_k, v_k+1)."""
    f = faces.astype(np.int64)
    a, b = f, np.roll(f, -1, axis=1)
    key = (np.minimum(a, b) * V + np.maximum(a, b)).reshape(-1)
    uk, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    return np.stack([uk // V, uk % V], 1), cnt, inv.reshape(-1, 3)


def _csr(ids, V):
    off = np.zeros(V + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(ids, minlength=V))
    return off


def quadrics(v, faces, V, nf, c2e, weight=BOUNDARY_WEIGHT):
    """[V, 10] f64: per vertex, faces ascending; per face its area-weighted plane, then the boundary planes of the edge leaving and the
    edge entering the vertex."""
    p = v.astype(np.float64)
    F = faces.shape[0]
    P = [p[faces[:, k]] for k in range(3)]
    n = _cross(P[1] - P[0], P[2] - P[0])
    nn = _dot(n, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        face_terms = _plane_terms(n, -_dot(n, P[0]), 0.5 / np.sqrt(nn))
    face_terms[~(nn > 0)] = 0.0
    bnd_terms = np.zeros((F, 3, 10))                       # corner c: boundary plane of the edge (v_c, v_c+1), zero unless boundary
    for c in range(3):
        a, b = P[c], P[(c + 1) % 3]
        e = b - a
        m = _cross(e, n)
        mm = _dot(m, m)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = _plane_terms(m, -_dot(m, a), (weight * _dot(e, e)) / mm)
        t[~((nf[c2e[:, c]] == 1) & (mm > 0))] = 0.0
        bnd_terms[:, c] = t
    Q = np.zeros((V, 10))
    cv = faces.reshape(-1)
    order = np.argsort(cv, kind="stable")
    off = _csr(cv, V)
    deg = np.diff(off)
    for j in range(int(deg.max()) if V else 0):
        vs = np.nonzero(deg > j)[0]
        corner = order[off[vs] + j]
        fid, k = corner // 3, corner % 3
        Q[vs] += face_terms[fid]                            # explicit sequence of adds: the device's order
        Q[vs] += bnd_terms[fid, k]
        Q[vs] += bnd_terms[fid, (k + 2) % 3]
    return Q


def _round(v, faces, Q, sel, target_left, optimal):
    """One round: (ids of the edges to collapse, edges, placement f32 [E, 3], nf)."""
    V = v.shape[0]
    edges, nf, c2e = edges_of(faces, V)
    E = edges.shape[0]
    a, b = edges[:, 0], edges[:, 1]
    # vertex flags
    frozen = np.zeros(V, bool)
    bnd = np.zeros(V, bool)
    for c in range(3):
        e = c2e[:, c]
        for w in (faces[:, c], faces[:, (c + 1) % 3]):
            frozen[w[nf[e] > 2]] = True
            bnd[w[nf[e] == 1]] = True
    if sel is not None:
        frozen[faces[sel == 0].reshape(-1)] = True
    bad = (nf > 2) | frozen[a] | frozen[b] | ((nf == 2) & bnd[a] & bnd[b])
    # link condition: common neighbours == faces on the edge
    keyset = a * V + b
    nbr_v = np.concatenate([a, b])
    nbr_o = np.concatenate([b, a])
    o = np.argsort(nbr_v * V + nbr_o)
    nbr_v, nbr_o = nbr_v[o], nbr_o[o]
    off = _csr(nbr_v, V)
    deg = np.diff(off)
    rows = np.repeat(np.arange(E), deg[a])
    cs = nbr_o[np.repeat(off[a], deg[a]) + np.arange(rows.size) - np.repeat(np.cumsum(deg[a]) - deg[a], deg[a])]
    bb = b[rows]
    k2 = np.minimum(bb, cs) * V + np.maximum(bb, cs)
    pos = np.searchsorted(keyset, k2)
    hit = (pos < E) & (keyset[np.minimum(pos, E - 1)] == k2) & (cs != bb)
    common = np.bincount(rows[hit], minlength=E)
    bad |= common != nf
    # placement and cost
    p = v.astype(np.float64)
    q = Q[a] + Q[b]
    pa, pb = p[a], p[b]
    mid = (pa + pb) * 0.5
    P = np.zeros((E, 3))
    solved = np.zeros(E, bool)
    if optimal:
        c00, c01, c02 = q[:, 4] * q[:, 7] - q[:, 5] * q[:, 5], q[:, 5] * q[:, 2] - q[:, 1] * q[:, 7], q[:, 1] * q[:, 5] - q[:, 4] * q[:, 2]
        c11, c12, c22 = q[:, 0] * q[:, 7] - q[:, 2] * q[:, 2], q[:, 2] * q[:, 1] - q[:, 0] * q[:, 5], q[:, 0] * q[:, 4] - q[:, 1] * q[:, 1]
        det = q[:, 0] * c00 + q[:, 1] * c01 + q[:, 2] * c02
        tr = q[:, 0] + q[:, 4] + q[:, 7]
        ok = np.abs(det) > 1e-12 * (tr * tr * tr)
        r0, r1, r2 = -q[:, 3], -q[:, 6], -q[:, 8]
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.stack([(c00 * r0 + c01 * r1 + c02 * r2) / det, (c01 * r0 + c11 * r1 + c12 * r2) / det, (c02 * r0 + c12 * r1 + c22 * r2) / det], 1)
            dm, ab = x - mid, pb - pa
            ok &= _dot(dm, dm) <= 4.0 * _dot(ab, ab)
            P[ok] = x[ok].astype(np.float32).astype(np.float64)
        solved = ok
    pm = mid.astype(np.float32).astype(np.float64)
    ca, cb, cm = _cost(q, pa), _cost(q, pb), _cost(q, pm)
    best, cost = pa.copy(), ca.copy()
    t = cb < cost
    best[t], cost[t] = pb[t], cb[t]
    t = cm < cost
    best[t], cost[t] = pm[t], cm[t]
    P[~solved] = best[~solved]
    cost = np.where(solved, _cost(q, P), cost)
    # flips: every face around a or b that does not contain both
    cv = faces.reshape(-1)
    vorder = np.argsort(cv, kind="stable")
    voff = _csr(cv, V)
    for endpoint in (a, b):
        cand = np.nonzero(~bad)[0]
        ends = endpoint[cand]
        cnt = voff[ends + 1] - voff[ends]
        rows = np.repeat(cand, cnt)
        if rows.size == 0:
            continue
        starts = np.repeat(voff[ends], cnt)
        within = np.arange(rows.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        fid = vorder[starts + within] // 3
        t = faces[fid]
        ea, eb = a[rows][:, None], b[rows][:, None]
        is_ab = (t == ea) | (t == eb)
        keep = ~(((t == ea).any(1)) & ((t == eb).any(1)))
        O = [p[t[:, k]] for k in range(3)]
        W = [np.where(is_ab[:, k:k + 1], P[rows], O[k]) for k in range(3)]
        n0 = _cross(O[1] - O[0], O[2] - O[0])
        n1 = _cross(W[1] - W[0], W[2] - W[0])
        flip = keep & ~(_dot(n1, n0) > 0)
        bad[np.unique(rows[flip])] = True
    c32 = np.where(cost > 0, cost, 0.0).astype(np.float32)
    keys = (c32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | mix_id(np.arange(E, dtype=np.uint32)).astype(np.uint64)
    keys[bad] = NO_KEY
    # independent set
    m1 = np.full(V, NO_KEY)
    np.minimum.at(m1, a, keys)
    np.minimum.at(m1, b, keys)
    m2 = m1.copy()
    np.minimum.at(m2, a, m1[b])
    np.minimum.at(m2, b, m1[a])
    pick = (keys != NO_KEY) & (keys == m2[a]) & (keys == m2[b])
    idx = np.nonzero(pick)[0]
    if idx.size and nf[idx].sum() > target_left:
        idx = idx[np.argsort(keys[idx])]
        rem = nf[idx]
        idx = idx[(np.cumsum(rem) - rem) < target_left]
    return idx, edges, P.astype(np.float32), nf


def decimate(v, faces, target, optimal_placement=True, selected=None, boundary_weight=BOUNDARY_WEIGHT):
    """-> (v, f, face_src) like nerf2mesh_amd.mesh_simplify.decimate; rounds in the same rule."""
    v = np.asarray(v, np.float32).copy()
    f = np.asarray(faces, np.int64).copy()
    V, F = v.shape[0], f.shape[0]
    sel = None if selected is None else (np.asarray(selected) != 0).astype(np.uint8)
    n_count = F if sel is None else int(sel.sum())
    src = np.arange(F)
    if target >= n_count or F == 0:
        return v, f.astype(np.int32), src
    edges, nf, c2e = edges_of(f, V)
    Q = quadrics(v, f, V, nf, c2e, boundary_weight)
    for _ in range(MAX_ROUNDS):
        idx, edges, P, nf = _round(v, f, Q, sel, n_count - target, optimal_placement)
        if idx.size == 0:
            break
        a, b = edges[idx, 0], edges[idx, 1]
        v[a] = P[idx]
        Q[a] = Q[a] + Q[b]
        dest = np.arange(V)
        dest[b] = a
        f = dest[f]
        alive = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
        f, src = f[alive], src[alive]
        if sel is not None:
            sel = sel[alive]
        n_count -= int(nf[idx].sum())
        if n_count <= target:
            break
    ref = np.zeros(V, bool)
    ref[f.reshape(-1)] = True
    new_id = np.cumsum(ref) - 1
    return v[ref], new_id[f].astype(np.int32), src


def subdivide_midpoint(v, faces, threshold, selected=None, iterations=3):
    """-> (v, f) like nerf2mesh_amd.mesh_simplify.subdivide_midpoint."""
    v = np.asarray(v, np.float32)
    f = np.asarray(faces, np.int64)
    sel = np.ones(f.shape[0], np.uint8) if selected is None else (np.asarray(selected) != 0).astype(np.uint8)
    thr2 = float(threshold) * float(threshold)
    for _ in range(iterations):
        V, F = v.shape[0], f.shape[0]
        edges, _, c2e = edges_of(f, V)
        p = v.astype(np.float64)
        split = np.zeros(edges.shape[0], bool)
        for k in range(3):
            d = p[f[:, (k + 1) % 3]] - p[f[:, k]]
            long_ = (_dot(d, d) > thr2) & (sel != 0)
            split[c2e[long_, k]] = True
        n_new = int(split.sum())
        if n_new == 0:
            break
        mid_id = np.full(edges.shape[0], -1)
        mid_id[split] = V + np.arange(n_new)
        mids = ((p[edges[split, 0]] + p[edges[split, 1]]) * 0.5).astype(np.float32)
        v = np.concatenate([v, mids])
        p = v.astype(np.float64)
        out, out_sel = [], []
        for fi in range(F):
            t = f[fi]
            m = [mid_id[c2e[fi, k]] for k in range(3)]
            pat = sum(1 << k for k in range(3) if m[k] >= 0)
            if pat == 0:
                ch = [(t[0], t[1], t[2])]
            elif pat == 7:
                ch = [(t[0], m[0], m[2]), (t[1], m[1], m[0]), (t[2], m[2], m[1]), (m[0], m[1], m[2])]
            elif pat in (1, 2, 4):
                k = {1: 0, 2: 1, 4: 2}[pat]
                vk, vk1, vk2 = t[k], t[(k + 1) % 3], t[(k + 2) % 3]
                ch = [(vk, m[k], vk2), (m[k], vk1, vk2)]
            else:
                k = {6: 0, 5: 1, 3: 2}[pat]
                vk, vk1, vk2 = t[k], t[(k + 1) % 3], t[(k + 2) % 3]
                m1, m2 = m[(k + 1) % 3], m[(k + 2) % 3]
                d1, d2 = p[m1] - p[vk], p[m2] - p[vk1]
                l1 = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2]
                l2 = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2]
                ch = [(m1, vk2, m2)] + ([(vk, vk1, m1), (vk, m1, m2)] if l1 <= l2 else [(vk, vk1, m2), (vk1, m1, m2)])
            out += ch
            out_sel += [sel[fi]] * len(ch)
        f = np.asarray(out, np.int64)
        sel = np.asarray(out_sel, np.uint8)
    return v, f.astype(np.int32)


def refine_classes(errors, cnt, n_inner, sdf=False):
    """Face classes of nerf/renderer.py:219-244: 2 refine (> 90th percentile), 1 decimate (< 50th), 0 otherwise, over the seen inner faces."""
    errors = np.asarray(errors, np.float32).copy()
    cnt = np.asarray(cnt, np.float32)
    seen = cnt > 0
    errors[seen] = errors[seen] / cnt[seen]
    errors, seen = errors[:n_inner], seen[:n_inner]
    if sdf:
        return np.ones(n_inner, np.uint8)
    mask = np.zeros(n_inner, np.uint8)
    if not seen.any():
        return mask
    t_ref = np.percentile(errors[seen], 90)
    t_dec = np.percentile(errors[seen], 50)
    mask[(errors > t_ref) & seen] = 2
    mask[(errors < t_dec) & seen] = 1
    return mask


def refine(v, f, mask, decimate_ratio=0.1, refine_size=0.01):
    """decimate_and_refine_mesh (meshutils.py:191-231) without the re-meshing: selected decimation of class 1 carrying the classes, then
    selected subdivision of class 2."""
    mask = np.asarray(mask, np.uint8)
    if decimate_ratio > 0:
        n1 = int((mask == 1).sum())
        v, f, src = decimate(v, f, int((1 - decimate_ratio) * n1), optimal_placement=True, selected=(mask == 1))
        mask = mask[src]
    if refine_size > 0:
        v, f = subdivide_midpoint(v, f, refine_size, selected=(mask == 2))
    return v, f


# ---------------------------------------------------------------------------------------------------------- test meshes
def icosphere(level=2, radius=1.0):
    """Closed sphere: an icosahedron with `level` rounds of 4-way splits, projected to the sphere (f32 vertices, i32 faces)."""
    t = (1.0 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        cache, nf = {}, []

        def mid(i, j):
            k = (min(i, j), max(i, j))
            if k not in cache:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius).astype(np.float32), np.asarray(f, np.int32)


def torus(n_major=48, n_minor=24, R=1.0, r=0.35):
    """Closed genus-1 surface (V - E + F = 0)."""
    i, j = np.meshgrid(np.arange(n_major), np.arange(n_minor), indexing="ij")
    u, w = 2 * np.pi * i / n_major, 2 * np.pi * j / n_minor
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], -1).reshape(-1, 3)
    idx = lambda a, b: (a % n_major) * n_minor + (b % n_minor)   # noqa: E731
    f = []
    for a in range(n_major):
        for b in range(n_minor):
            f += [(idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)), (idx(a, b), idx(a + 1, b + 1), idx(a, b + 1))]
    return v.astype(np.float32), np.asarray(f, np.int32)


def grid_patch(n=24, h=1.0 / 16, jitter=False):
    """Open planar patch z = 0 on a dyadic grid (every quadric term exact), alternating diagonals; corners (0, 0) and (n h, n h) etc."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    v = np.stack([i * h, j * h, np.zeros_like(i, dtype=np.float64)], -1).reshape(-1, 3)
    f = []
    for a in range(n):
        for b in range(n):
            p, q, r, s = a * (n + 1) + b, (a + 1) * (n + 1) + b, (a + 1) * (n + 1) + b + 1, a * (n + 1) + b + 1
            f += [(p, q, r), (p, r, s)] if (a + b) % 2 == 0 else [(p, q, s), (q, r, s)]
    return v.astype(np.float32), np.asarray(f, np.int32)


def with_fin(v, f):
    """Adds a fin: a second face on one edge of the mesh and a third on the same edge (an edge with 3 faces: non-manifold)."""
    a, b, c = f[0]
    ctr = (v[a] + v[b]) / 2
    n = np.cross(v[b] - v[a], v[c] - v[a])
    tip = (ctr + 0.3 * n / np.linalg.norm(n)).astype(np.float32)
    v2 = np.concatenate([v, tip[None]])
    return v2, np.concatenate([f, np.asarray([[a, b, len(v)]], np.int32)])


def edge_face_counts(f):
    _, nf, _ = edges_of(np.asarray(f), int(np.asarray(f).max()) + 1)
    return nf


def euler(v, f):
    f = np.asarray(f)
    return len(np.unique(f)) - len(edge_face_counts(f)) + len(f)


def signed_volume(v, f):
    p = np.asarray(v, np.float64)[np.asarray(f)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def area(v, f):
    p = np.asarray(v, np.float64)[np.asarray(f)]
    return float(np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).sum() / 2.0)
