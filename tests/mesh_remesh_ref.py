"""numpy restatement of the device isotropic re-meshing (nerf2mesh_amd/mesh_remesh.py, csrc/meshremesh.hip; rule in DESIGN.md section 4.14).

Written from the rule: whole-array numpy in fp64 with the same operation order wherever a value feeds a comparison or is stored, so the
device results are reproduced bit for bit (same faces in the same order, same vertex bits, same face sources, same round counts).  Fast
enough for meshes of some ten thousand faces.  No GPU and no torch needed."""
import math

import numpy as np

import mesh_simplify_ref as R
from mesh_simplify_ref import _cross, _csr, _dot, mix_id, NO_KEY  # noqa: F401

MAX_SPLIT_ROUNDS = 32
MAX_COLLAPSE_ROUNDS = 128
MAX_FLIP_ROUNDS = 128
FROZEN, BOUNDARY, FEATURE = 1, 2, 4
MAX_GAIN = 1 << 30


def thresholds(target_len):
    hi, lo = (4.0 / 3.0) * float(target_len), (4.0 / 5.0) * float(target_len)
    return lo * lo, hi * hi


def cos_feature(feature_deg):
    return math.cos(math.radians(float(feature_deg)))


def _expand(off, ids):
    """Rows of a CSR for a list of row ids: (index into ids of every item, position of the item in the CSR's value array)."""
    cnt = off[ids + 1] - off[ids]
    rows = np.repeat(np.arange(len(ids)), cnt)
    within = np.arange(rows.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return rows, np.repeat(off[ids], cnt) + within


def _normals(p, f):
    return _cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])


class Topo:
    """Edges, CSRs (vertex -> faces ascending, vertex -> edges by ascending neighbour, edge -> corners ascending) and the classes."""

    def __init__(self, v, f, sel, cos_f):
        V = v.shape[0]
        self.V = V
        self.edges, self.nf, self.c2e = R.edges_of(f, V)
        E = self.E = self.edges.shape[0]
        a, b = self.edges[:, 0], self.edges[:, 1]
        self.ekeys = a * V + b
        flat = self.c2e.reshape(-1)
        self.ecorn = np.argsort(flat, kind="stable")
        self.eoff = _csr(flat, E)
        cv = f.reshape(-1)
        self.vf_faces = np.argsort(cv, kind="stable") // 3
        self.vf_off = _csr(cv, V)
        ends, other = np.concatenate([a, b]), np.concatenate([b, a])
        o = np.argsort(ends * V + other)
        self.ve_edges, self.ve_other, self.ve_vertex = np.tile(np.arange(E), 2)[o], other[o], ends[o]
        self.ve_off = _csr(ends, V)
        self.valence = np.diff(self.ve_off)
        p = self.p = v.astype(np.float64)
        self.fn = _normals(p, f)
        # the flags of 4.11: frozen on an edge with more than two faces or on an unselected face, boundary on an edge with one face
        flags = np.zeros(V, np.int64)
        flags[np.unique(self.edges[self.nf > 2])] |= FROZEN
        flags[np.unique(self.edges[self.nf == 1])] |= BOUNDARY
        flags[np.unique(f[sel == 0])] |= FROZEN
        # feature edges
        efeat = self.nf != 2
        two = np.nonzero(self.nf == 2)[0]
        n0, n1 = self.fn[self.ecorn[self.eoff[two]] // 3], self.fn[self.ecorn[self.eoff[two] + 1] // 3]
        efeat[two] = _dot(n0, n1) < cos_f * (np.sqrt(_dot(n0, n0)) * np.sqrt(_dot(n1, n1)))
        self.efeat = efeat
        # vertex classes
        on = efeat[self.ve_edges]
        fv, fo = self.ve_vertex[on], self.ve_other[on]
        n = np.bincount(fv, minlength=V)
        vclass = flags.copy()
        vclass[(n != 0) & (n != 2)] |= FROZEN
        vs = np.nonzero(n == 2)[0]
        first = np.searchsorted(fv, vs)
        d1, d2 = p[fo[first]] - p[vs], p[fo[first + 1]] - p[vs]
        corner = _dot(d1, d2) > -cos_f * (np.sqrt(_dot(d1, d1)) * np.sqrt(_dot(d2, d2)))
        vclass[vs[corner]] |= FROZEN
        vclass[vs[~corner]] |= FEATURE
        self.vclass = vclass

    def vertex_normals(self):
        """[V, 3]: the sum of the cross products of every vertex's faces, in ascending face id."""
        degf = np.diff(self.vf_off)
        n = np.zeros((self.V, 3))
        for j in range(int(degf.max()) if self.V else 0):
            vs = np.nonzero(degf > j)[0]
            n[vs] = n[vs] + self.fn[self.vf_faces[self.vf_off[vs] + j]]
        return n

    def has_edge(self, x, y):
        k = np.minimum(x, y) * self.V + np.maximum(x, y)
        pos = np.minimum(np.searchsorted(self.ekeys, k), max(self.E - 1, 0))
        return (self.ekeys[pos] == k) & (x != y)

    def valence_dev(self):
        d = self.valence - np.where(self.vclass & BOUNDARY, 4, 6)
        return int((d * d)[self.valence > 0].sum())


# ------------------------------------------------------------------------------------------------------------------- split
def split_marks(v, f, sel, hi2, edges, c2e):
    p = v.astype(np.float64)
    d = p[edges[:, 1]] - p[edges[:, 0]]
    split = _dot(d, d) > hi2
    split[c2e[sel == 0].reshape(-1)] = False
    return split


def split_round(v, f, sel, src, hi2):
    """-> (v, f, sel, src, number of new vertices)."""
    V, F = v.shape[0], f.shape[0]
    edges, _, c2e = R.edges_of(f, V)
    split = split_marks(v, f, sel, hi2, edges, c2e)
    n_new = int(split.sum())
    if n_new == 0:
        return v, f, sel, src, 0
    p = v.astype(np.float64)
    mid_id = np.full(edges.shape[0], -1)
    mid_id[split] = V + np.arange(n_new)
    v = np.concatenate([v, ((p[edges[split, 0]] + p[edges[split, 1]]) * 0.5).astype(np.float32)])
    p = v.astype(np.float64)
    m = mid_id[c2e]
    pat = (m[:, 0] >= 0) * 1 + (m[:, 1] >= 0) * 2 + (m[:, 2] >= 0) * 4
    ch = np.full((F, 4, 3), -1)
    g = pat == 0
    ch[g, 0] = f[g]
    g = pat == 7
    t, mm = f[g], m[g]
    ch[g, 0] = np.stack([t[:, 0], mm[:, 0], mm[:, 2]], 1)
    ch[g, 1] = np.stack([t[:, 1], mm[:, 1], mm[:, 0]], 1)
    ch[g, 2] = np.stack([t[:, 2], mm[:, 2], mm[:, 1]], 1)
    ch[g, 3] = mm
    for k, one, two in ((0, 1, 6), (1, 2, 5), (2, 4, 3)):
        g = pat == one                                           # only edge k split
        vk, vk1, vk2, mk = f[g, k], f[g, (k + 1) % 3], f[g, (k + 2) % 3], m[g, k]
        ch[g, 0] = np.stack([vk, mk, vk2], 1)
        ch[g, 1] = np.stack([mk, vk1, vk2], 1)
        g = pat == two                                           # all but edge k split: the quad is cut by its shorter diagonal
        vk, vk1, vk2, m1, m2 = f[g, k], f[g, (k + 1) % 3], f[g, (k + 2) % 3], m[g, (k + 1) % 3], m[g, (k + 2) % 3]
        d1, d2 = p[m1] - p[vk], p[m2] - p[vk1]
        first = (_dot(d1, d1) <= _dot(d2, d2))[:, None]
        ch[g, 0] = np.stack([m1, vk2, m2], 1)
        ch[g, 1] = np.where(first, np.stack([vk, vk1, m1], 1), np.stack([vk, vk1, m2], 1))
        ch[g, 2] = np.where(first, np.stack([vk, m1, m2], 1), np.stack([vk1, m1, m2], 1))
    keep = ch[:, :, 0] >= 0
    cnt = keep.sum(1)
    return v, ch[keep], np.repeat(sel, cnt), np.repeat(src, cnt), n_new


# ------------------------------------------------------------------------------------------------------------------- collapse
def collapse_keys(v, f, sel, lo2, hi2, cos_f, topo=None):
    """-> (keys [E] u64, NO_KEY where the edge is not shorter than lo or its collapse is not valid; placement f32 [E, 3]; topo)."""
    t = topo or Topo(v, f, sel, cos_f)
    p, E = t.p, t.E
    a, b = t.edges[:, 0], t.edges[:, 1]
    ab = p[b] - p[a]
    len2 = _dot(ab, ab)
    fa, fb = (t.vclass[a] & FEATURE) != 0, (t.vclass[b] & FEATURE) != 0
    ok = (len2 < lo2) & (t.nf <= 2) & (((t.vclass[a] | t.vclass[b]) & FROZEN) == 0) & ~(fa & fb & ~t.efeat)
    mid = ((p[a] + p[b]) * 0.5).astype(np.float32).astype(np.float64)
    P = np.where((fa == fb)[:, None], mid, np.where(fa[:, None], p[a], p[b]))
    cand = np.nonzero(ok)[0]
    # link condition: common neighbours == faces on the edge
    rows, pos = _expand(t.ve_off, a[cand])
    common = np.bincount(rows[t.has_edge(t.ve_other[pos], b[cand][rows])], minlength=len(cand))
    cand = cand[common == t.nf[cand]]
    vn = t.vertex_normals()
    for end in (a, b):
        # no surviving face around the endpoint turns against its old normal or against the endpoint's old vertex normal
        rows, pos = _expand(t.vf_off, end[cand])
        tri = f[t.vf_faces[pos]]
        ea, eb = a[cand][rows][:, None], b[cand][rows][:, None]
        dies = (tri == ea).any(1) & (tri == eb).any(1)
        moved = (tri == ea) | (tri == eb)
        W = [np.where(moved[:, k:k + 1], P[cand][rows], p[tri[:, k]]) for k in range(3)]
        n1 = _cross(W[1] - W[0], W[2] - W[0])
        bad = ~dies & ~((_dot(n1, t.fn[t.vf_faces[pos]]) > 0) & (_dot(n1, vn[end[cand]][rows]) > 0))
        # no edge from the new position to a neighbour becomes longer than hi
        rows2, pos2 = _expand(t.ve_off, end[cand])
        w = t.ve_other[pos2]
        d = p[w] - P[cand][rows2]
        long_ = (w != a[cand][rows2]) & (w != b[cand][rows2]) & (_dot(d, d) > hi2)
        drop = np.zeros(len(cand), bool)
        drop[rows[bad]] = True
        drop[rows2[long_]] = True
        cand = cand[~drop]
    keys = np.full(E, NO_KEY)
    keys[cand] = (len2[cand].astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | mix_id(cand.astype(np.uint32)).astype(np.uint64)
    return keys, P.astype(np.float32), t


def collapse_round(v, f, sel, src, lo2, hi2, cos_f):
    """-> (f, sel, src, number of collapses); v is updated in place."""
    keys, P, t = collapse_keys(v, f, sel, lo2, hi2, cos_f)
    a, b = t.edges[:, 0], t.edges[:, 1]
    m1 = np.full(t.V, NO_KEY)
    np.minimum.at(m1, a, keys)
    np.minimum.at(m1, b, keys)
    m2 = m1.copy()
    np.minimum.at(m2, a, m1[b])
    np.minimum.at(m2, b, m1[a])
    idx = np.nonzero((keys != NO_KEY) & (keys == m2[a]) & (keys == m2[b]))[0]
    if idx.size == 0:
        return f, sel, src, 0
    v[a[idx]] = P[idx]
    dest = np.arange(t.V)
    dest[b[idx]] = a[idx]
    f = dest[f]
    alive = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    return f[alive], sel[alive], src[alive], idx.size


# ------------------------------------------------------------------------------------------------------------------- flip
def flip_round(v, f, sel, src, cos_f):
    """-> (number of flips, valence deviation before the round); f and src are updated in place."""
    t = Topo(v, f, sel, cos_f)
    p = t.p
    e = np.nonzero((t.nf == 2) & ~t.efeat)[0]
    c0, c1 = t.ecorn[t.eoff[e]], t.ecorn[t.eoff[e] + 1]
    f0, k0, f1, k1 = c0 // 3, c0 % 3, c1 // 3, c1 % 3
    x, y, c = f[f0, k0], f[f0, (k0 + 1) % 3], f[f0, (k0 + 2) % 3]
    d = f[f1, (k1 + 2) % 3]
    ok = (sel[f0] != 0) & (sel[f1] != 0) & (f[f1, k1] == y) & (f[f1, (k1 + 1) % 3] == x) & (c != d) & ~t.has_edge(c, d)
    tgt = np.where(t.vclass & BOUNDARY, 4, 6)

    def dev(w, delta):
        q = t.valence[w] + delta - tgt[w]
        return q * q
    gain = dev(x, 0) + dev(y, 0) + dev(c, 0) + dev(d, 0) - dev(x, -1) - dev(y, -1) - dev(c, 1) - dev(d, 1)
    ok &= gain > 0
    n0, n1 = _cross(p[y] - p[x], p[c] - p[x]), _cross(p[x] - p[y], p[d] - p[y])
    g0, g1 = _cross(p[x] - p[c], p[d] - p[c]), _cross(p[y] - p[d], p[c] - p[d])
    ok &= (_dot(g0, n0) > 0) & (_dot(g0, n1) > 0) & (_dot(g1, n0) > 0) & (_dot(g1, n1) > 0)
    e, x, y, c, d, f0, f1, gain = (z[ok] for z in (e, x, y, c, d, f0, f1, gain))
    keys = ((MAX_GAIN - np.minimum(gain, MAX_GAIN)).astype(np.uint64) << np.uint64(32)) | mix_id(e.astype(np.uint32)).astype(np.uint64)
    m1 = np.full(t.V, NO_KEY)
    for w in (x, y, c, d):
        np.minimum.at(m1, w, keys)
    pick = (keys == m1[x]) & (keys == m1[y]) & (keys == m1[c]) & (keys == m1[d])
    x, y, c, d, f0, f1 = (z[pick] for z in (x, y, c, d, f0, f1))
    f[f0] = np.stack([c, x, d], 1)
    f[f1] = np.stack([d, y, c], 1)
    s = np.minimum(src[f0], src[f1])
    src[f0] = s
    src[f1] = s
    return int(pick.sum()), t.valence_dev()


# ------------------------------------------------------------------------------------------------------------------- relax
def closest_on_triangle(p, a, b, c):
    """Closest point of the triangles (a, b, c) to the points p, by Voronoi region: a, b, edge ab, c, edge ac, edge bc, inside."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        s = (va + vb) + vc
        col = lambda z: z[:, None]   # noqa: E731
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        vals = [a, b, a + ab * col(d1 / (d1 - d3)), c, a + ac * col(d2 / (d2 - d6)), b + (c - b) * col((d4 - d3) / ((d4 - d3) + (d5 - d6)))]
        out = (a + ab * col(vb / s)) + ac * col(vc / s)
        for cond, val in zip(conds[::-1], vals[::-1]):
            out = np.where(col(cond), val, out)
    return out


def relax(v, f, sel, cos_f):
    """-> (new vertices f32, number of vertices put back)."""
    t = Topo(v, f, sel, cos_f)
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
        c = closest_on_triangle(r[vs], p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]])
        d = c - r[vs]
        dd = _dot(d, d)
        up = dd < best[vs]
        best[vs[up]] = dd[up]
        hit[vs[up]] = c[up]
    moved = movable & (best < np.inf)
    out = v.copy()
    out[moved] = hit[moved].astype(np.float32)
    reverted = 0
    while True:
        touched = moved[f].any(1)
        g = _normals(out.astype(np.float64), f)
        ok = _dot(g, t.fn) > 0
        for k in range(3):                                       # and with the old vertex normal of every corner that moved
            ok &= ~moved[f[:, k]] | (_dot(g, n[f[:, k]]) > 0)
        bad = touched & ~ok
        back = np.zeros(V, bool)
        back[f[bad].reshape(-1)] = True
        back &= moved
        if not back.any():
            return out, reverted
        out[back] = v[back]
        moved &= ~back
        reverted += int(back.sum())


# ------------------------------------------------------------------------------------------------------------------- the operator
def remesh_isotropic(v, faces, target_len, iterations=3, selected=None, feature_deg=30.0, stats=None, hook=None):
    """-> (v, f, face_src) like nerf2mesh_amd.mesh_remesh.remesh_isotropic.  hook(stage, iteration, v, f, sel), stage in "split",
    "collapse", "flip", "relax", is called after every pass."""
    v = np.asarray(v, np.float32).copy()
    f = np.asarray(faces, np.int64).copy()
    F = f.shape[0]
    sel = np.ones(F, np.uint8) if selected is None else (np.asarray(selected) != 0).astype(np.uint8)
    src = np.arange(F)
    if stats is not None:
        stats["iterations"] = []
    if iterations == 0 or F == 0 or sel.sum() == 0:
        return v, f.astype(np.int32), src
    lo2, hi2 = thresholds(target_len)
    cos_f = cos_feature(feature_deg)
    for it in range(iterations):
        if f.shape[0] == 0:
            break
        n_split = MAX_SPLIT_ROUNDS
        for r in range(MAX_SPLIT_ROUNDS):
            v, f, sel, src, n = split_round(v, f, sel, src, hi2)
            if n == 0:
                n_split = r
                break
        if hook:
            hook("split", it, v, f, sel)
        n_collapse = MAX_COLLAPSE_ROUNDS
        for r in range(MAX_COLLAPSE_ROUNDS):
            f, sel, src, n = collapse_round(v, f, sel, src, lo2, hi2, cos_f)
            if n == 0:
                n_collapse = r
                break
        if hook:
            hook("collapse", it, v, f, sel)
        n_flip, devs = MAX_FLIP_ROUNDS, []
        for r in range(MAX_FLIP_ROUNDS):
            n, dev = flip_round(v, f, sel, src, cos_f)
            devs.append(dev)
            if n == 0:
                n_flip = r
                break
        else:
            devs.append(Topo(v, f, sel, cos_f).valence_dev())
        if hook:
            hook("flip", it, v, f, sel)
        v, n_revert = relax(v, f, sel, cos_f)
        if hook:
            hook("relax", it, v, f, sel)
        if stats is not None:
            stats["iterations"].append({"split_rounds": n_split, "collapse_rounds": n_collapse, "flip_rounds": n_flip, "relax_reverts": n_revert,
                                        "faces": int(f.shape[0]), "valence_dev": devs})
    ref = np.zeros(v.shape[0], bool)
    ref[f.reshape(-1)] = True
    new_id = np.cumsum(ref) - 1
    return v[ref], new_id[f].astype(np.int32), src


def refine(v, f, mask, decimate_ratio=0.1, remesh_size=0.02, refine_size=0.01):
    """decimate_and_refine_mesh (meshutils.py:191-231) with the re-meshing: selected decimation of class 1, isotropic re-meshing of class
    1, selected subdivision of class 2, the classes carried through the face sources.  -> (v, f, faces after the decimation, after the
    re-meshing)."""
    mask = np.asarray(mask, np.uint8)
    if decimate_ratio > 0 and (mask == 1).any():
        v, f, src = R.decimate(v, f, int((1 - decimate_ratio) * int((mask == 1).sum())), optimal_placement=True, selected=(mask == 1))
        mask = mask[src]
    n_before = len(f)
    if remesh_size > 0 and (mask == 1).any():
        v, f, src = remesh_isotropic(v, f, remesh_size, iterations=3, selected=(mask == 1))
        mask = mask[src]
    n_after = len(f)
    if refine_size > 0 and (mask == 2).any():
        v, f = R.subdivide_midpoint(v, f, refine_size, selected=(mask == 2))
    return v, f, n_before, n_after
