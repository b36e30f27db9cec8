"""Sequential numpy restatement of the device UV atlas (nerf2mesh_amd/uv_atlas.py, csrc/uvatlas.hip; rule in DESIGN.md section 4.13).

Written from the rule: every index-deciding value is computed in the operand order and precision DESIGN 4.13 fixes (fp64 of the fp32
inputs, one rounding per operation, no fused multiply-add), so the device result must equal this one bit for bit.  The faces are visited
one after the other for the relaxation and for the two canvas passes; charts come from scipy's connected components, re-numbered by
their smallest face.  A few thousand faces run in seconds.  No GPU and no torch needed."""
import math

import numpy as np

PACK_SHRINK = 0.96        # the scale search: s_i = s_0 * PACK_SHRINK ** i
MAX_PACK_TRIALS = 256
MAX_EVICT_ROUNDS = 64
SUM_LANES = 256           # fixed_sum: partial t adds the elements t, t + 256, ... in order; the partials are then added in order
RECT_CLAMP = 1 << 30      # ceil(s * extent) is clamped here before it becomes an integer
STAT_KEYS = ("charts", "uv_vertices", "relax_changed", "evict_rounds", "evicted_faces", "pack_trials", "pack_scales", "scale",
             "utilisation", "density_min", "density_max")


def fixed_sum(a):
    """The fp64 sum in the one order the device uses (np.cumsum adds strictly left to right)."""
    a = np.asarray(a, np.float64)
    part = np.zeros(SUM_LANES)
    for t in range(min(SUM_LANES, len(a))):
        part[t] = np.cumsum(a[t::SUM_LANES])[-1]
    return float(np.cumsum(part)[-1])


def face_frames(v, f):
    """(n [F, 3] fp64 = (b - a) x (c - a), da [F] fp64 = |n|) of the fp32 corners."""
    p = np.asarray(v, np.float32).astype(np.float64)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    u, w = b - a, c - a
    n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    da = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    return n, da


def dots(n):
    """n . d_k for the six directions k = 2 * axis + (sign < 0): [F, 6]."""
    return np.stack([n[:, 0], -n[:, 0], n[:, 1], -n[:, 1], n[:, 2], -n[:, 2]], 1)


def initial_labels(n):
    return np.argmax(dots(n), 1).astype(np.int32)           # the first maximum: ties to the lowest k


def edge_tables(f, V):
    """c2e [F, 3] (corner k -> the edge (v_k, v_k+1)), nf [E], emin / emax [E] (smallest / largest face on the edge)."""
    f = np.asarray(f, np.int64)
    a, b = f, np.roll(f, -1, 1)
    key = (np.minimum(a, b) * V + np.maximum(a, b)).reshape(-1)
    _, inv, nf = np.unique(key, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    face = np.repeat(np.arange(len(f)), 3)
    emin = np.full(len(nf), np.iinfo(np.int64).max)
    emax = np.full(len(nf), -1)
    np.minimum.at(emin, inv, face)
    np.maximum.at(emax, inv, face)
    return inv.reshape(-1, 3), nf, emin, emax


def edge_lengths(v, f):
    """[F, 3] fp64: |v_k+1 - v_k| = sqrt((dx * dx + dy * dy) + dz * dz)."""
    p = np.asarray(v, np.float32).astype(np.float64)
    d = p[np.roll(f, -1, 1)] - p[f]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def relax_round(label, n, da, c2e, nf, emin, emax, elen, min_cos):
    """One Jacobi round -> (new labels, faces that changed)."""
    new = label.copy()
    dk = dots(n)
    for f in range(len(label)):
        sums = [0.0] * 6
        for k in range(3):
            e = c2e[f, k]
            if nf[e] == 2:
                sums[label[emin[e] + emax[e] - f]] += elen[f, k]
        cand = int(np.argmax(sums))
        if sums[cand] > 0.0 and cand != label[f] and dk[f, cand] >= min_cos * da[f]:
            new[f] = cand
    return new, int((new != label).sum())


def charts_of(label, gen, c2e, nf, emin, emax):
    """chart [F]: components over the edges with exactly two faces of equal label and generation; ids ascend with the smallest face."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    F = len(label)
    two = nf == 2
    a, b = emin[two], emax[two]
    ok = (label[a] == label[b]) & (gen[a] == gen[b])
    a, b = a[ok], b[ok]
    _, comp = connected_components(coo_matrix((np.ones(len(a)), (a, b)), shape=(F, F)), directed=False)
    first = np.full(comp.max() + 1, F)
    np.minimum.at(first, comp, np.arange(F))
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[comp]


def uv_axes(k):
    """(u axis, v axis) of direction k: the pair that gives a face with n . d_k > 0 a positive UV area."""
    a = k // 2
    return ((a + 1) % 3, (a + 2) % 3) if k % 2 == 0 else ((a + 2) % 3, (a + 1) % 3)


def rect_sizes(s, lo, hi, gutter):
    """[C, 2] int64 (width, height) of the charts' rectangles at scale s."""
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    return np.minimum(np.ceil(s * ext), float(RECT_CLAMP)).astype(np.int64) + 1 + 2 * gutter


def shelf_pack(rect, height, width):
    """Shelves, left to right, in (height desc, width desc, id) order -> (fits, origin [C, 2] int64 (x, y), order)."""
    C = len(rect)
    order = np.lexsort((np.arange(C), -rect[:, 0], -rect[:, 1]))
    origin = np.zeros((C, 2), np.int64)
    x = y = shelf = 0
    fits = True
    for c in order:
        w, h = int(rect[c, 0]), int(rect[c, 1])
        if w > width:
            fits = False
        if x + w > width:
            y += shelf
            x = shelf = 0
        origin[c] = (x, y)
        x += w
        shelf = max(shelf, h)
    return fits and y + shelf <= height, origin, order


def texel_coords(vt, height, width):
    """UV vertices in texels, fp64 (exact products of the fp32 uv and the resolution)."""
    return np.stack([vt[:, 0].astype(np.float64) * float(width), vt[:, 1].astype(np.float64) * float(height)], 1)


def _edge_fn(ip, iq, P, Q, px, py):
    """Edge function of the directed edge P -> Q, evaluated from the endpoint with the smaller UV-vertex id (so that the two faces of an
    edge get values that are exact negatives of each other)."""
    if ip < iq:
        return (Q[0] - P[0]) * (py - P[1]) - (Q[1] - P[1]) * (px - P[0])
    return -((P[0] - Q[0]) * (py - Q[1]) - (P[1] - Q[1]) * (px - Q[0]))


def interior_texels(tri_ids, T, height, width):
    """(ys, xs) of the texels whose centre lies strictly inside the UV triangle with corner ids tri_ids (T: texel coordinates)."""
    A, B, C = (T[i] for i in tri_ids)
    xs_, ys_ = (A[0], B[0], C[0]), (A[1], B[1], C[1])
    x0, x1 = max(0, int(math.floor(min(xs_) - 0.5))), min(width - 1, int(math.ceil(max(xs_) - 0.5)))
    y0, y1 = max(0, int(math.floor(min(ys_) - 0.5))), min(height - 1, int(math.ceil(max(ys_) - 0.5)))
    if x1 < x0 or y1 < y0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    ys, xs = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
    px, py = xs + 0.5, ys + 0.5
    ia, ib, ic = (int(i) for i in tri_ids)
    inside = (_edge_fn(ia, ib, A, B, px, py) > 0) & (_edge_fn(ib, ic, B, C, px, py) > 0) & (_edge_fn(ic, ia, C, A, px, py) > 0)
    return ys[inside], xs[inside]


def evictions(ft, vt, height, width):
    """evicted [F] bool: some texel strictly inside the face is also strictly inside a face of lower id."""
    T = texel_coords(vt, height, width)
    canvas = np.full((height, width), np.iinfo(np.int32).max, np.int64)
    inner = [interior_texels(ft[f], T, height, width) for f in range(len(ft))]
    for f, (ys, xs) in enumerate(inner):
        np.minimum.at(canvas, (ys, xs), f)
    return np.array([bool((canvas[ys, xs] < f).any()) for f, (ys, xs) in enumerate(inner)], bool)


def face_metrics(ft, vt, da, height, width):
    """(texel area [F] fp64 (signed), density [F] = texel area / surface area)."""
    T = texel_coords(vt, height, width)
    A, B, C = T[ft[:, 0]], T[ft[:, 1]], T[ft[:, 2]]
    area = 0.5 * ((B[:, 0] - A[:, 0]) * (C[:, 1] - A[:, 1]) - (C[:, 0] - A[:, 0]) * (B[:, 1] - A[:, 1]))
    return area, area / (0.5 * da)


def check_args(vertices, triangles, height, width, gutter, relax_rounds, min_cos):
    v, f = np.asarray(vertices), np.asarray(triangles)
    if v.ndim != 2 or v.shape[1] != 3 or v.dtype != np.float32 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("uv_atlas: vertices must be float32 [V, 3], triangles [F, 3]")
    if not (int(height) >= 1 and int(width) >= 1 and int(gutter) >= 0 and int(relax_rounds) >= 0 and 0.0 < float(min_cos) <= 1.0):
        raise ValueError("uv_atlas: height, width >= 1, gutter >= 0, relax_rounds >= 0 and 0 < min_cos <= 1 are required")
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("uv_atlas: triangle indices out of range")


def uv_atlas(vertices, triangles, height, width, gutter=2, relax_rounds=4, min_cos=0.5, stats=None):
    """The rule of DESIGN 4.13 -> (vt [T, 2] float32, ft [F, 3] int32, vmapping [T] int32)."""
    check_args(vertices, triangles, height, width, gutter, relax_rounds, min_cos)
    v, f = np.asarray(vertices, np.float32), np.asarray(triangles, np.int64)
    V, F = len(v), len(f)
    height, width, gutter, min_cos = int(height), int(width), int(gutter), float(min_cos)
    st = {"charts": 0, "uv_vertices": 0, "relax_changed": [], "evict_rounds": 0, "evicted_faces": 0, "pack_trials": 0, "pack_scales": [],
          "scale": 0.0, "utilisation": 0.0, "density_min": 0.0, "density_max": 0.0}
    if F == 0:
        if stats is not None:
            stats.update(st)
        return np.zeros((0, 2), np.float32), np.zeros((0, 3), np.int32), np.zeros(0, np.int32)
    # 1 + 2: frames, initial labels
    n, da = face_frames(v, f)
    if ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0]) | (da == 0.0)).any():
        raise ValueError("uv_atlas: faces with a repeated corner or zero area (run clean_mesh first)")
    label = initial_labels(n)
    c2e, nf, emin, emax = edge_tables(f, V)
    # 3: relaxation
    elen = edge_lengths(v, f)
    for _ in range(int(relax_rounds)):
        label, changed = relax_round(label, n, da, c2e, nf, emin, emax, elen, min_cos)
        st["relax_changed"].append(changed)
    parea = 0.5 * np.abs(n[np.arange(F), label // 2])
    s0 = math.sqrt(float(height * width) / fixed_sum(parea))
    gen = np.zeros(F, np.int32)
    for rnd in range(MAX_EVICT_ROUNDS + 1):
        # 4: charts
        chart = charts_of(label, gen, c2e, nf, emin, emax)
        C = int(chart.max()) + 1
        clabel = np.zeros(C, np.int32)
        clabel[chart] = label
        # 5: UV vertices and their projections
        uk, inv = np.unique((chart[:, None] * V + f).reshape(-1), return_inverse=True)
        ft = inv.reshape(-1, 3).astype(np.int32)
        vmapping, vchart = (uk % V).astype(np.int32), uk // V
        axes = np.array([uv_axes(k) for k in range(6)])[clabel[vchart]]
        p = np.stack([v[vmapping, axes[:, 0]], v[vmapping, axes[:, 1]]], 1)                  # fp32 [T, 2]
        # 6: boxes, scale search, shelves
        lo, hi = np.full((C, 2), np.inf, np.float32), np.full((C, 2), -np.inf, np.float32)
        np.minimum.at(lo, vchart, p)
        np.maximum.at(hi, vchart, p)
        if C * (2 + 2 * gutter) ** 2 > height * width:
            raise RuntimeError(f"uv_atlas: {C} charts do not fit in {height} x {width} texels")
        scales = []
        for i in range(MAX_PACK_TRIALS):
            s = s0 * PACK_SHRINK ** i
            scales.append(s)
            st["pack_trials"] += 1
            fits, origin, _ = shelf_pack(rect_sizes(s, lo, hi, gutter), height, width)
            if fits:
                break
        else:
            raise RuntimeError(f"uv_atlas: {C} charts do not fit in {height} x {width} texels")
        st["pack_scales"] = scales
        d = p.astype(np.float64) - lo[vchart].astype(np.float64)
        o = origin[vchart].astype(np.float64)
        vt = np.stack([((o[:, 0] + gutter + 0.5) + s * d[:, 0]) / float(width), ((o[:, 1] + gutter + 0.5) + s * d[:, 1]) / float(height)],
                      1).astype(np.float32)
        # 7: overlaps
        ev = evictions(ft, vt, height, width)
        if not ev.any():
            break
        if rnd == MAX_EVICT_ROUNDS:
            raise RuntimeError("uv_atlas: the overlap evictions did not end")
        st["evict_rounds"] += 1
        st["evicted_faces"] += int(ev.sum())
        gen[ev] += 1
    area, density = face_metrics(ft, vt, da, height, width)
    st.update(charts=C, uv_vertices=len(uk), scale=s, utilisation=fixed_sum(area) / float(height * width),
              density_min=float(density.min()), density_max=float(density.max()))
    if stats is not None:
        stats.update(st)
        stats["chart"] = chart.astype(np.int32)
        stats["label"] = label
    return vt, ft, vmapping


# ------------------------------------------------------------------------------------------------ hand-built meshes
def cube(lo=-0.5, hi=0.5):
    """12 faces, outward normals."""
    v = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], np.float32)           # id = 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]          # -x +x -y +y -z +z
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, f


def subdivide(v, f):
    """Midpoint subdivision, 1 -> 4."""
    v = [tuple(p) for p in np.asarray(v, np.float32)]
    mid, out = {}, []

    def m(a, b):
        k = (min(a, b), max(a, b))
        if k not in mid:
            mid[k] = len(v)
            v.append(tuple((np.float32(v[a][i]) + np.float32(v[b][i])) * np.float32(0.5) for i in range(3)))
        return mid[k]
    for a, b, c in np.asarray(f):
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    return np.array(v, np.float32), np.array(out, np.int32)


def grid_sheet(nx, ny, origin, du, dv):
    """(nx x ny) quads spanned by du, dv from origin, two faces each; the normal is du x dv."""
    o, du, dv = (np.asarray(x, np.float64) for x in (origin, du, dv))
    v = np.array([o + i * du + j * dv for j in range(ny + 1) for i in range(nx + 1)], np.float32)
    f = []
    for j in range(ny):
        for i in range(nx):
            a = j * (nx + 1) + i
            b, c, d = a + 1, a + nx + 2, a + nx + 1
            f += [(a, b, c), (a, c, d)]
    return v, np.array(f, np.int32)


def merge_meshes(parts, decimals=6):
    """Concatenation with coincident vertices (rounded to `decimals`) welded."""
    vs, fs, seen = [], [], {}
    for v, f in parts:
        ids = []
        for p in v:
            k = tuple(np.round(p.astype(np.float64), decimals) + 0.0)
            if k not in seen:
                seen[k] = len(vs)
                vs.append(p)
            ids.append(seen[k])
        fs.append(np.asarray(ids)[f])
    return np.array(vs, np.float32), np.concatenate(fs).astype(np.int32)


def uneven_box(res=(1, 1, 2, 2, 24, 24)):
    """The unit box with its six sides (-x +x -y +y -z +z) tessellated res[k] x res[k]: very different face areas."""
    sides = [((0, 0, 0), (0, 0, 1), (0, 1, 0)), ((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((0, 0, 0), (1, 0, 0), (0, 0, 1)),
             ((0, 1, 0), (0, 0, 1), (1, 0, 0)), ((0, 0, 0), (0, 1, 0), (1, 0, 0)), ((0, 0, 1), (1, 0, 0), (0, 1, 0))]
    parts = []
    for (o, du, dv), r in zip(sides, res):
        parts.append(grid_sheet(r, r, o, np.asarray(du) / r, np.asarray(dv) / r))
    return merge_meshes(parts)


def helical_ramp(turns=2, steps=24, r0=0.4, r1=0.9, rise=0.5):
    """A ramp winding `turns` times round the z axis, every face looking up (+z): one chart whose turns overlap in projection."""
    n = turns * steps
    v = []
    for i in range(n + 1):
        a = 2.0 * math.pi * i / steps
        z = rise * i / steps
        v += [(r0 * math.cos(a), r0 * math.sin(a), z), (r1 * math.cos(a), r1 * math.sin(a), z)]
    f = []
    for i in range(n):
        a, b, c, d = 2 * i, 2 * i + 1, 2 * i + 3, 2 * i + 2                  # inner_i, outer_i, outer_i+1, inner_i+1
        f += [(a, b, c), (a, c, d)]
    return np.array(v, np.float32), np.array(f, np.int32)


def overlap_pairs(vt, ft, height, width):
    """Independent check: the number of texels whose centre is strictly inside more than one face (plain counting, no minimum)."""
    T = texel_coords(vt, height, width)
    count = np.zeros((height, width), np.int64)
    for f in range(len(ft)):
        ys, xs = interior_texels(ft[f], T, height, width)
        count[ys, xs] += 1
    return int((count > 1).sum())
