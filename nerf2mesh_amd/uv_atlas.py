"""UV atlas on the device (include/n2m_hip.h, csrc/uvatlas.hip): the step the reference leaves to xatlas on the host
(nerf/renderer.py:312-322).  Not an xatlas port: axis-direction charts, orthographic parametrisation at one global scale, shelf packing and
overlap eviction, with guarantees export.grid_atlas lacks -- charts instead of single faces, a texel density within
[min(min_cos, 0.577), 1] * scale^2 of every face's surface area, no texel centre strictly inside two faces.

The per-element work (face frames, labels, relaxation rounds, the filtered union-find, projection and chart boxes, rectangles, the shelf
recurrence, the uv write, the overlap canvas, the per-face metrics) is HIP; unique-ing edges and (chart, vertex) pairs, the sort of the
rectangles and the scans are torch plumbing, as in mesh_clean.py.  The rule, and why it does not depend on thread timing: DESIGN.md section
4.13.  tests/uv_atlas_ref.py restates it sequentially in numpy.
"""
import math
import operator
import time

import torch

from . import _lib as L
from .mesh_clean import _check_input
from .mesh_simplify import _edges

_p = L.ptr

PACK_SHRINK = 0.96        # the scale search: s_i = s_0 * PACK_SHRINK ** i
MAX_PACK_TRIALS = 256
MAX_EVICT_ROUNDS = 64
STAT_KEYS = ("charts", "uv_vertices", "relax_changed", "evict_rounds", "evicted_faces", "pack_trials", "pack_scales", "scale",
             "utilisation", "density_min", "density_max")


def _fixed_sum(x, out, s):
    L.call("n2m_uv_sum_f64", _p(x), int(x.shape[0]), _p(out), s)
    return float(out.item())


def uv_atlas(vertices, triangles, height, width, gutter=2, relax_rounds=4, min_cos=0.5, stats=None):
    """Unwraps a clean triangle mesh into charts packed into a `height` x `width` texel image (the resolution the atlas will be rasterised
    at: the gutter and the overlap rule are in texels).

    vertices float32 [V, 3], triangles int32/int64 [F, 3], CUDA.  Returns (vt [T, 2] float32 in [0, 1], ft [F, 3] int32 -- row i is input
    face i --, vmapping [T] int32: the mesh vertex behind each UV vertex, xatlas's first return value).  In order:
    1. fp64 face normals;  2. every face is labelled with the axis direction closest to its normal;  3. `relax_rounds` Jacobi rounds let a
    face take the label that most of its shared edge length carries, if its normal keeps a cosine of at least `min_cos` to it;  4. charts are
    the edge-connected faces of equal label;  5. a chart is projected along its direction (one UV vertex per (chart, mesh vertex));  6. the
    charts' rectangles (`gutter` free texels on every side) are shelf-packed at the largest scale of s_0 * 0.96^i that fits;  7. faces that
    overlap a face of lower id in the packed atlas are evicted into charts of their own, and 4-7 repeat until nothing overlaps.

    Faces of zero area or with a repeated corner are rejected (the atlas does not repair: run mesh_clean.clean_mesh first).
    stats: optional dict, filled with STAT_KEYS (`relax_changed`: faces re-labelled per round; `pack_trials`: over all eviction rounds;
    `pack_scales`: the scales tried in the last one; `scale`: texels per world unit; `utilisation`: UV triangle area as a share of the image;
    `density_min` / `density_max`: texel area / surface area over the faces).  A stats dict that comes in with a true "timings" entry gets
    it replaced by wall seconds per phase (labels_relax, and per round / trial: components, pack_trials, evict_rounds), at the price of a
    device synchronisation around each."""
    vertices, faces = _check_input("uv_atlas", vertices, triangles)
    try:
        height, width, gutter, relax_rounds = (operator.index(x) for x in (height, width, gutter, relax_rounds))
    except TypeError:
        raise ValueError("uv_atlas: height, width, gutter and relax_rounds must be integers") from None
    if not (height >= 1 and width >= 1 and height * width < 1 << 31):
        raise ValueError(f"uv_atlas: height and width must be >= 1 with height * width < 2^31, got {height}, {width}")
    if not 0 <= gutter < 1 << 20:
        raise ValueError(f"uv_atlas: gutter must lie in [0, 2^20), got {gutter}")
    if relax_rounds < 0:
        raise ValueError(f"uv_atlas: relax_rounds must be >= 0, got {relax_rounds}")
    min_cos = float(min_cos)
    if not 0.0 < min_cos <= 1.0:
        raise ValueError(f"uv_atlas: min_cos must lie in (0, 1], got {min_cos}")
    dev = vertices.device
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    st = {"charts": 0, "uv_vertices": 0, "relax_changed": [], "evict_rounds": 0, "evicted_faces": 0, "pack_trials": 0, "pack_scales": [],
          "scale": 0.0, "utilisation": 0.0, "density_min": 0.0, "density_max": 0.0}
    if F == 0:
        if stats is not None:
            stats.update(st)
        return (torch.zeros(0, 2, dtype=torch.float32, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev),
                torch.zeros(0, dtype=torch.int32, device=dev))
    timings = {"labels_relax": 0.0, "components": [], "pack_trials": [], "evict_rounds": []} if stats is not None and stats.get("timings") else None

    def tick():
        if timings is None:
            return 0.0
        torch.cuda.synchronize(dev)
        return time.perf_counter()
    with torch.cuda.device(dev):
        s = L.stream()
        t0 = tick()
        totals = torch.empty(1, dtype=torch.int64, device=dev)
        scalar = torch.empty(1, dtype=torch.float64, device=dev)
        # 1 + 2. frames, initial labels
        normal = torch.empty(F, 3, dtype=torch.float64, device=dev)
        da = torch.empty(F, dtype=torch.float64, device=dev)
        elen = torch.empty(F, 3, dtype=torch.float64, device=dev)
        label = torch.empty(F, dtype=torch.int32, device=dev)
        L.call("n2m_uv_face_frames", _p(vertices), _p(faces), F, _p(normal), _p(da), _p(elen), _p(label), _p(totals), s)
        bad = int(totals.item())
        if bad:
            raise ValueError(f"uv_atlas: {bad} faces have zero area or a repeated corner; the atlas does not repair -- run clean_mesh first")
        _, nf, c2e = _edges(faces, V)
        E = int(nf.shape[0])
        emin = torch.empty(E, dtype=torch.int32, device=dev)
        emax = torch.empty(E, dtype=torch.int32, device=dev)
        L.call("n2m_uv_edge_faces", _p(c2e), F, E, _p(emin), _p(emax), s)
        # 3. relaxation
        other = torch.empty_like(label)
        changed = torch.zeros(max(relax_rounds, 1), dtype=torch.int64, device=dev)
        for rnd in range(relax_rounds):
            L.call("n2m_uv_relax_round", F, _p(c2e), _p(nf), _p(emin), _p(emax), _p(elen), _p(normal), _p(da), min_cos, _p(label), _p(other),
                   changed[rnd:].data_ptr(), s)
            label, other = other, label
        st["relax_changed"] = changed[:relax_rounds].tolist()                     # one host read for all rounds
        parea = 0.5 * normal.gather(1, (label // 2).long()[:, None]).abs().reshape(-1).contiguous()
        s0 = math.sqrt(float(height * width) / _fixed_sum(parea, scalar, s))      # nothing larger can fit
        if timings is not None:
            timings["labels_relax"] = tick() - t0
        gen = torch.zeros(F, dtype=torch.int32, device=dev)
        parent = torch.empty(F, dtype=torch.int32, device=dev)
        root = torch.empty(F, dtype=torch.int32, device=dev)
        is_root = torch.empty(F, dtype=torch.uint8, device=dev)
        canvas = torch.empty(height, width, dtype=torch.int32, device=dev)
        evicted = torch.empty(F, dtype=torch.uint8, device=dev)
        result = torch.empty(2, dtype=torch.int32, device=dev)
        fl = faces.long()
        for rnd in range(MAX_EVICT_ROUNDS + 1):
            # 4. charts, numbered in the order of their smallest face
            t0 = tick()
            L.call("n2m_uv_charts", F, _p(c2e), _p(nf), _p(emin), _p(emax), _p(label), _p(gen), _p(parent), _p(root), _p(is_root), s)
            scan = torch.cumsum(is_root, 0, dtype=torch.int64)
            chart = scan[root.long()] - 1
            C = int(scan[-1])                                                      # the round's first host read
            if C * (2 + 2 * gutter) ** 2 > height * width:
                raise RuntimeError(f"uv_atlas: {C} charts do not fit in {height} x {width} texels")
            chart_label = torch.empty(C, dtype=torch.int32, device=dev)
            chart_label[chart] = label                                             # (every face of a chart writes the same value)
            # 5. one UV vertex per (chart, mesh vertex), ordered by (chart, vertex)
            uk, inv = torch.unique((chart[:, None] * V + fl).reshape(-1), sorted=True, return_inverse=True)
            T = int(uk.shape[0])
            ft = inv.view(F, 3).to(torch.int32).contiguous()
            vmapping = (uk % V).to(torch.int32).contiguous()
            vchart = (uk // V).to(torch.int32).contiguous()
            proj = torch.empty(T, 2, dtype=torch.float32, device=dev)
            box = torch.empty(C, 4, dtype=torch.int32, device=dev)
            L.call("n2m_uv_project", _p(vertices), _p(vmapping), _p(vchart), _p(chart_label), T, C, _p(proj), _p(box), s)
            if timings is not None:
                timings["components"].append(tick() - t0)
            # 6. scale search: rectangles, sort, shelves; one scalar read per trial
            rect = torch.empty(C, 2, dtype=torch.int32, device=dev)
            key = torch.empty(C, dtype=torch.int64, device=dev)
            origin = torch.empty(C, 2, dtype=torch.int32, device=dev)
            scales = []
            for i in range(MAX_PACK_TRIALS):
                scale = s0 * PACK_SHRINK ** i
                scales.append(scale)
                st["pack_trials"] += 1
                t0 = tick()
                L.call("n2m_uv_rects", _p(box), C, scale, gutter, _p(rect), _p(key), s)
                order = torch.sort(key, stable=True).indices.to(torch.int32).contiguous()
                L.call("n2m_uv_shelf_pack", _p(rect), _p(order), C, height, width, _p(origin), _p(result), s)
                fits = int(result[0])
                if timings is not None:
                    timings["pack_trials"].append(tick() - t0)
                if fits:
                    break
            else:
                raise RuntimeError(f"uv_atlas: {C} charts do not fit in {height} x {width} texels")
            st["pack_scales"] = scales
            vt = torch.empty(T, 2, dtype=torch.float32, device=dev)
            L.call("n2m_uv_write_vt", _p(proj), _p(vchart), _p(box), _p(origin), T, scale, gutter, height, width, _p(vt), s)
            # 7. overlaps
            t0 = tick()
            L.call("n2m_uv_canvas_evict", _p(vt), _p(ft), F, height, width, _p(canvas), _p(evicted), s)
            n_ev = int(evicted.sum())                                              # the round's last host read
            if timings is not None:
                timings["evict_rounds"].append(tick() - t0)
            if n_ev == 0:
                break
            if rnd == MAX_EVICT_ROUNDS:
                raise RuntimeError("uv_atlas: the overlap evictions did not end")
            st["evict_rounds"] += 1
            st["evicted_faces"] += n_ev
            gen += evicted
        area = torch.empty(F, dtype=torch.float64, device=dev)
        density = torch.empty(F, dtype=torch.float64, device=dev)
        L.call("n2m_uv_face_metrics", _p(vt), _p(ft), _p(da), F, height, width, _p(area), _p(density), s)
        util = _fixed_sum(area, scalar, s) / float(height * width)
        dmin, dmax = torch.stack([density.amin(), density.amax()]).tolist()
        st.update(charts=C, uv_vertices=T, scale=scale, utilisation=util, density_min=dmin, density_max=dmax)
    if stats is not None:
        stats.update(st)
        if timings is not None:
            stats["timings"] = timings
        stats["chart"] = chart.to(torch.int32)
        stats["label"] = label
    return vt, ft, vmapping
