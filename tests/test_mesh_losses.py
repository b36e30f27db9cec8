"""CPU: trainer.MeshEdgeTerms -- the topology of the normal-consistency and edge-length losses (nerf/utils.py:759-769, pytorch3d's
mesh_normal_consistency / mesh_edge_loss) against a brute-force enumeration, and its torch form against the definitions written out in
tests/mesh_loss_case.py (float64, and torch.cosine_similarity).  The HIP kernels are tested in tests/test_mesh_losses_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_loss_case as MC   # noqa: E402

from nerf2mesh_amd.trainer import MeshEdgeTerms   # noqa: E402


def terms(v, f):
    return MeshEdgeTerms(torch.from_numpy(f), v.shape[0])


COUNTS = {"tetrahedron": (4, 4, 6, 6), "triangle": (3, 1, 3, 0), "book": (5, 3, 7, 3), "grid": (441, 800, 1240, 1160),
          "two cascades": (441 + 81, 800 + 128, 1240 + 208, 1160 + 176)}


@pytest.mark.parametrize("name", list(MC.cases()))
def test_topology_equals_the_brute_force_enumeration(name):
    """edges, pairs (as records, in order) and both CSRs: every (term, corner) a vertex takes part in, once, ascending within its row."""
    v, f, _ = MC.cases()[name]
    t = terms(v, f)
    edges, pairs = MC.brute_topology(f)
    V = v.shape[0]
    if name in COUNTS:
        assert (V, f.shape[0], t.n_edges, t.n_pairs) == COUNTS[name]
    assert t.edges.dtype == t.pairs.dtype == t.pair_ref.dtype == t.edge_ptr.dtype == torch.int32
    assert t.edges.shape == (len(edges), 2) and np.array_equal(t.edges.numpy(), edges)
    assert t.pairs.shape == (len(pairs), 4) and np.array_equal(t.pairs.numpy(), pairs)
    assert bool((t.edges[:, 0] < t.edges[:, 1]).all()) and (len(pairs) == 0 or bool((t.pairs[:, 0] < t.pairs[:, 1]).all()))
    for table, ptr, ref in ((t.pairs, t.pair_ptr, t.pair_ref), (t.edges, t.edge_ptr, t.edge_ref)):
        flat, ptr, ref = table.reshape(-1).numpy(), ptr.numpy(), ref.numpy()
        assert ptr.shape == (V + 1,) and ptr[0] == 0 and ptr[-1] == flat.size == ref.size
        assert sorted(ref.tolist()) == list(range(flat.size))                      # every corner of every term exactly once
        for i in range(V):
            row = ref[ptr[i]:ptr[i + 1]]
            assert np.all(flat[row] == i) and np.all(np.diff(row) > 0)


def test_empty_mesh_and_two_cascades_are_one_mesh():
    t = MeshEdgeTerms(torch.zeros(0, 3, dtype=torch.int32), 5)
    assert t.n_edges == t.n_pairs == 0 and t.pairs.shape == (0, 4) and t.pair_ptr.tolist() == [0] * 6
    x = torch.rand(5, 3, requires_grad=True)
    assert float(t(x).detach()) == 0.0
    # the concatenation is ONE mesh: one mean over all pairs / edges, not a mean of the parts' means
    a, b = MC.grid(noise=0.02, seed=4), MC.grid(9, noise=0.05, seed=5)
    v, f = MC.concat(a, b)
    ta, tb, tc = terms(*a), terms(*b), terms(v, f)
    va, vb, vc = torch.from_numpy(a[0]).double(), torch.from_numpy(b[0]).double(), torch.from_numpy(v).double()
    want_n = (ta.normal_consistency(va) * ta.n_pairs + tb.normal_consistency(vb) * tb.n_pairs) / (ta.n_pairs + tb.n_pairs)
    want_e = (ta.edge_length(va) * ta.n_edges + tb.edge_length(vb) * tb.n_edges) / (ta.n_edges + tb.n_edges)
    assert abs(float(tc.normal_consistency(vc)) - float(want_n)) < 1e-14 and abs(float(tc.edge_length(vc)) - float(want_e)) < 1e-14


def test_single_triangle_has_no_pair_and_a_normal_loss_of_exactly_zero():
    v, f = MC.triangle()
    t = terms(v, f)
    x = torch.from_numpy(v).requires_grad_()
    n = t.normal_consistency(x)
    assert float(n.detach()) == 0.0
    n.backward()
    assert float(x.grad.abs().max()) == 0.0
    assert float(t(x, 1.0, 0.0).detach()) == 0.0


@pytest.mark.parametrize("name", list(MC.cases()))
def test_torch_form_in_float64_equals_the_definitions(name):
    """Value and gradient of the torch form against the definitions written out independently (tests/mesh_loss_case.py); the cosine also
    against torch.cosine_similarity."""
    v, f, settings = MC.cases()[name]
    t = terms(v, f)
    edges, pairs = MC.brute_topology(f)
    for lam_n, lam_e in settings:
        x = torch.from_numpy(v).double().requires_grad_()
        got = t(x, lam_n, lam_e)
        (got * MC.UPSTREAM).backward()
        ref_val, ref_grad = MC.yardstick(name)[(lam_n, lam_e)]
        assert abs(float(got.detach()) - ref_val) <= 1e-14 * max(1.0, abs(ref_val))
        assert float((x.grad - ref_grad).abs().max()) <= 1e-12 * max(float(ref_grad.abs().max()), 1e-300)
    if len(pairs):
        x = torch.from_numpy(v).double()
        v0, v1, a, b = (x[torch.as_tensor(pairs[:, k])] for k in range(4))
        n0, n1 = torch.linalg.cross(v1 - v0, a - v0), -torch.linalg.cross(v1 - v0, b - v0)
        want = (1 - torch.cosine_similarity(n0, n1, dim=1)).mean()
        assert abs(float(t.normal_consistency(x)) - float(want)) <= 1e-14


def test_value_does_not_depend_on_the_winding():
    """v0 < v1 come from the sorted edge, not from a face's winding: flipping a random half of the faces leaves the value EQUAL."""
    for noise, seed in ((0.0, 0), (0.05, 6)):
        v, f = MC.grid(noise=noise, seed=seed)
        flip = np.random.default_rng(7).random(f.shape[0]) < 0.5
        assert 300 < flip.sum() < 500
        g = f.copy()
        g[flip] = g[flip][:, [0, 2, 1]]
        for dtype in (torch.float32, torch.float64):
            x = torch.from_numpy(v).to(dtype)
            a, b = terms(v, f), terms(v, g)
            assert float(a.normal_consistency(x)) == float(b.normal_consistency(x))
            assert float(a.edge_length(x)) == float(b.edge_length(x))


def test_zero_area_face_value_and_finite_gradient():
    """A pair with a collinear face: n1 = 0, its clamped cosine is 0 and the term 1; the gradient follows the clamped expression (of order 1e8)
    and is finite -- in the torch form in both precisions."""
    v, f = MC.zero_area()
    t = terms(v, f)
    edges, pairs = MC.brute_topology(f)
    assert t.n_pairs == 1
    for dtype in (torch.float64, torch.float32):
        x = torch.from_numpy(v).to(dtype).requires_grad_()
        got = t.normal_consistency(x)
        y = torch.from_numpy(v).to(dtype).requires_grad_()
        want, _ = MC.defined_losses(y, edges, pairs)
        assert float(got.detach()) == float(want.detach()) == 1.0
        got.backward()
        assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 1e6


def test_float32_torch_form_within_the_bound_the_kernels_get():
    """Measures the distance of the float32 torch form to the float64 yardstick on every case (the figures tests/mesh_loss_case.py records) and
    holds it to the bound the kernels get: 8 x the recorded largest distance."""
    worst_v, worst_g = (-1.0, ()), (-1.0, ())
    for name, (v, f, settings) in MC.cases().items():
        t = terms(v, f)
        for w in settings:
            x = torch.from_numpy(v).requires_grad_()
            val = t(x, *w)
            (val * MC.UPSTREAM).backward()
            dv, dg = MC.distances(name, w, val, x.grad)
            print(f"{name:18s} weights {w}: value {float(val.detach()):.6g}  |diff| {dv:.3g}   gradient diff / max {dg:.3g}")
            worst_v, worst_g = max(worst_v, (dv, (name, w))), max(worst_g, (dg, (name, w)))
            assert dv <= MC.VALUE_BOUND and dg <= MC.GRAD_BOUND, (name, w, dv, dg)
    print(f"largest: value {worst_v}, gradient {worst_g}; recorded {MC.FP32_VALUE_DIST:.3g}, {MC.FP32_GRAD_DIST:.3g}")
