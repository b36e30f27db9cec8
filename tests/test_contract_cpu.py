"""renderer.contract / renderer.uncontract, the CPU torch statements (nerf/renderer.py:25-41), against float64 restatements of the two
formulas in numpy (tests/contract_case.py), and the options of the SDF recipe on an unbounded scene.  No GPU."""
import numpy as np
import torch

import contract_case as C

# Largest distance of the fp32 torch statement from the float64 restatement over the point sets of contract_case.py, in fp32 ulp of the
# float64 value (measured once, recorded in DESIGN 4.23): contract 1.74, uncontract 27.1 (its 2 * mag - mag * mag cancels towards
# mag = 2; the set ends at 2 - 2/64, the edge of a 64-point lattice).  The bounds are those values with a factor-2 margin.
CONTRACT_ULP = 2 * 1.74
UNCONTRACT_ULP = 2 * 27.1


def test_round_trip_in_float64():
    """uncontract(contract(x)) == x: the restatements are inverses of each other.  float64 carries 1.1e-16; the inverse divides by
    mag * (2 - mag) with 2 - mag down to 1e-4 (mag = 1e4 before the contraction), which costs four digits: 1e-10 of the row's magnitude."""
    x = C.contract_points().astype(np.float64)
    c = C.contract64(x)
    assert float(np.abs(c).max()) < 2.0
    back = C.uncontract64(c)
    rel = np.abs(back - x) / np.maximum(np.abs(x).max(axis=1, keepdims=True), 1e-300)
    print("round trip, largest relative distance:", rel.max())
    assert rel.max() <= 1e-10
    inside = np.abs(x).max(axis=1) <= 1
    assert inside.any() and np.array_equal(c[inside], x[inside]) and np.array_equal(back[inside], x[inside])


def test_contract_statement_against_float64():
    from nerf2mesh_amd.renderer import contract
    x = C.contract_points()
    got = contract(torch.from_numpy(x)).numpy()
    assert got.dtype == np.float32
    d = C.ulp_distance(got, C.contract64(x))
    print("contract: largest ulp distance", d.max())
    assert d.max() <= CONTRACT_ULP
    inside = np.abs(x).max(axis=1) <= 1                       # mag exactly 1 included: the row itself, in its own bits
    assert np.array_equal(got[inside].view(np.int32), x[inside].view(np.int32))
    # (the next float above 1 takes the other branch and lands on itself, 1 + e - e^2 rounded: the ulp bound above covers it)
    assert np.allclose(contract(torch.tensor([[1.5, 0.0, -0.75]])).numpy(), [[4 / 3, 0.0, -2 / 3]], rtol=1e-6)
    assert float(np.abs(got).max()) < 2.0


def test_uncontract_statement_against_float64():
    from nerf2mesh_amd.renderer import contract, uncontract
    x = C.uncontract_points()
    got = uncontract(torch.from_numpy(x)).numpy()
    assert got.dtype == np.float32
    d = C.ulp_distance(got, C.uncontract64(x))
    print("uncontract: largest ulp distance", d.max())
    assert d.max() <= UNCONTRACT_ULP
    inside = np.abs(x).max(axis=1) <= 1
    assert np.array_equal(got[inside].view(np.int32), x[inside].view(np.int32))
    # the edge of the lattice lands where the formula says: 1 / (2 - mag) = 32
    e = uncontract(torch.tensor([[C.EDGE, 0.0, -C.EDGE]], dtype=torch.float32)).numpy()
    assert np.allclose(e, [[32.0, 0.0, -32.0]], rtol=1e-5)
    # fp32 round trip of world points that a bound-2 scene holds
    w = torch.from_numpy(C.contract_points()[:, :]).clamp(-8, 8)
    back = uncontract(contract(w))
    assert float(((back - w).abs() / w.abs().amax(dim=1, keepdim=True).clamp_min(1)).max()) <= 1e-4


def test_nonfinite_rows_follow_the_statement():
    """A row with a NaN comes out all NaN from both (torch.amax hands the NaN on, `mag <= 1` fails); mag > 2 uncontracts through the
    formula's negative denominator, mag == 2 through its zero."""
    from nerf2mesh_amd.renderer import contract, uncontract
    x = C.nonfinite_points()
    has_nan = np.isnan(x).any(axis=1)
    assert has_nan.sum() >= 4
    for fn in (contract, uncontract):
        got = fn(torch.from_numpy(x)).numpy()
        assert np.isnan(got[has_nan]).all()
    u = uncontract(torch.tensor([[3.0, 0.5, 0.0], [2.0, -2.0, 1.0]])).numpy()
    assert np.allclose(u[0], [-1.0, -1.0 / 6.0, 0.0], rtol=1e-6) and np.isinf(u[1]).all()
    c = contract(torch.tensor([[np.inf, 1.0, 0.0]])).numpy()
    assert np.isnan(c[0, 0]) and c[0, 1] == 0.0 and c[0, 2] == 0.0          # inf * 2 / inf, 1 * 2 / inf, 0 * 2 / inf


def test_sdf_recipe_on_an_unbounded_scene_contracts():
    """make_options(sdf=True, bound=2) (main.py:138-157): contract on, the grid bound 2, two cascades -- stage 1 expects mesh_0 and mesh_1."""
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    opt = make_options(sdf=True, bound=2)
    assert opt.contract and opt.enable_offset_nerf_grad and not opt.mark_untrained
    model = NeRFNetwork(opt)
    assert model.cascade == 2 and model.bound == 2 and model.real_bound == 2
    assert model.aabb_train.tolist() == [-2, -2, -2, 2, 2, 2]
    assert not make_options(sdf=True, bound=1).contract
