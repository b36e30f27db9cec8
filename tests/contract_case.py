"""Points and float64 restatements shared by tests/test_contract_cpu.py and tests/test_contract_kernels_gpu.py.

contract (nerf/renderer.py:25-32):    mag = max |x_i|;  mag <= 1 ? x : x * (2 - 1 / mag) / mag
uncontract (nerf/renderer.py:34-41):  mag = max |x_i|;  mag <= 1 ? x : x * (1 / (2 * mag - mag * mag))
"""
import numpy as np

R = 64
EDGE = 2.0 - 2.0 / R            # the largest contracted magnitude a lattice of R points per axis reaches (export_stage0's scale)


def contract64(x):
    x = np.asarray(x, dtype=np.float64)
    mag = np.max(np.abs(x), axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        return np.where(mag <= 1, x, x * (2 - 1 / mag) / mag)


def uncontract64(x):
    x = np.asarray(x, dtype=np.float64)
    mag = np.max(np.abs(x), axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        return np.where(mag <= 1, x, x * (1 / (2 * mag - mag * mag)))


def special_points():
    """fp32 [n,3]: mag exactly 1 and the next float above it, 0, negative components, ties between two axes, mag = 1e4, mag = 2 - 2/64."""
    up = np.nextafter(np.float32(1), np.float32(2))
    dn = np.nextafter(np.float32(1), np.float32(0))
    pts = [
        [0, 0, 0], [1, 0, 0], [0, -1, 0], [0.3, 1, -1], [1, 1, 1], [-1, -1, -1], [dn, dn, -dn],
        [up, 0, 0], [0, -up, 0.5], [up, up, -0.25], [-up, up, up], [0.999, -0.5, up],
        [1.5, 1.5, 0.1], [-1.5, 0.2, 1.5], [1.5, -1.5, -1.5], [0.25, -3, 3],
        [1e4, 0, 0], [-1e4, 1e4, 3], [12.5, -1e4, 1e-3], [1e4, 1e4, 1e4],
        [EDGE, 0, 0], [-EDGE, EDGE, 0.5], [0.1, -0.2, -EDGE], [EDGE, EDGE, EDGE],
        [1.25, -0.75, 0.5], [-0.5, 0.25, -1.75], [1e-30, 2.5, -1e-30], [-0.0, 1.5, 0.0],
    ]
    return np.asarray(pts, dtype=np.float32)


def contract_points(n_random=4096, seed=11):
    """Inputs of `contract`: the special points and random points in [-8, 8]^3."""
    rng = np.random.default_rng(seed)
    return np.concatenate([special_points(), rng.uniform(-8, 8, size=(n_random, 3)).astype(np.float32)])


def uncontract_points(n_random=4096, seed=12):
    """Inputs of `uncontract` where it is well conditioned, the contracted cube a 64-point lattice spans: the special points with
    mag <= 2 - 2/64 and random points in [-(2 - 2/64), 2 - 2/64]^3.  (Towards mag = 2 the statement's 2 * mag - mag * mag cancels: its
    fp32 form is then as far from the real inverse as the cancellation makes it, which is a property of the statement, not a defect.)"""
    rng = np.random.default_rng(seed)
    sp = special_points()
    sp = sp[np.abs(sp).max(axis=1) <= np.float32(EDGE)]
    return np.concatenate([sp, rng.uniform(-EDGE, EDGE, size=(n_random, 3)).astype(np.float32)])


def nonfinite_points():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    return np.asarray([[inf, 0, 0], [-inf, 1, 2], [inf, inf, -inf], [nan, 0, 0], [0.5, nan, 0.25], [3, nan, inf], [nan, nan, nan],
                       [2, 0, 0], [2, -2, 1], [3, 0.5, 0], [1e30, -1e30, 1], [3e38, 1, -3e38], [1e-40, 1e-45, 0]], dtype=np.float32)


def ulp_distance(got32, want64):
    """|got - want| in units of the fp32 spacing at |want| (got fp32, want the float64 restatement), elementwise."""
    want64 = np.asarray(want64, dtype=np.float64)
    ulp = np.spacing(np.maximum(np.abs(want64), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got32, dtype=np.float64) - want64) / ulp
