"""Float64 model of the pose-refinement kernels (csrc/posegrad.hip) in numpy: apply, ray_grad, view_grad, and the function
whose gradient they are.  Written from the definitions, not from the kernels: the rotation and SO(3)'s left Jacobian are summed as the
power series  E = sum_k K^k / k!,  J_l = sum_k K^k / (k + 1)!  (K = [omega]x), which need no branch at small angles.

The `planted` switches of ray_grad / view_grad state three mistakes an implementation can make; the CPU tests show that the
finite-difference check tells each of them from the model."""
import numpy as np

TERMS = 48          # |omega| <= 2.5: 2.5^48 / 48! = 1e-42


def skew(w):
    x, y, z = (float(c) for c in w)
    return np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]], dtype=np.float64)


def _series(w, shift):
    K, term, out = skew(w), np.eye(3), np.zeros((3, 3))
    fact = 1.0
    for k in range(TERMS):
        if k > 0:
            term = term @ K
            fact *= k
        out = out + term / (fact * (k + 1 if shift else 1))
    return out


def rotation(w):
    """exp([w]x), float64 [3,3]."""
    return _series(np.asarray(w, np.float64), False)


def left_jacobian(w):
    return _series(np.asarray(w, np.float64), True)


def apply(poses0, delta):
    """[V,4,4] float64: [E(omega) R0 | t0 + tau], the bottom row as stored."""
    p0, d = np.asarray(poses0, np.float64), np.asarray(delta, np.float64)
    out = p0.copy()
    for v in range(p0.shape[0]):
        out[v, :3, :3] = rotation(d[v, :3]) @ p0[v, :3, :3]
        out[v, :3, 3] = p0[v, :3, 3] + d[v, 3:]
    return out


def contract_vjp(xyzs, grad):
    """(J^T g, |k g| + |k'(m)| sum_a |x_a g_a| on the axis of the maximum) for the contraction y = k(m) x, m = max_a |x_a|, k = (2 - 1/m) / m,
    evaluated at the contracted points y = xyzs (max_a |y_a| = 2 - 1/m); the identity where max_a |y_a| <= 1.  The second value is the sum
    of the absolute values of each component's terms."""
    y, g = np.asarray(xyzs, np.float64), np.asarray(grad, np.float64)
    out, mag_out = g.copy(), np.abs(g)
    for i in range(y.shape[0]):
        mag = np.abs(y[i]).max()
        if mag <= 1:
            continue
        m = 1 / max(2 - mag, 1e-6)
        k, dk = (2 - 1 / m) / m, -2 / m ** 2 + 2 / m ** 3
        x, a = y[i] / k, int(np.abs(y[i]).argmax())
        out[i], mag_out[i] = k * g[i], np.abs(k * g[i])
        out[i, a] += np.sign(y[i, a]) * dk * (x @ g[i])
        mag_out[i, a] += abs(dk) * (np.abs(x) @ np.abs(g[i]))
    return out, mag_out


def ray_grad(grad_xyzs, grad_dirs, ts, rays, rays_d, planted=None, xyzs=None):
    """(ray6 [N,6] = (g_o, d x g_d), S [N,6]: the sum of the absolute values of each component's terms), float64.  t_i = ts[i,0] - ts[i,1].
    planted: None | "no_t" (g_d without the t_i factor) | "swap_cross" (g_d x d).  xyzs: the contracted samples (opt.contract) -- grad_xyzs
    is taken back through the contraction first."""
    g = np.asarray(grad_xyzs, np.float64)
    g_abs = np.abs(g)
    if xyzs is not None:
        g, g_abs = contract_vjp(xyzs, g)
    h = np.zeros_like(g) if grad_dirs is None else np.asarray(grad_dirs, np.float64)
    ts, d = np.asarray(ts, np.float64), np.asarray(rays_d, np.float64)
    N, M = rays.shape[0], g.shape[0]
    out, S = np.zeros((N, 6)), np.zeros((N, 6))
    for r in range(N):
        off, cnt = int(rays[r, 0]), int(rays[r, 1])
        if off < 0 or cnt <= 0 or off + cnt > M:
            continue
        sl = slice(off, off + cnt)
        t = (ts[sl, 0] - ts[sl, 1])[:, None]
        if planted == "no_t":
            t = np.ones_like(t)
        terms = t * g[sl]
        g_d, a_d = (terms + h[sl]).sum(0), (np.abs(t) * g_abs[sl] + np.abs(h[sl])).sum(0)
        out[r, :3], S[r, :3] = g[sl].sum(0), g_abs[sl].sum(0)
        out[r, 3:] = np.cross(g_d, d[r]) if planted == "swap_cross" else np.cross(d[r], g_d)
        a = np.abs(d[r])
        S[r, 3:] = [a[1] * a_d[2] + a[2] * a_d[1], a[2] * a_d[0] + a[0] * a_d[2], a[0] * a_d[1] + a[1] * a_d[0]]
    return out, S


def view_grad(ray6, view, delta, planted=None):
    """(grad_delta [V,6] = (J_l^T sum d x g_d, sum g_o), S [V,6], rays per view [V]).  S: the sum over the view's rays of |ray6| per
    component; for the rotational half the largest of the three, times the largest absolute row sum of J_l^T (at most 3).
    planted: None | "no_jacobian"."""
    r6, d = np.asarray(ray6, np.float64), np.asarray(delta, np.float64)
    mag = np.abs(r6)
    V = d.shape[0]
    out, S, count = np.zeros((V, 6)), np.zeros((V, 6)), np.zeros(V, dtype=np.int64)
    for v in range(V):
        rows = np.nonzero(np.asarray(view) == v)[0]
        count[v] = len(rows)
        J = np.eye(3) if planted == "no_jacobian" else left_jacobian(d[v, :3])
        out[v, :3], out[v, 3:] = J.T @ r6[rows, 3:].sum(0), r6[rows, :3].sum(0)
        S[v, :3], S[v, 3:] = np.abs(J.T).sum(1).max() * mag[rows, 3:].sum(0).max(initial=0.0) * np.ones(3), mag[rows, :3].sum(0)
    return out, S, count


# --------------------------------------------------------------------------------------------------------- the function itself
def make_case(V=3, rays_per_view=3, samples=(0, 1, 5, 7), seed=0, norms=(0.0, 0.3, 2.5)):
    """A small scene for the finite-difference check: V stored poses (random rotations), delta with the given |omega| per view, rays with
    camera-frame directions, fixed ts = (t after the step, dt), random c (per sample) and e (per sample)."""
    rng = np.random.default_rng(seed)
    poses0 = np.tile(np.eye(4), (V, 1, 1))
    delta = np.zeros((V, 6))
    for v in range(V):
        poses0[v, :3, :3] = rotation(rng.normal(size=3))
        poses0[v, :3, 3] = rng.normal(size=3)
        axis = rng.normal(size=3)
        delta[v, :3] = axis / np.linalg.norm(axis) * norms[v % len(norms)]
        delta[v, 3:] = rng.normal(size=3) * 0.1
    N = V * rays_per_view
    view = np.repeat(np.arange(V), rays_per_view).astype(np.int32)
    rng.shuffle(view)
    d_cam = rng.normal(size=(N, 3))
    cnt = np.array([samples[r % len(samples)] for r in range(N)], dtype=np.int32)
    order = rng.permutation(N)                                   # the rays tile [0, M) in a shuffled order
    off = np.zeros(N, dtype=np.int32)
    off[order] = np.concatenate([[0], np.cumsum(cnt[order])[:-1]])
    rays = np.stack([off, cnt], 1).astype(np.int32)
    M = int(cnt.sum())
    dt = rng.uniform(0.01, 0.05, size=M)
    ts = np.stack([rng.uniform(0.5, 4.0, size=M) + dt, dt], 1)
    return dict(poses0=poses0, delta=delta, view=view, d_cam=d_cam, rays=rays, ts=ts, c=rng.normal(size=(M, 3)), e=rng.normal(size=(M, 3)), M=M, N=N, V=V)


def world_dirs(case, delta):
    """rays_d [N,3] at `delta`: E(omega_v) R0_v d_cam."""
    P = apply(case["poses0"], delta)
    return np.einsum("nij,nj->ni", P[case["view"], :3, :3], case["d_cam"])


def objective(case, delta):
    """sum_i <c_i, x_i(delta)> + <e_i, d(delta)>, x_i = o + t_i d, o the refined camera centre, t_i = ts[i,0] - ts[i,1] held fixed."""
    P, d = apply(case["poses0"], delta), world_dirs(case, delta)
    total = 0.0
    for r in range(case["N"]):
        off, cnt = case["rays"][r]
        for i in range(off, off + cnt):
            t = case["ts"][i, 0] - case["ts"][i, 1]
            total += case["c"][i] @ (P[case["view"][r], :3, 3] + t * d[r]) + case["e"][i] @ d[r]
    return total


def finite_differences(case, delta, step=1e-6):
    g = np.zeros_like(delta)
    for idx in np.ndindex(*delta.shape):
        hi, lo = delta.copy(), delta.copy()
        hi[idx] += step
        lo[idx] -= step
        g[idx] = (objective(case, hi) - objective(case, lo)) / (2 * step)
    return g


def model_gradient(case, delta, planted=None):
    """d objective / d delta through ray_grad + view_grad (g_i = c_i, h_i = e_i)."""
    r6, _ = ray_grad(case["c"], case["e"], case["ts"], case["rays"], world_dirs(case, delta), planted=planted if planted != "no_jacobian" else None)
    return view_grad(r6, case["view"], delta, planted=planted if planted == "no_jacobian" else None)[0]
