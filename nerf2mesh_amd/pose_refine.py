"""Camera-pose refinement in stage 0 (options.optimize_poses; not a reference feature -- DESIGN 4.31).

A view's stored pose is camera-to-world [R0 | t0]; its correction delta = (omega, tau) refines it to [E(omega) R0 | t0 + tau] with
E = exp([omega]x): a rotation about the camera centre in world axes, so ray origins depend on tau only.  For a ray of view v with origin o,
world direction d and samples x_i = o + t_i d (t_i = ts[i,0] - ts[i,1]: the marcher writes t after the step and forms x_i before it), with
g_i = dL/dx_i and h_i = dL/d(dirs_i):

    g_o = sum_i g_i,   g_d = sum_i (t_i g_i + h_i),   dL/dtau_v = sum_rays g_o,   dL/domega_v = J_l(omega_v)^T sum_rays (d x g_d)

J_l the left Jacobian of SO(3).  The sample depths are not differentiated (the marcher is not differentiable in the reference either), and
neither is the clamp of a sample to the scene box.  Under opt.contract the marcher hands out contracted samples: the gradient is taken back
through the contraction first (inside n2m_pose_ray_grad; contract_vjp is its torch statement).

PoseRefiner holds delta and its optimizer; `attach` is the link from the renderer's samples to delta.grad (n2m_pose_ray_grad +
n2m_pose_view_grad on the device); `attach_torch` states the same computation in torch ops (CPU tensors, any float dtype; what the kernels
are timed against)."""
import copy
import hashlib

import torch
from torch import nn
from torch.autograd import Function

SERIES_THETA = 1e-2       # N2M_POSE_SERIES_THETA of include/n2m_hip.h: below it the coefficients come from their Taylor series


def _coefficients(omega):
    """(A, B, C) [V] of omega [V,3]: sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3, from their series below SERIES_THETA."""
    t2 = (omega * omega).sum(-1)
    small = t2 < SERIES_THETA * SERIES_THETA
    th = torch.sqrt(torch.where(small, torch.ones_like(t2), t2))
    s2 = torch.where(small, t2, torch.zeros_like(t2))
    A = torch.where(small, 1 - s2 / 6 + s2 * s2 / 120 - s2 ** 3 / 5040, torch.sin(th) / th)
    B = torch.where(small, 0.5 - s2 / 24 + s2 * s2 / 720 - s2 ** 3 / 40320, (1 - torch.cos(th)) / (th * th))
    C = torch.where(small, 1 / 6 - s2 / 120 + s2 * s2 / 5040 - s2 ** 3 / 362880, (th - torch.sin(th)) / (th * th * th))
    return A, B, C


def _skew(omega):
    x, y, z = omega.unbind(-1)
    o = torch.zeros_like(x)
    return torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).view(*omega.shape[:-1], 3, 3)


def rotation(omega):
    """E(omega) = exp([omega]x) [V,3,3] by Rodrigues' formula."""
    A, B, _ = _coefficients(omega)
    K = _skew(omega)
    return torch.eye(3, dtype=omega.dtype, device=omega.device) + A[:, None, None] * K + B[:, None, None] * (K @ K)


def left_jacobian(omega):
    """J_l(omega) [V,3,3] = I + (1 - cos th) / th^2 [omega]x + (th - sin th) / th^3 [omega]x^2."""
    _, B, C = _coefficients(omega)
    K = _skew(omega)
    return torch.eye(3, dtype=omega.dtype, device=omega.device) + B[:, None, None] * K + C[:, None, None] * (K @ K)


def pose_apply_torch(poses0, delta):
    """The refined pose table in torch ops (float64 inside, rounded once): [E(omega) R0 | t0 + tau]; what delta leaves at zero keeps its bits."""
    out = poses0.clone()
    d = delta.detach()
    R = (rotation(d[:, :3].double()) @ poses0[:, :3, :3].double()).to(poses0.dtype)
    turned = (d[:, :3] != 0).any(-1)
    out[:, :3, :3] = torch.where(turned[:, None, None], R, poses0[:, :3, :3])
    out[:, :3, 3] = torch.where(d[:, 3:] != 0, poses0[:, :3, 3] + d[:, 3:].to(poses0.dtype), poses0[:, :3, 3])
    return out


def contract_vjp(xyzs, grad):
    """grad [M,3] with respect to the contracted samples xyzs (renderer.contract of the world points, as the marcher writes them under
    opt.contract) -> the gradient with respect to the world points.  Inside the unit box the contraction is the identity; outside,
    y = k(m) x with m = max_a |x_a| and k = (2 - 1/m) / m, so J^T g = k g + e_a sign(x_a) k'(m) <x, g>, a the axis of the maximum."""
    mag = xyzs.abs().amax(dim=1, keepdim=True)
    outside = mag > 1
    m = 1 / (2 - torch.where(outside, mag, torch.ones_like(mag))).clamp_min(1e-6)      # |y| = 2 - 1/m
    k = (2 - 1 / m) / m
    x = xyzs / k
    dk = -2 / m ** 2 + 2 / m ** 3
    axis = xyzs.abs().argmax(dim=1, keepdim=True)
    e = torch.zeros_like(xyzs).scatter_(1, axis, torch.sign(xyzs.gather(1, axis)))
    back = k * grad + e * dk * (x * grad).sum(1, keepdim=True)
    return torch.where(outside, back, grad)


def _view_rows(view, N, device):
    """`view` as int32 [N]: one integer (a single-view batch: a sparse-depth step) names every ray's view."""
    if view is None:
        raise ValueError("pose refinement needs the view of every ray (`index`)")
    if not torch.is_tensor(view):
        return torch.full((N,), int(view), dtype=torch.int32, device=device)
    view = view.reshape(-1).to(device=device, dtype=torch.int32)
    if view.numel() == 1 and N != 1:
        view = view.expand(N)
    if view.numel() != N:
        raise ValueError(f"pose refinement: `view` names {view.numel()} views for {N} rays")
    return view.contiguous()


def pose_grad_torch(grad_xyzs, grad_dirs, ts, rays, rays_d, view, delta):
    """grad_delta [V,6] in torch ops, in grad_xyzs' dtype: what n2m_pose_ray_grad + n2m_pose_view_grad compute."""
    dt, dev = grad_xyzs.dtype, grad_xyzs.device
    M, N, V = grad_xyzs.shape[0], rays.shape[0], delta.shape[0]
    off, cnt = rays[:, 0].long(), rays[:, 1].long()
    ok = (off >= 0) & (cnt > 0) & (off + cnt <= M)
    cnt = torch.where(ok, cnt, torch.zeros_like(cnt))
    rid = torch.repeat_interleave(torch.arange(N, device=dev), cnt)          # the ray of every owned sample, ray by ray
    first = torch.cumsum(cnt, 0) - cnt
    idx = off[rid] + (torch.arange(rid.shape[0], device=dev) - first[rid])
    g = grad_xyzs[idx]
    t = (ts[idx, 0].to(dt) - ts[idx, 1].to(dt)).unsqueeze(1)
    terms = t * g if grad_dirs is None else t * g + grad_dirs[idx].to(dt)
    g_o = torch.zeros(N, 3, dtype=dt, device=dev).index_add_(0, rid, g)
    g_d = torch.zeros(N, 3, dtype=dt, device=dev).index_add_(0, rid, terms)
    turn = torch.cross(rays_d.to(dt), g_d, dim=1)
    view = view.long()
    known = (view >= 0) & (view < V)                                         # a view outside [0, V) is skipped
    s_tau = torch.zeros(V, 3, dtype=dt, device=dev).index_add_(0, view[known], g_o[known])
    s_rot = torch.zeros(V, 3, dtype=dt, device=dev).index_add_(0, view[known], turn[known])
    J = left_jacobian(delta.detach()[:, :3].to(dt))
    return torch.cat([torch.einsum("vji,vj->vi", J, s_rot), s_tau], 1)


class _AttachTorch(Function):
    @staticmethod
    def forward(ctx, xyzs, dirs, delta, ts, rays, rays_d, view, contract):
        ctx.save_for_backward(xyzs, delta, ts, rays, rays_d, view)
        ctx.contract = bool(contract)
        ctx.set_materialize_grads(False)
        return xyzs.view_as(xyzs), dirs.view_as(dirs)

    @staticmethod
    def backward(ctx, grad_xyzs, grad_dirs):
        xyzs, delta, ts, rays, rays_d, view = ctx.saved_tensors
        if grad_xyzs is None and grad_dirs is None:
            return (None,) * 8
        if grad_xyzs is None:
            grad_xyzs = torch.zeros_like(grad_dirs)
        if ctx.contract:
            grad_xyzs = contract_vjp(xyzs.to(grad_xyzs.dtype), grad_xyzs)
        g = pose_grad_torch(grad_xyzs, grad_dirs, ts, rays, rays_d, view, delta)
        return None, None, g.to(delta.dtype), None, None, None, None, None


class _AttachDevice(Function):
    @staticmethod
    def forward(ctx, xyzs, dirs, delta, ts, rays, rays_d, view, contract):
        ctx.save_for_backward(xyzs, delta, ts, rays, rays_d, view)
        ctx.contract = bool(contract)
        ctx.set_materialize_grads(False)
        return xyzs.view_as(xyzs), dirs.view_as(dirs)

    @staticmethod
    def backward(ctx, grad_xyzs, grad_dirs):
        from . import _lib as L
        xyzs, delta, ts, rays, rays_d, view = ctx.saved_tensors
        if grad_xyzs is None and grad_dirs is None:
            return (None,) * 8
        M, N, V, dev = xyzs.shape[0], rays.shape[0], delta.shape[0], xyzs.device
        grad_xyzs = torch.zeros(M, 3, dtype=torch.float32, device=dev) if grad_xyzs is None else grad_xyzs.float().contiguous()
        grad_dirs = None if grad_dirs is None else grad_dirs.float().contiguous()
        ray6 = torch.empty(N, 6, dtype=torch.float32, device=dev)
        grad_delta = torch.empty(V, 6, dtype=torch.float32, device=dev)
        L.call("n2m_pose_ray_grad", L.ptr(grad_xyzs), L.ptr(grad_dirs), L.ptr(xyzs) if ctx.contract else None, L.ptr(ts), L.ptr(rays), L.ptr(rays_d), M, N, L.ptr(ray6), L.stream())
        L.call("n2m_pose_view_grad", L.ptr(ray6), L.ptr(view), L.ptr(delta), N, V, L.ptr(grad_delta), L.stream())
        return None, None, grad_delta, None, None, None, None, None


def attach_torch(xyzs, dirs, delta, ts, rays, rays_d, view, contract=False):
    """(xyzs, dirs) with unchanged values whose gradients reach delta [V,6] -- the torch statement of PoseRefiner.attach."""
    view = _view_rows(view, rays.shape[0], xyzs.device)
    return _AttachTorch.apply(xyzs, dirs, delta, ts, rays, rays_d, view, contract)


class PoseRefiner:
    """delta [V,6] = (omega, tau) per view, zeros at the start, with an Adam of its own on the trainer's learning-rate schedule."""

    def __init__(self, poses0, lr=1e-3, iters=30000, contract=False):
        from .trainer import LambdaLR, lr_schedule
        poses0 = torch.as_tensor(poses0)
        if poses0.dim() != 3 or tuple(poses0.shape[1:]) != (4, 4):
            raise ValueError("poses0 must be [V,4,4]")
        self.poses0 = poses0.detach().float().contiguous().clone()
        dev = self.poses0.device
        self.contract = bool(contract)
        self.delta = nn.Parameter(torch.zeros(self.poses0.shape[0], 6, dtype=torch.float32, device=dev))
        self.optimizer = torch.optim.Adam([self.delta], lr=float(lr), eps=1e-15, fused=(dev.type == "cuda"))
        self.scheduler = LambdaLR(self.optimizer, lr_schedule(int(iters)))       # the trainer's own schedule
        self._poses = self.poses0.clone()          # the one buffer poses() writes: a trainer's pose table may BE this tensor
        self.checksum = hashlib.sha256(self.poses0.cpu().numpy().tobytes()).hexdigest()

    def __len__(self):
        return int(self.poses0.shape[0])

    @torch.no_grad()
    def poses(self):
        """The refined pose table [V,4,4], written into the persistent buffer (n2m_pose_apply)."""
        if self.poses0.is_cuda:
            from . import _lib as L
            L.call("n2m_pose_apply", L.ptr(self.poses0), L.ptr(self.delta), len(self), L.ptr(self._poses), L.stream())
        else:
            self._poses.copy_(pose_apply_torch(self.poses0, self.delta))
        return self._poses

    def attach(self, xyzs, dirs, ts, rays, rays_d, view):
        """(xyzs, dirs) with unchanged values; their gradients are reduced per ray and per view into delta.grad on the way back.
        view: int32 [N], or one integer for a single-view batch."""
        view = _view_rows(view, rays.shape[0], xyzs.device)
        if not xyzs.is_cuda:
            return _AttachTorch.apply(xyzs, dirs, self.delta, ts, rays, rays_d, view, self.contract)
        return _AttachDevice.apply(xyzs.contiguous(), dirs.contiguous(), self.delta, ts.float().contiguous(), rays.to(torch.int32).contiguous(),
                                   rays_d.float().contiguous(), view, self.contract)

    def refined(self, capture):
        """A Capture with the refined poses (and the model-view-projections that follow from them); everything else is shared."""
        from .capture import proj_matrix
        if len(capture) != len(self):
            raise ValueError(f"the capture has {len(capture)} views, the refiner {len(self)}")
        out = copy.copy(capture)
        poses = self.poses().detach().clone()
        out.poses = poses.to(capture.poses.device)
        host = poses.cpu()
        out.mvps = torch.stack([proj_matrix(capture.H, capture.W, *capture.intrinsics_of(v)) @ torch.inverse(p)
                                for v, p in enumerate(host)]).to(capture.mvps.device)
        return out

    def state_dict(self):
        return {"delta": self.delta.detach().clone(), "poses0_checksum": self.checksum, "optimizer": self.optimizer.state_dict(),
                "last_epoch": int(self.scheduler.last_epoch)}

    @torch.no_grad()
    def load_state_dict(self, sd):
        if sd["poses0_checksum"] != self.checksum:
            raise ValueError("pose refinement: the checkpoint's corrections belong to other stored poses (checksum mismatch)")
        if tuple(sd["delta"].shape) != tuple(self.delta.shape):
            raise ValueError(f"pose refinement: the checkpoint holds delta {tuple(sd['delta'].shape)}, this run {tuple(self.delta.shape)}")
        self.delta.copy_(sd["delta"].to(self.delta.device))
        self.optimizer.load_state_dict(sd["optimizer"])
        self.scheduler.load_state_dict({"last_epoch": int(sd["last_epoch"])})
        self.poses()


class JointStep:
    """What a GradScaler is handed in place of the field's optimizer when poses are refined: one unscale_ over both optimizers' gradients
    and one inf / nan verdict, so either both step or neither does.  The verdict arrives the way torch's fused Adam takes it (the
    `grad_scale` / `found_inf` attributes GradScaler.step sets) and is passed on as it is: no host read."""
    _step_supports_amp_scaling = True

    def __init__(self, *optimizers):
        self.optimizers = optimizers

    @property
    def param_groups(self):
        return [g for o in self.optimizers for g in o.param_groups]

    def step(self):
        scale, found = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        for o in self.optimizers:
            if found is not None:
                o.grad_scale, o.found_inf = scale, found
            try:
                o.step()
            finally:
                if found is not None:
                    del o.grad_scale, o.found_inf
