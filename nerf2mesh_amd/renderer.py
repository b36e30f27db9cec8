"""Stage-0 volume renderer on the HIP operators: the caller-side logic of nerf/renderer.py (render :676-813,
update_extra_state :1074-1149, mark_untrained_grid :985-1071) restated on top of nerf2mesh_amd.raymarching.

Buffer names/shapes follow the reference (`density_grid [cascade, H^3]`, `density_bitfield [cascade*H^3/8]`,
`aabb_train/aabb_infer [6]`) so its checkpoints load.  What changed for ROCm:
* the occupancy refresh walks the grid in Morton order (cell i -> morton3D_invert(i)), so densities land in
  `tmp_grid` without the index scatter of :1118; the cell coordinates are cached across refreshes;
* the inference loop compacts the alive list on the device (raymarching.compact_alive) instead of boolean
  indexing (:798).
"""
import math

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import raymarching
from . import raster as dr


def safe_normalize(x, eps=1e-20):
    return x / torch.sqrt(torch.clamp(torch.sum(x * x, -1, keepdim=True), min=eps))   # nerf/utils.py:safe_normalize


class _to_clip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, mvp):
        from . import _lib as L
        vertices, mvp = vertices.float().contiguous(), mvp.float().contiguous()
        clip = torch.empty(vertices.shape[0], 4, dtype=torch.float32, device=vertices.device)
        L.call("n2m_to_clip", L.ptr(vertices), L.ptr(mvp), vertices.shape[0], L.ptr(clip), L.stream())
        ctx.save_for_backward(mvp)
        return clip

    @staticmethod
    def backward(ctx, g):
        from . import _lib as L
        mvp, = ctx.saved_tensors
        g = g.float().contiguous()
        d = torch.empty(g.shape[0], 3, dtype=torch.float32, device=g.device)
        L.call("n2m_to_clip_backward", L.ptr(g), L.ptr(mvp), g.shape[0], L.ptr(d), L.stream())
        return d, None


def to_clip(vertices, mvp):
    """[V,3] world -> [V,4] clip = [v,1] @ mvp^T (nerf/renderer.py:858).  On the GPU one launch each way (n2m_to_clip); elsewhere three
    broadcast multiply-adds in the same association (the BLAS library runs this (V x 4) x (4 x 4) product as a single-workgroup GEMM:
    2.7 ms for 159k vertices, measured)."""
    if vertices.is_cuda and vertices.dim() == 2:
        return _to_clip.apply(vertices, mvp)
    m = mvp.float()
    return (vertices[:, 0:1] * m[:, 0] + vertices[:, 1:2] * m[:, 1] + vertices[:, 2:3] * m[:, 2] + m[:, 3]).contiguous()


def percentile_linear(x, q):
    """numpy.percentile(x, q) (method "linear") of a 1-D float tensor, on its device, in numpy's arithmetic: q / 100 and the virtual index
    (n - 1) * q in the data's dtype, then numpy's two-sided lerp -- the threshold compares the same way numpy's does."""
    n = x.numel()
    s = torch.sort(x).values
    qq = torch.tensor(float(q), dtype=x.dtype) / 100
    vi = (n - 1) * qq
    lo_t = torch.floor(vi)
    g = (vi - lo_t).to(x.device)
    lo = int(lo_t)
    hi = min(lo + 1, n - 1)
    a, b = s[lo], s[hi]
    d = b - a
    return torch.where(g >= 0.5, b - d * (1 - g), a + d * g)


def _contract_rows(name, xyzs):
    """n2m_contract / n2m_uncontract on a device tensor [N,3] fp32 with no graph attached: one launch, the bits of the torch statement."""
    from . import _lib as L
    x = xyzs.contiguous()
    out = torch.empty_like(x)
    L.call(name, L.ptr(x), x.shape[0], L.ptr(out), L.stream())
    return out


def _device_rows(xyzs):
    return xyzs.is_cuda and xyzs.dim() == 2 and xyzs.shape[1] == 3 and xyzs.dtype == torch.float32 and not (torch.is_grad_enabled() and xyzs.requires_grad)


def contract(xyzs):
    """nerf/renderer.py:25-32.  Device rows without a gradient take one launch (n2m_contract, same bits); everything else the statement."""
    if _device_rows(xyzs):
        return _contract_rows("n2m_contract", xyzs)
    mag = torch.amax(torch.abs(xyzs), dim=1, keepdim=True)
    return torch.where(mag <= 1, xyzs, xyzs * (2 - 1 / mag) / mag)


def uncontract(xyzs):
    """The inverse (nerf/renderer.py:34-41): points of the contracted cube (-2, 2)^3 back to world space.  Device route as `contract`."""
    if _device_rows(xyzs):
        return _contract_rows("n2m_uncontract", xyzs)
    mag = torch.amax(torch.abs(xyzs), dim=1, keepdim=True)
    return torch.where(mag <= 1, xyzs, xyzs * (1 / (2 * mag - mag * mag)))


def dilate_cross(a):
    """One step of scipy.ndimage.binary_dilation with its default (4-neighbour cross) structuring element, on a [H,W] bool tensor."""
    b = a.clone()
    b[1:] |= a[:-1]; b[:-1] |= a[1:]; b[:, 1:] |= a[:, :-1]; b[:, :-1] |= a[:, 1:]
    return b


def erode_cross(a):
    """One step of scipy.ndimage.binary_erosion (cross element, border_value = 0: the outside of the image counts as empty)."""
    b = a.clone()
    b[1:] &= a[:-1]; b[:-1] &= a[1:]; b[:, 1:] &= a[:, :-1]; b[:, :-1] &= a[:, 1:]
    b[0] = False; b[-1] = False; b[:, 0] = False; b[:, -1] = False
    return b


# A/B switch: the reference's host-paced inference loop (one read of n_alive per round) instead of the device-count loop
_HOST_INFER_LOOP = os.environ.get("N2M_INFER_HOST_LOOP", "0") == "1"


class NeRFRenderer(nn.Module):
    @property
    def mean_density(self):
        t = getattr(self, "_mean_density_t", None)
        return float(t) if t is not None else 0.0

    @mean_density.setter
    def mean_density(self, v):
        self._mean_density_t = None if v == 0 else torch.tensor(float(v))

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.real_bound = opt.bound                        # marching bound (world)
        self.bound = 2 if opt.contract else opt.bound      # grid / hashing bound
        self.cascade = 1 + math.ceil(math.log2(self.bound))
        self.grid_size = opt.grid_size
        self.min_near = opt.min_near
        self.density_thresh = opt.density_thresh
        self.max_level = 16
        rb = self.real_bound
        self.register_buffer("aabb_train", torch.tensor([-rb, -rb, -rb, rb, rb, rb], dtype=torch.float32))
        self.register_buffer("aabb_infer", self.aabb_train.clone())
        self.individual_num, self.individual_dim = opt.ind_num, opt.ind_dim
        self.individual_codes = nn.Parameter(torch.randn(opt.ind_num, opt.ind_dim) * 0.1) if opt.ind_dim > 0 else None
        self.cuda_ray = True
        self.register_buffer("density_grid", torch.zeros(self.cascade, self.grid_size ** 3))
        self.register_buffer("density_bitfield", torch.zeros(self.cascade * self.grid_size ** 3 // 8, dtype=torch.uint8))
        self.mean_density = 0
        self.iter_density = 0
        self._cell_unit = None      # cached [H^3,3] cell centres in [-1,1], Morton order
        self.glctx = None
        # opt-in hook (pose refinement): a callable (xyzs, dirs, ts, rays, rays_d, index) -> (xyzs, dirs) that render() runs on a
        # training batch's samples right before the field is evaluated; the values stay, the gradients find their way to the cameras
        self.ray_attach = None

    def get_params(self, lr):
        params = []
        if self.individual_codes is not None:
            params.append({"params": self.individual_codes, "lr": self.opt.lr * 0.1, "weight_decay": 0})
        return params

    def density(self, x):
        raise NotImplementedError()

    def reset_extra_state(self):
        self.density_grid.zero_()
        self.mean_density = 0
        self.iter_density = 0

    def update_aabb(self, aabb):
        if not torch.is_tensor(aabb):
            aabb = torch.as_tensor(aabb).float()
        self.aabb_train = aabb.clamp(-self.real_bound, self.real_bound).to(self.aabb_train.device)
        self.aabb_infer = self.aabb_train.clone()

    # ------------------------------------------------------------------------------------------ stage 0
    @torch.no_grad()
    def march_ahead(self, rays_o, rays_d, dt_gamma=0, perturb=True, max_steps=1024, cam_near_far=None, expect_points=0, noises=None,
                    nears_fars=None):
        """Enqueue near/far + march pass 1 for a FUTURE training batch (they read only the occupancy bit field) and return a
        ticket for render(..., ticket=...).  Lets the training loop keep the GPU queue full across the sample-count read-back.
        nears_fars: (nears, fars) the batch kernel already derived (aabb slab test + the per-view cam_near_far clamp)."""
        rays_o = rays_o.contiguous().view(-1, 3)
        rays_d = rays_d.contiguous().view(-1, 3)
        if nears_fars is not None:
            nears, fars = nears_fars
        else:
            nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, self.aabb_train, self.min_near)
        if cam_near_far is not None:
            nears = torch.maximum(nears, cam_near_far[:, 0])
            fars = torch.minimum(fars, cam_near_far[:, 1])
        return raymarching.march_rays_train_begin(rays_o, rays_d, self.real_bound, self.opt.contract, self.density_bitfield, self.cascade,
                                                  self.grid_size, nears, fars, perturb, dt_gamma, max_steps, noises=noises,
                                                  expect_points=expect_points)

    def render(self, rays_o, rays_d, index=None, dt_gamma=0, bg_color=None, perturb=False, max_steps=1024, T_thresh=1e-4,
               cam_near_far=None, shading="full", ticket=None, blend_bg=True, nears_fars=None, **kwargs):
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3)
        rays_d = rays_d.contiguous().view(-1, 3)
        N, device = rays_o.shape[0], rays_o.device

        if ticket is None and nears_fars is not None:
            nears, fars = nears_fars                       # the batch kernel's: aabb slab test + the per-view clamp (as march_ahead takes them)
        elif ticket is None:
            nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, self.aabb_train if self.training else self.aabb_infer, self.min_near)
            if cam_near_far is not None:
                nears = torch.maximum(nears, cam_near_far[:, 0])
                fars = torch.minimum(fars, cam_near_far[:, 1])
        if bg_color is None:
            bg_color = 1
        ind_code = None
        fuse_ind = False      # per-image codes through the fused field: the kernel reads the parameter and a per-sample row (fused.IndCode)
        if self.individual_dim > 0:
            fuse_ind = hasattr(self, "ind_code") and not torch.is_tensor(self.ind_code())
            if fuse_ind:
                ind_code = self.ind_code()           # row 0 (eval); training: the samples' rows, once the marcher's table is known
            else:
                ind_code = self.individual_codes[index.long() if torch.is_tensor(index) else index] if self.training else self.individual_codes[[0]]
        results = {}
        amp = torch.autocast(device_type="cuda", dtype=torch.float16, enabled=bool(self.opt.fp16))

        if self.training:
            if ticket is not None:      # a MarchTicket of march_ahead, or the (xyzs, dirs, ts, rays) its finish() returned
                marched = ticket if isinstance(ticket, tuple) else raymarching.march_rays_train_finish(ticket)
                xyzs, dirs, ts, rays = marched
                # what the marcher was given (a plain 4-tuple from a caller of its own does not say: None)
                nears, fars = getattr(marched, "nears", None), getattr(marched, "fars", None)
            else:
                xyzs, dirs, ts, rays = raymarching.march_rays_train(rays_o, rays_d, self.real_bound, self.opt.contract, self.density_bitfield,
                                                                    self.cascade, self.grid_size, nears, fars, perturb, dt_gamma, max_steps)
            if xyzs.shape[0] == 0:
                # The reference launches zero-sized grids here and carries on with undefined outputs (no launch-error checks,
                # raymarching.cu / gridencoder.cu); the C ABI of this package rejects empty tensors.  The step executor
                # (engine.Stage0Engine) handles sample-free batches -- a rank in that state still takes part in every collective;
                # this autograd path does not, and says so instead of hanging a multi-rank job half-way through its collectives.
                raise RuntimeError("render: the batch marched no sample at all (cameras outside the scene / empty occupancy grid); "
                                   "the autograd renderer needs at least one sample -- the step executor handles empty batches")
            if fuse_ind:
                from .fused import sample_views
                if index is None:
                    raise ValueError("render: training with individual codes needs `index`, the view of every ray")
                idx = torch.as_tensor(index, device=device).reshape(-1).to(torch.int32).contiguous()
                if idx.numel() not in (1, N):
                    raise ValueError(f"render: `index` names {idx.numel()} views for {N} rays")
                ind_code = self.ind_code(sample_views(rays, idx, xyzs.shape[0]) if idx.numel() > 1 else idx.expand(xyzs.shape[0]).contiguous())
            elif ind_code is not None and ind_code.shape[0] > 1:
                ind_code = ind_code[raymarching.flatten_rays(rays, xyzs.shape[0]).long()]
            if self.ray_attach is not None:      # (in front of safe_normalize: the gradient wanted is the raw direction's, the one the pose turns)
                xyzs, dirs = self.ray_attach(xyzs, dirs, ts, rays, rays_d, index)
            in_kernel = hasattr(self, "_can_fuse") and self._can_fuse(ind_code)      # fused field: safe_normalize happens on load
            if not in_kernel:
                dirs = safe_normalize(dirs)
            with amp:
                sigmas, rgbs, speculars = self(xyzs, dirs, ind_code, shading, raw_dirs=True) if in_kernel else self(xyzs, dirs, ind_code, shading)
            if self.opt.sdf:
                raw_normal = self.normal(xyzs, self.opt.normal_anneal_epsilon)
                results["normal"] = raw_normal
                # (the fused field normalises the ray directions on load and leaves `dirs` raw: the cosine needs the unit vectors of
                # nerf/renderer.py:720 -- rounds 1-2 used the raw ones here, |d| up to 1.1, found when the step executor's SDF head, written
                # from the reference text, disagreed with this path)
                unit_dirs = safe_normalize(dirs) if in_kernel else dirs
                true_cos = (unit_dirs * safe_normalize(raw_normal)).sum(-1)
                car = self.opt.cos_anneal_ratio
                iter_cos = -(F.relu(-true_cos * 0.5 + 0.5) * (1.0 - car) + F.relu(-true_cos) * car)
                sigmas = self._sdf_to_alpha(sigmas, iter_cos, ts[:, 1])
            weights, weights_sum, depth, image = raymarching.composite_rays_train(sigmas, rgbs, ts, rays, T_thresh, self.opt.sdf,
                                                                                  rays_tile_samples=True)   # our marcher's ranges tile [0, M)
            results.update(num_points=xyzs.shape[0], xyzs=xyzs, speculars=speculars, weights=weights, weights_sum=weights_sum)
            results.update(ts=ts, rays=rays, nears=nears, fars=fars)      # the batch's intervals and ray table (losses.distortion_loss)
        else:
            weights_sum = torch.zeros(N, dtype=torch.float32, device=device)
            depth = torch.zeros(N, dtype=torch.float32, device=device)
            image = torch.zeros(N, 3, dtype=torch.float32, device=device)
            if device.type == "cuda" and not _HOST_INFER_LOOP and N > 0:
                self._infer_loop_device(rays_o, rays_d, nears, fars, ind_code, shading, dt_gamma, max_steps, T_thresh, perturb, amp,
                                        weights_sum, depth, image)
            else:
                self._infer_loop_host(rays_o, rays_d, nears, fars, ind_code, shading, dt_gamma, max_steps, T_thresh, perturb, amp,
                                      weights_sum, depth, image)
            results["weights_sum"] = weights_sum.view(*prefix)      # the rays' opacity, next to "depth" = sum of w t (tsdf.surface_depth)

        if blend_bg:       # blend_bg=False: the caller folds the blend into its loss kernel (losses.photo_loss)
            image = image + (1 - weights_sum).unsqueeze(-1) * bg_color
        results["depth"] = depth.view(*prefix)
        results["image"] = image.view(*prefix, 3)
        return results

    def _infer_shade(self, xyzs, dirs, ts, ind_code, shading, amp):
        """Field evaluation of one inference round (nerf/renderer.py:779-794): (sigmas | alphas, rgbs)."""
        if not self.opt.sdf and not torch.is_tensor(ind_code) and getattr(self, "_can_fuse", lambda c=None: False)(ind_code):
            # the fused field kernel normalises the ray directions on load (same arithmetic as safe_normalize): four launches fewer per round
            # (ind_code: None, or the fused kernels' IndCode without rows -- code row 0 for every sample)
            with amp:
                sigmas, rgbs, _ = self(xyzs, dirs, ind_code, shading, raw_dirs=True)
            return sigmas, rgbs
        dirs = safe_normalize(dirs)
        with amp:
            sigmas, rgbs, _ = self(xyzs, dirs, ind_code, shading)
        if self.opt.sdf:
            true_cos = -F.relu(-(dirs * safe_normalize(self.normal(xyzs))).sum(-1))
            sigmas = self._sdf_to_alpha(sigmas, true_cos, ts[:, 1])
        return sigmas, rgbs

    def _infer_loop_host(self, rays_o, rays_d, nears, fars, ind_code, shading, dt_gamma, max_steps, T_thresh, perturb, amp,
                         weights_sum, depth, image):
        """The reference's loop as it is written (nerf/renderer.py:764-802): one host read of n_alive per round."""
        N, device = rays_o.shape[0], rays_o.device
        rays_alive = torch.arange(N, dtype=torch.int32, device=device)
        rays_t = nears.clone()
        step = 0
        while step < max_steps:
            n_alive = rays_alive.shape[0]
            if n_alive <= 0:
                break
            n_step = max(min(N // n_alive, 8), 1)
            xyzs, dirs, ts = raymarching.march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, self.real_bound,
                                                    self.opt.contract, self.density_bitfield, self.cascade, self.grid_size, nears,
                                                    fars, perturb if step == 0 else False, dt_gamma, max_steps)
            sigmas, rgbs = self._infer_shade(xyzs, dirs, ts, ind_code, shading, amp)
            raymarching.composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image, T_thresh,
                                       self.opt.sdf)
            rays_alive = raymarching.compact_alive(rays_alive)
            step += n_step

    def _infer_loop_device(self, rays_o, rays_d, nears, fars, ind_code, shading, dt_gamma, max_steps, T_thresh, perturb, amp,
                           weights_sum, depth, image, run_ahead=3):
        """The same loop with the ray count on the device (n2m_*_dev, include/n2m_hip.h): the kernels of a round read {n_alive, step} from
        device memory and derive n_step like the host code above; the host sizes launches from an upper bound of n_alive that reaches it
        through asynchronous copies `run_ahead` rounds late, so no round waits for a read-back (the reference -- and _infer_loop_host --
        drain the queue up to 1024 times per image).  Same per-ray arithmetic: the image is bit-identical as long as the field's per-sample
        results do not depend on the batch size (true of the fused field kernels; BLAS GEMMs may pick another kernel for another M)."""
        from . import _lib as L
        p = L.ptr
        N, device = rays_o.shape[0], rays_o.device
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=device)
        alive = [torch.arange(N, dtype=torch.int32, device=device), i32(N)]
        state = [torch.tensor([N, 0], dtype=torch.int32, device=device), i32(2)]
        rays_t = nears.clone()
        xyzs, dirs = torch.zeros(N, 3, device=device), torch.zeros(N, 3, device=device)
        ts = torch.zeros(N, 2, device=device)
        bits = self.density_bitfield.contiguous()
        noises = torch.rand(N, dtype=torch.float32, device=device) if perturb else None      # first round only (:777)
        host = [torch.empty(2, dtype=torch.int32, pin_memory=True) for _ in range(run_ahead + 1)]
        events = [torch.cuda.Event() for _ in range(run_ahead + 1)]
        pending = []                      # rounds whose next-state copy is in flight: (slot, round index)
        ub, done, rnd = N, False, 0
        while not done:
            # every count that has arrived tightens the bound (and tells when the loop is over); at most run_ahead rounds in flight
            while pending and (len(pending) > run_ahead or events[pending[0]].query()):
                slot = pending.pop(0)
                events[slot].synchronize()
                ub = min(ub, int(host[slot][0]))
                if ub <= 0 or int(host[slot][1]) >= max_steps:
                    done = True
            if done:
                break
            cur, nxt = rnd & 1, (rnd & 1) ^ 1
            s = L.stream()
            m = max(1, min(N, ub * 8))                    # rows any round of <= ub rays can fill: n_alive * n_step <= min(N, 8 n_alive)
            L.call("n2m_march_rays_dev", p(state[cur]), ub, N, p(alive[cur]), p(rays_t), p(rays_o), p(rays_d), float(self.real_bound),
                   int(bool(self.opt.contract)), float(dt_gamma), int(max_steps), int(self.cascade), int(self.grid_size), p(bits), p(fars),
                   p(xyzs), p(dirs), p(ts), p(noises) if rnd == 0 else None, s)
            sigmas, rgbs = self._infer_shade(xyzs[:m], dirs[:m], ts[:m], ind_code, shading, amp)
            sigmas, rgbs = sigmas.float().contiguous(), rgbs.float().contiguous()
            L.call("n2m_composite_rays_dev", p(state[cur]), ub, N, int(max_steps), float(T_thresh), int(bool(self.opt.sdf)), p(alive[cur]),
                   p(rays_t), p(sigmas), p(rgbs), p(ts), p(weights_sum), p(depth), p(image), s)
            L.call("n2m_compact_alive_dev", p(alive[cur]), p(state[cur]), ub, N, int(max_steps), p(alive[nxt]), p(state[nxt]), s)
            slot = rnd % (run_ahead + 1)
            host[slot].copy_(state[nxt], non_blocking=True)
            events[slot].record()
            pending.append(slot)
            rnd += 1
        self.last_infer_rounds = rnd

    def _sdf_to_alpha(self, sdf, cos, dt):
        """NeuS-style alpha from sdf samples (nerf/renderer.py:724-739)."""
        inv_s = torch.exp(self.variance * 10.0).clip(1e-6, 1e6)
        prev_cdf = torch.sigmoid((sdf - cos * dt * 0.5) * inv_s)
        next_cdf = torch.sigmoid((sdf + cos * dt * 0.5) * inv_s)
        return ((prev_cdf - next_cdf + 1e-5) / (prev_cdf + 1e-5)).view(-1).clip(0, 1)

    # ------------------------------------------------------------------------------- occupancy-grid upkeep
    def _cells(self):
        """[H^3,3] fp32 cell coordinates 2*c/(H-1)-1 in Morton order (cell i = morton3D_invert(i))."""
        dev = self.density_bitfield.device
        if self._cell_unit is None or self._cell_unit.device != dev:
            H = self.grid_size
            coords = raymarching.morton3D_invert(torch.arange(H ** 3, dtype=torch.int32, device=dev))
            self._cell_unit = 2 * coords.float() / (H - 1) - 1
        return self._cell_unit

    @torch.no_grad()
    def update_extra_state(self, decay=0.95):
        """Occupancy refresh (nerf/renderer.py:1074-1149): one jittered density sample per cell and cascade,
        grid = max(grid*decay, sample) where both are valid, threshold = min(mean, density_thresh), packbits."""
        if self.opt.stage > 0:
            return
        from . import _lib as L
        _p = L.ptr
        cells = self._cells()
        grid = self.density_grid
        dev = grid.device
        st = getattr(self, "_refresh_bufs", None)
        if st is None or st["tmp"].shape != grid.shape or st["tmp"].device != dev:
            n_part = int(L.lib().n2m_occupancy_update_partials(grid.numel()))
            st = self._refresh_bufs = {"tmp": torch.empty_like(grid), "xyz": torch.empty_like(cells),
                                       "partials": torch.empty(n_part, dtype=torch.float32, device=dev),
                                       "ticket": torch.zeros(1, dtype=torch.int32, device=dev),
                                       "mean": torch.zeros(1, dtype=torch.float32, device=dev), "thresh": torch.zeros(1, dtype=torch.float32, device=dev)}
        tmp_grid, xyzs = st["tmp"], st["xyz"]
        # Cells marked -1 (mark_untrained_grid: outside every camera frustum or the training AABB) are never updated (:1131-1134), so their
        # density is not queried: per cascade the list of the other cells, rebuilt (one host sync) whenever the grid was changed through
        # torch -- marking, a checkpoint load; the update below goes through the raw pointer and leaves the version counter alone.  The
        # random draws still cover ALL cells, so a listed cell gets the point it would have got.  Outdoor recipe: 37 % of 5 x 2 M cells.
        key = (grid.data_ptr(), grid._version)
        if st.get("valid_key") != key:
            st["valid_key"] = key
            st["valid"] = []
            for cas in range(self.cascade):
                idx = torch.nonzero(grid[cas] >= 0).reshape(-1)
                st["valid"].append(None if idx.numel() == grid.shape[1] else (idx.to(torch.int32), idx))
        n_cells = cells.shape[0]
        if any(v is not None for v in st["valid"]):
            tmp_grid.fill_(-1.0)
        # Multi-GPU: the cells to query are dealt to the ranks by MORTON RANGE -- rank r evaluates the r-th slice of every cascade's
        # list -- and the densities are all-gathered (4 bytes per queried cell in all): 1 / W of the query per rank instead of a replicated
        # one.  The jitter is still drawn for every cell from the generator the ranks seeded identically (parallel.sync_rng_for_grid_update),
        # so a cell gets the point it would have got on one GPU and the bit field is the replicated one, bit for bit.
        shard = getattr(self, "refresh_shard", None)
        if shard is not None and shard[1] <= 1:
            shard = None
        if shard is not None:
            # The ranks must hold the SAME list of cells to query, or the gathers below have different shapes on different ranks (a hang or
            # garbage over RCCL).  The decision is made SYMMETRICALLY at every refresh: each rank's summary of its lists -- per cascade
            # (count, index sum), recomputed only when its own list was rebuilt -- is all-gathered (a few dozen bytes) and read on the host;
            # any difference (a rank-local write to density_grid: a checkpoint loaded on rank 0 only, a reset, a mark) puts EVERY rank on
            # the replicated query for this refresh.  One small collective + one host read per 16 steps; no rank ever decides alone.
            from .parallel import all_ranks_hold
            if st.get("summary_key") != key:
                vals = []
                for v in st["valid"]:
                    vals += [-1, 0] if v is None else [int(v[0].numel()), int(v[1].sum())]
                st["summary_key"] = key
                st["summary"] = torch.tensor(vals, dtype=torch.int64, device=dev)
            st["shard_ok"] = all_ranks_hold(st["summary"], shard[1])
            if not st["shard_ok"]:
                shard = None
        for cas in range(self.cascade):
            bound = min(2 ** cas, self.bound)
            hgs = bound / self.grid_size
            idx = st["valid"][cas]
            n = n_cells if idx is None else idx[0].numel()
            u = torch.rand_like(cells)                    # (drawn for every cascade, whether or not any of its cells is valid)
            if n == 0:
                continue
            lo, m = 0, n
            if shard is not None:
                rank, world = shard
                per = (n + world - 1) // world
                lo = min(n, rank * per)
                m = min(n, lo + per) - lo
            sigmas = None
            if m > 0:
                # xyzs = cells * (bound - hgs) + (u * 2 - 1) * hgs: the draws stay torch's, the arithmetic is one launch
                if idx is not None:
                    L.call("n2m_occupancy_points", _p(cells), _p(u), _p(idx[0][lo:lo + m]), float(bound - hgs), float(hgs), _p(xyzs), m, L.stream())
                else:
                    L.call("n2m_occupancy_points", _p(cells[lo:lo + m]), _p(u[lo:lo + m]), None, float(bound - hgs), float(hgs), _p(xyzs), m, L.stream())
                with torch.autocast(device_type="cuda", dtype=torch.float16, enabled=bool(self.opt.fp16)):
                    sigmas = self.density(xyzs[:m])["sigma"].reshape(-1).detach()
                    if self.opt.sdf:
                        inv_s = torch.exp(self.variance * 10.0).clip(1e-6, 1e6)
                        sigmas = torch.sigmoid(-sigmas * inv_s) * inv_s
                sigmas = sigmas.float()
            if shard is not None:
                import torch.distributed as dist
                gath = st.get("gather")
                if gath is None or gath.numel() < per * world:
                    gath = st["gather"] = torch.empty(per * world, dtype=torch.float32, device=dev)
                mine = gath[rank * per:(rank + 1) * per]
                if m > 0:
                    mine[:m].copy_(sigmas)
                # (RCCL gathers in place; gloo -- the CPU / shared-GPU tests -- gets a copy of the slice)
                dist.all_gather_into_tensor(gath[:per * world], mine if dist.get_backend() == "nccl" else mine.clone())
                sigmas = gath[:n]                         # slices are full except the last non-empty one: the first n values are the list, in order
            if idx is None:
                tmp_grid[cas] = sigmas
            else:
                tmp_grid[cas].index_copy_(0, idx[1], sigmas)
        # grid = max(grid * decay, sample) where both are valid; mean of max(grid, 0); threshold = min(mean, density_thresh): one launch, and
        # both scalars stay on the device (the reference reads the mean back every refresh, :1142): no queue drain
        L.call("n2m_occupancy_update", _p(grid), _p(tmp_grid), float(decay), grid.numel(), float(self.density_thresh), _p(st["partials"]),
               _p(st["ticket"]), _p(st["mean"]), _p(st["thresh"]), L.stream())
        self._mean_density_t = st["mean"]
        self.iter_density += 1
        self.density_bitfield = raymarching.packbits(grid, st["thresh"], self.density_bitfield)

    @torch.no_grad()
    def mark_untrained_grid(self, poses, intrinsics, cam_near_far=None, S=64):
        """Marks cells no training camera sees, or that lie outside aabb_train, with -1 (nerf/renderer.py:985-1071).
        poses [B,4,4] cam2world, intrinsics (fx, fy, cx, cy), or [B,4] of them (a set with per-view intrinsics, capture.Capture.intrinsics):
        cx / fx and cy / fy are then a column per camera of the chunk -- the quotient taken in float64 and rounded to fp32 once, as the
        tuple form's is -- and the expression is otherwise the same."""
        dev = self.density_grid.device
        poses = poses.to(dev)
        B = poses.shape[0]
        per_view = getattr(intrinsics, "ndim", 1) == 2            # a tensor or an array [B,4]; the tuple form has no ndim
        if per_view:
            k = torch.as_tensor(intrinsics).to(dev).double()
            if tuple(k.shape) != (B, 4):
                raise ValueError(f"per-view intrinsics must be [{B},4], not {tuple(k.shape)}")
            rx, ry = (k[:, 2] / k[:, 0]).float().unsqueeze(1), (k[:, 3] / k[:, 1]).float().unsqueeze(1)      # [B,1]
        else:
            fx, fy, cx, cy = intrinsics
        cells = self._cells().unsqueeze(0)                    # [1,N,3]; already Morton-ordered
        mask_cam = torch.zeros_like(self.density_grid)
        mask_aabb = torch.zeros_like(self.density_grid)
        for cas in range(self.cascade):
            bound = min(2 ** cas, self.bound)
            hgs = bound / self.grid_size
            pts = cells * (bound - hgs)
            inside = ((pts >= (self.aabb_train[:3] - hgs)).all(-1) & (pts <= (self.aabb_train[3:] + hgs)).all(-1)).reshape(-1)
            mask_aabb[cas] += inside
            for head in range(0, B, S):
                tail = min(head + S, B)
                cam = pts - poses[head:tail, :3, 3].unsqueeze(1)
                cam = cam @ poses[head:tail, :3, :3]
                z = -cam[:, :, 2]
                near = self.opt.min_near if cam_near_far is None else cam_near_far[head:tail, 0].unsqueeze(1)
                if per_view:
                    seen = (z > near) & (cam[:, :, 0].abs() < rx[head:tail] * z + hgs * 2) & (cam[:, :, 1].abs() < ry[head:tail] * z + hgs * 2)
                else:
                    seen = (z > near) & (cam[:, :, 0].abs() < cx / fx * z + hgs * 2) & (cam[:, :, 1].abs() < cy / fy * z + hgs * 2)
                mask_cam[cas] += seen.any(0)
        self.density_grid[(mask_cam == 0) | (mask_aabb == 0)] = -1


    # ------------------------------------------------------------------------------------- stage-0 mesh export
    @torch.no_grad()
    def density_volume(self, resolution, S=128, scale=1.0):
        """[R,R,R] fp32 density at linspace(-1, 1, R)^3 * scale, queried in S^3 blocks like nerf/renderer.py:493-506 (one block for R <= S)."""
        dev = self.density_bitfield.device
        sigmas = torch.zeros([resolution] * 3, dtype=torch.float32, device=dev)
        axis = (torch.linspace(-1, 1, resolution, device=dev) * scale).split(S)
        for xi, xs in enumerate(axis):
            for yi, ys in enumerate(axis):
                for zi, zs in enumerate(axis):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], dim=-1).contiguous()
                    with torch.autocast(device_type="cuda", dtype=torch.float16, enabled=bool(self.opt.fp16)):
                        val = self.density(pts)["sigma"]
                    sigmas[xi * S:xi * S + len(xs), yi * S:yi * S + len(ys), zi * S:zi * S + len(zs)] = val.reshape(len(xs), len(ys), len(zs)).float()
        return sigmas

    def _grid_as_volume(self, cas):
        """density_grid[cas] (Morton order) as a [H,H,H] volume indexed [x,y,z] (nerf/renderer.py:487-489)."""
        H = self.grid_size
        coords = raymarching.morton3D_invert(torch.arange(H ** 3, dtype=torch.int32, device=self.density_grid.device)).long()
        vol = torch.zeros([H] * 3, dtype=torch.float32, device=self.density_grid.device)
        vol[coords[:, 0], coords[:, 1], coords[:, 2]] = self.density_grid[cas]
        return vol

    @torch.no_grad()
    def export_stage0(self, save_path, resolution=None, decimate_target=1e5, dataset=None, S=128, decimate=False, clean=False,
                      method="density", tsdf=None):
        """Stage-0 mesh extraction (nerf/renderer.py:472-672): density volume -> marching cubes -> mesh_{cas}.ply.  The volume never leaves
        the device: the reference copies it to the host for PyMCubes (:518); here marching cubes is a HIP kernel (marching_cubes.py).
        clean=True runs the device clean_mesh of mesh_clean.py where the reference runs pymeshlab's (merging close vertices, removing
        duplicate / null faces and floaters, repairing non-manifold geometry): on the inner mesh after its visibility filter with
        repair=True (:537), on each outer cascade after the out-of-AABB removal with repair=False, skipping a cascade it empties
        (:653-655); min_f / min_d are opt.clean_min_f / clean_min_d.  decimate=True honours `decimate_target` where the reference does,
        with the device decimation of mesh_simplify.py: the inner mesh after its visibility filter (and cleaning) to `decimate_target` faces
        with optimal placement (:540-541), the outer cascades to `decimate_target // 2` without it, before their visibility filter
        (:582-583, :658-659).  With neither (the default) the raw iso-surfaces are written.
        SDF recipe with bound > 1 (the contracted background, :548-601): the outer shell mesh_1.ply.  The field is queried at
        2 * linspace(-1, 1, R)^3 (contracted coordinates, R = resolution), nan_to_num, marching cubes of -sdf at 0; the vertices with all
        |x| <= 0.5 (the unit box, which mesh_0 covers) go, the rest is scaled by 2 - 2 / R, cleaned (clean=True, repair=False), decimated to
        2 * decimate_target faces without optimal placement (decimate=True, when it has more), brought back to world space by
        `uncontract`, cut at aabb_train (any coordinate <= lo or >= hi goes) and visibility-filtered (dataset).  The lattice is queried
        whatever resolution == grid_size is: the reference reuses the X, Y, Z of its lattice branch there and raises a NameError when
        that branch did not run.  A shell that any removal empties is skipped -- no file, no key, like an emptied density-mode cascade --
        and stage 1 then has ONE cascade: its loader (export.load_stage0_meshes) stops at the first missing mesh_{cas}.ply.
        dataset: object with `.mvps [B,4,4]`, `.H`, `.W` for the visibility test, or None.
        method="tsdf" (not a reference path; the default "density" is the path above, untouched): the inner mesh's volume and marching
        cubes are replaced by TSDF fusion (tsdf.py) -- the field's inference render gives a depth map at every view of
        `dataset`, which must be a capture.Capture then; the maps are fused into a TSDFVolume(resolution) on the unit box and its zero
        level set, minus what no view observed, goes on through the visibility filter, cleaning, decimation and the PLY as before.  The
        outer cascades of bound > 1 still come from the occupancy grid.  tsdf: a dict of TSDFVolume's (trunc, w_max, min_depth),
        surface_depth's (alpha_min, carve, alpha_carve) and fuse_views' (chunk) keywords.  The SDF recipe already meshes a signed distance:
        opt.sdf with method="tsdf" raises ValueError.
        Returns {cascade: (vertices [V,3] f32, triangles [F,3] i32)} (device tensors)."""
        import os
        from . import export
        from .marching_cubes import marching_cubes
        from .mesh_clean import clean_mesh
        from .mesh_simplify import decimate as decimate_mesh
        if method not in ("density", "tsdf"):
            raise ValueError(f"export_stage0: method must be 'density' or 'tsdf', got {method!r}")
        if method == "tsdf":
            from .capture import Capture
            if self.opt.sdf:
                raise ValueError("export_stage0: method='tsdf' is for the density recipe; the SDF recipe (opt.sdf) already meshes a signed distance")
            if not isinstance(dataset, Capture):
                raise ValueError("export_stage0: method='tsdf' renders a depth map at every training camera and needs dataset=<capture.Capture>")
        dec_target = int(decimate_target) if decimate and decimate_target > 0 else 0     # 0: no decimation
        os.makedirs(save_path, exist_ok=True)
        dev = self.density_bitfield.device
        if resolution is None:
            resolution = self.grid_size
        density_thresh = min(self.mean_density, self.density_thresh)
        if method == "tsdf":
            vertices, triangles = self._tsdf_inner_mesh(resolution, dataset, tsdf)
        else:
            if resolution == self.grid_size:
                sigmas = self._grid_as_volume(0)
            else:
                sigmas = self.density_volume(resolution, S)
                if not self.opt.sdf:      # the occupancy grid as a baseline mask (also excludes untrained regions), :509-516
                    mask = F.interpolate(self._grid_as_volume(0)[None, None], size=[resolution] * 3, mode="nearest")[0, 0]
                    sigmas = sigmas * (mask > density_thresh)
            sigmas = torch.nan_to_num(sigmas, 0)
            if self.opt.sdf:
                vertices, triangles = marching_cubes(-sigmas, 0.0, div=resolution - 1.0, mul=2.0, add=-1.0)
            else:
                vertices, triangles = marching_cubes(sigmas, density_thresh, div=resolution - 1.0, mul=2.0, add=-1.0)
        if dataset is not None and triangles.shape[0] > 0:
            unseen = self.mark_unseen_triangles(vertices, triangles, dataset.mvps, dataset.H, dataset.W)
            vertices, triangles = export.remove_faces(vertices, triangles, unseen, dilation=getattr(self.opt, "visibility_mask_dilation", 5))
        if clean:
            vertices, triangles, _ = clean_mesh(vertices, triangles, min_f=self.opt.clean_min_f, min_d=self.opt.clean_min_d, repair=True)
        if dec_target and triangles.shape[0] > dec_target:
            vertices, triangles, _ = decimate_mesh(vertices, triangles, dec_target, optimal_placement=True)
        meshes = {0: (vertices, triangles)}
        export.write_ply(os.path.join(save_path, "mesh_0.ply"), vertices.cpu().numpy(), triangles.cpu().numpy())
        if self.bound > 1 and not self.opt.sdf:
            # outer cascades from the occupancy grid itself (:603-672): trilinear resample to env_reso, binarise, iso 0.5, drop the centre
            # that the inner cascades cover and everything outside aabb_train
            target = int(getattr(self.opt, "env_reso", 256))
            for cas in range(1, self.cascade):
                bound = min(2 ** cas, self.bound)
                hgs = bound / target
                occ = F.interpolate(self._grid_as_volume(cas)[None, None], [target] * 3, mode="trilinear")[0, 0]
                occ = (torch.nan_to_num(occ, 0) > density_thresh).float()
                v, t = marching_cubes(occ, 0.5, div=target - 1.0, mul=2.0, add=-1.0)
                r = 0.45
                v, t = export.remove_vertices(v, t, (v.abs() <= r).all(dim=1))
                if v.shape[0] == 0:
                    continue
                v = v * (bound - hgs)
                lo, hi = self.aabb_train[:3] + hgs, self.aabb_train[3:] - hgs
                v, t = export.remove_vertices(v, t, ((v <= lo) | (v >= hi)).any(dim=1))
                if v.shape[0] == 0:
                    continue
                if clean:
                    v, t, _ = clean_mesh(v, t, min_f=self.opt.clean_min_f, min_d=self.opt.clean_min_d, repair=False)
                    if v.shape[0] == 0:
                        continue
                if dec_target and t.shape[0] > dec_target // 2:
                    v, t, _ = decimate_mesh(v, t, dec_target // 2, optimal_placement=False)
                if dataset is not None and t.shape[0] > 0:
                    unseen = self.mark_unseen_triangles(v, t, dataset.mvps, dataset.H, dataset.W)
                    v, t = export.remove_faces(v, t, unseen, dilation=getattr(self.opt, "visibility_mask_dilation", 5))
                meshes[cas] = (v, t)
                export.write_ply(os.path.join(save_path, f"mesh_{cas}.ply"), v.cpu().numpy(), t.cpu().numpy())
        elif self.bound > 1:
            shell = self._sdf_outer_shell(resolution, S, dec_target, dataset, clean)
            if shell is not None:
                meshes[1] = shell
                export.write_ply(os.path.join(save_path, "mesh_1.ply"), shell[0].cpu().numpy(), shell[1].cpu().numpy())
        return meshes

    def _tsdf_inner_mesh(self, resolution, capture, kw):
        """The inner mesh of export_stage0(method="tsdf"): the inference render's depth at every view of `capture`, fused into a
        TSDFVolume(resolution) on the unit box (tsdf.fuse_views), and its zero level set (TSDFVolume.extract).  kw: the keywords of
        TSDFVolume, surface_depth and fuse_views, told apart by name."""
        from . import tsdf as T
        from .metrics import field_renderer
        kw = dict(kw or {})
        unknown = set(kw) - {"trunc", "w_max", "min_depth", "alpha_min", "carve", "alpha_carve", "chunk"}
        if unknown:
            raise ValueError(f"export_stage0: unknown tsdf option(s) {sorted(unknown)}")
        vol_kw = {k: kw.pop(k) for k in ("trunc", "w_max", "min_depth") if k in kw}
        was_training = self.training
        volume = T.TSDFVolume(int(resolution), device=self.density_bitfield.device, **vol_kw)
        try:
            T.fuse_views(field_renderer(self, capture), capture, volume, **kw)
        finally:
            self.train(was_training)            # field_renderer puts the model into eval mode
        return volume.extract()

    def _sdf_outer_shell(self, resolution, S, dec_target, dataset, clean):
        """The contracted background of the SDF recipe as a world-space mesh (nerf/renderer.py:548-601, in its order), or None when a
        removal leaves nothing.  dec_target: the inner mesh's face target (0: no decimation); the shell's is twice that (:581)."""
        from . import export
        from .marching_cubes import marching_cubes
        from .mesh_clean import clean_mesh
        from .mesh_simplify import decimate as decimate_mesh
        sigmas = torch.nan_to_num(self.density_volume(resolution, S, scale=2.0), 0)
        v, t = marching_cubes(-sigmas, 0.0, div=resolution - 1.0, mul=2.0, add=-1.0)
        r = 0.5
        v, t = export.remove_vertices(v, t, (v.abs() <= r).all(dim=1))
        if v.shape[0] == 0:
            return None
        bound = 2
        v = v * (bound - bound / resolution)
        if clean:
            v, t, _ = clean_mesh(v, t, min_f=self.opt.clean_min_f, min_d=self.opt.clean_min_d, repair=False)
            if v.shape[0] == 0:
                return None
        if dec_target and t.shape[0] > 2 * dec_target:
            v, t, _ = decimate_mesh(v, t, 2 * dec_target, optimal_placement=False)
        v = uncontract(v.float().contiguous())
        lo, hi = self.aabb_train[:3], self.aabb_train[3:]
        v, t = export.remove_vertices(v, t, ((v <= lo) | (v >= hi)).any(dim=1))
        if v.shape[0] == 0:
            return None
        if dataset is not None and t.shape[0] > 0:
            unseen = self.mark_unseen_triangles(v, t, dataset.mvps, dataset.H, dataset.W)
            v, t = export.remove_faces(v, t, unseen, dilation=getattr(self.opt, "visibility_mask_dilation", 5))
            if v.shape[0] == 0:
                return None
        return v, t

    # ------------------------------------------------------------------------------------------ stage 1
    @torch.no_grad()
    def refine_and_decimate(self, save_path=None, remesh=False, remesh_project=False):
        """Stage-1 mesh refinement (nerf/renderer.py:209-294, meshutils.py:191-231) on the device.  The accumulated per-face errors,
        averaged by their counts, classify the seen faces of the inner mesh: above the 90th percentile -> 2 (subdivide), below the 50th
        -> 1 (decimate), numpy.percentile's linear rule; SDF: every face is 1.  Cascade 0 is decimated on the class-1 faces
        (selected-only target int((1 - refine_decimate_ratio) * n1), classes carried through), then midpoint-subdivided on the class-2
        faces at `refine_size`; the other cascades are copied and v_cumsum / f_cumsum rebuilt.  Offsets and error accumulators restart
        at zero on the new mesh; with `save_path`, mesh_{cas}_updated.ply is written.  Returns the counts before / after, and the class-1
        faces before ("decimate") and after the decimation ("decimate_after").
        No seen face: the mesh is left as it is ("changed": False).
        remesh=True (opt-in; the default leaves this method as it was): with `opt.refine_remesh_size` > 0, the class-1 faces are
        re-meshed isotropically towards that edge length between the decimation and the subdivision
        (mesh_remesh.remesh_isotropic, 3 iterations, selected-only: meshutils.py:208-209), the classes carried through its face sources,
        and the result reports "remesh": {"faces_before", "faces_after"}.  It is the project's own rule for the published algorithm
        (DESIGN 4.14), not MeshLab's vertex positions.  remesh_project=True passes project=True on: every relaxed vertex is brought back
        onto the mesh the re-meshing started from (MeshLab's `reprojectflag`), and "remesh" also reports "projected", the
        vertices projected per iteration.
        Differences: the non-manifold repairs after the re-meshing (:212-213; the device passes keep a manifold input manifold) are not
        done, and without `remesh` neither is the re-meshing."""
        from .mesh_simplify import decimate, subdivide_midpoint
        opt = self.opt
        dev = self.vertices.device
        v_all = (self.vertices + self.vertices_offsets).detach().float().contiguous()
        f_all = self.triangles.int()
        n_inner = self.f_cumsum[1]
        before = {"vertices": int(v_all.shape[0]), "faces": int(f_all.shape[0])}
        err = self.triangles_errors[:n_inner].float()
        cnt = self.triangles_errors_cnt[:n_inner].float()
        seen = cnt > 0
        err = torch.where(seen, err / torch.where(seen, cnt, torch.ones_like(cnt)), err)
        if opt.sdf:
            mask = torch.ones(n_inner, dtype=torch.uint8, device=dev)
        else:
            e = err[seen]
            if e.numel() == 0:
                return {"changed": False, "before": before, "after": before, "decimate": 0, "decimate_after": 0, "refine": 0}
            t_ref, t_dec = percentile_linear(e, 90), percentile_linear(e, 50)
            mask = torch.zeros(n_inner, dtype=torch.uint8, device=dev)
            mask[(err > t_ref) & seen] = 2
            mask[(err < t_dec) & seen] = 1
        n_dec, n_ref = int((mask == 1).sum()), int((mask == 2).sum())
        n_dec_after = n_dec
        remeshed = None
        meshes = []
        for cas in range(len(self.v_cumsum) - 1):
            v = v_all[self.v_cumsum[cas]:self.v_cumsum[cas + 1]].contiguous()
            f = (f_all[self.f_cumsum[cas]:self.f_cumsum[cas + 1]] - self.v_cumsum[cas]).contiguous()
            if cas == 0:
                if opt.refine_decimate_ratio > 0 and n_dec:
                    v, f, src = decimate(v, f, int((1 - opt.refine_decimate_ratio) * n_dec), optimal_placement=True, selected=mask == 1)
                    mask = mask[src]
                    n_dec_after = int((mask == 1).sum())
                if remesh and opt.refine_remesh_size > 0 and n_dec_after:
                    from .mesh_remesh import remesh_isotropic
                    remeshed = {"faces_before": int(f.shape[0])}
                    if remesh_project:
                        rstats = {}
                        v, f, src = remesh_isotropic(v, f, opt.refine_remesh_size, iterations=3, selected=mask == 1, stats=rstats, project=True)
                        remeshed["projected"] = [it["projected"] for it in rstats["iterations"]]
                    else:
                        v, f, src = remesh_isotropic(v, f, opt.refine_remesh_size, iterations=3, selected=mask == 1)
                    mask = mask[src]
                    remeshed["faces_after"] = int(f.shape[0])
                if opt.refine_size > 0 and n_ref:
                    v, f = subdivide_midpoint(v, f, opt.refine_size, selected=mask == 2)
            meshes.append((v, f))
        if save_path is not None:
            from . import export
            os.makedirs(save_path, exist_ok=True)
            for cas, (v, f) in enumerate(meshes):
                export.write_ply(os.path.join(save_path, f"mesh_{cas}_updated.ply"), v.cpu().numpy(), f.cpu().numpy())
        v_cumsum, f_cumsum = [0], [0]
        for v, f in meshes:
            v_cumsum.append(v_cumsum[-1] + int(v.shape[0]))
            f_cumsum.append(f_cumsum[-1] + int(f.shape[0]))
        self.vertices = torch.cat([v for v, _ in meshes]).contiguous()
        self.triangles = torch.cat([f + v0 for (_, f), v0 in zip(meshes, v_cumsum)]).to(torch.int32).contiguous()
        self.v_cumsum, self.f_cumsum = v_cumsum, f_cumsum
        self.vertices_offsets = nn.Parameter(torch.zeros_like(self.vertices))
        self.triangles_errors = torch.zeros(self.triangles.shape[0], dtype=torch.float32, device=dev)
        self.triangles_errors_cnt = torch.zeros(self.triangles.shape[0], dtype=torch.float32, device=dev)
        self.triangles_errors_id = None
        after = {"vertices": int(self.vertices.shape[0]), "faces": int(self.triangles.shape[0])}
        out = {"changed": True, "before": before, "after": after, "decimate": n_dec, "decimate_after": n_dec_after, "refine": n_ref}
        if remeshed is not None:
            out["remesh"] = remeshed
        return out

    def init_stage1(self, vertices, triangles, v_cumsum=None, f_cumsum=None):
        """Attach the stage-0 mesh (what NeRFRenderer.__init__ loads from mesh_stage0/*.ply, nerf/renderer.py:123-165):
        vertices [V,3] f32, triangles [F,3] int32, learnable per-vertex offsets, per-face error accumulators."""
        dev = self.density_bitfield.device
        self.glctx = dr.RasterizeGLContext(output_db=False)
        self.vertices = vertices.float().to(dev).contiguous()
        self.triangles = triangles.int().to(dev).contiguous()
        self.v_cumsum = [int(x) for x in v_cumsum] if v_cumsum is not None else [0, self.vertices.shape[0]]
        if f_cumsum is None:
            # cascades are concatenated in order and a cascade's faces only name its own vertices (nerf/renderer.py:143-150): the face
            # ranges follow from the vertex ranges (number of faces whose first vertex lies below each vertex bound)
            first = self.triangles[:, 0].long()
            f_cumsum = [0] + [int((first < b).sum()) for b in self.v_cumsum[1:]]
        self.f_cumsum = [int(x) for x in f_cumsum]
        assert len(self.f_cumsum) == len(self.v_cumsum) and self.f_cumsum[-1] == self.triangles.shape[0]
        self.vertices_offsets = nn.Parameter(torch.zeros_like(self.vertices))
        self.triangles_errors = torch.zeros(self.triangles.shape[0], dtype=torch.float32, device=dev)
        self.triangles_errors_cnt = torch.zeros(self.triangles.shape[0], dtype=torch.float32, device=dev)
        self.triangles_errors_id = None

    @torch.no_grad()
    def bake_textures(self, v, f, vt, ft, h0, w0, ssaa=1, pad=32):
        """The texture bake of nerf/renderer.py:324-397 for one mesh: rasterise the atlas (uv -> clip space), interpolate the surface
        position of every covered texel, evaluate geo_feat there (6 channels: diffuse + specular features), quantise to uint8, fill the
        band around the charts from the nearest chart-boundary texel, reduce by `ssaa`.  Everything up to the two uint8 images stays on
        the device: the reference's host kd-tree search is a ring walk per band texel (csrc/texture.hip).
        v [V,3], f [F,3] int32, vt [T,2] in [0,1], ft [F,3] int32 -> (feat0 [h0,w0,3] uint8, feat1 [h0,w0,3] uint8, mask [h,w] bool)."""
        from . import _lib as L
        dev = v.device
        h, w = (int(h0 * ssaa), int(w0 * ssaa)) if ssaa > 1 else (h0, w0)
        uv = vt.float() * 2.0 - 1.0
        uv = torch.cat((uv, torch.zeros_like(uv[..., :1]), torch.ones_like(uv[..., :1])), dim=-1).contiguous()
        ctx = self.glctx or dr.RasterizeGLContext(output_db=False)
        rast, _ = dr.rasterize(ctx, uv.unsqueeze(0), ft.int().contiguous(), (h, w))
        xyzs, _ = dr.interpolate(v.float().unsqueeze(0).contiguous(), rast, f.int().contiguous())
        mask = (rast[..., 3] > 0).view(-1)        # == (interpolate(ones) > 0) of :333-338: a covered texel's barycentrics sum to one
        xyzs = xyzs.view(-1, 3)
        if self.opt.contract:
            xyzs = contract(xyzs)
        feats = torch.zeros(h * w, 6, device=dev, dtype=torch.float32)
        idx = torch.nonzero(mask, as_tuple=False).squeeze(1)
        ind_code = self.individual_codes[[0]] if self.individual_dim > 0 else None
        for head in range(0, idx.numel(), 640000):
            sel = idx[head:head + 640000]
            with torch.autocast(device_type="cuda", dtype=torch.float16, enabled=bool(self.opt.fp16)):
                feats[sel] = self.geo_feat(xyzs[sel].contiguous(), ind_code).float()
        q = (feats * 255).to(torch.uint8).view(h, w, 6).contiguous()          # (feats * 255).astype(np.uint8): truncation (:366)
        m = mask.view(h, w)
        # band = 32 steps of 4-neighbour dilation minus the charts; sources = the charts minus their 3-step erosion (:371-377;
        # scipy's default structuring element is the cross, the outside of the image counts as empty)
        band = m
        for _ in range(int(pad)):
            band = dilate_cross(band)
        band = band & ~m
        core = m
        for _ in range(3):
            core = erode_cross(core)
        ring = m & ~core
        role = (ring.to(torch.uint8) | (band.to(torch.uint8) << 1)).contiguous()
        if bool(ring.any()):
            L.call("n2m_texture_pad_nearest", L.ptr(q), L.ptr(role), h, w, 6, int(pad), L.stream())
        if ssaa > 1:      # cv2.resize(..., INTER_LINEAR) of :393-395; here bilinear on the device, rounded to nearest
            x = q.permute(2, 0, 1).float().unsqueeze(0)
            x = F.interpolate(x, size=(h0, w0), mode="bilinear", align_corners=False)
            q = x[0].permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8)
        return q[..., :3].contiguous(), q[..., 3:].contiguous(), m

    @torch.no_grad()
    def export_stage1(self, path, h0=2048, w0=2048, atlas=None):
        """nerf/renderer.py:298-468: per cascade `mesh_{cas}.obj/.mtl`, `feat0_{cas}.jpg` (diffuse), `feat1_{cas}.jpg` (specular
        features), and `mlp.json` -- the files renderer.html loads.  atlas: {cas: (vt [T,2] in [0,1], ft [F,3])}, or "charts": every
        cascade is unwrapped on the device by uv_atlas.uv_atlas at its own (h0 * ssaa, w0 * ssaa) -- of contract(v) when opt.contract is
        set, as the reference's xatlas call sees it (:312-322) --; None: every face gets its own cell (export.grid_atlas, the stand-in).
        self.last_atlas keeps {cas: (vt, ft, vmapping-or-None)} of the call."""
        import os
        from . import export
        assert self.opt.stage > 0, "export_stage1 needs the stage-1 mesh (init_stage1)"
        if isinstance(atlas, str):
            if atlas != "charts":
                raise ValueError(f"export_stage1: atlas must be None, a dict or \"charts\", got {atlas!r}")
            from .uv_atlas import uv_atlas
        self.last_atlas = {}
        os.makedirs(path, exist_ok=True)
        v_all = (self.vertices + self.vertices_offsets).detach()
        f_all = self.triangles.detach()
        ssaa = int(getattr(self.opt, "ssaa", 1))
        out = {}
        for cas in range(len(self.v_cumsum) - 1):
            v = v_all[self.v_cumsum[cas]:self.v_cumsum[cas + 1]].contiguous()
            f = (f_all[self.f_cumsum[cas]:self.f_cumsum[cas + 1]] - self.v_cumsum[cas]).contiguous()
            if f.shape[0] > 0:       # (an empty cascade writes nothing but still takes part in the halving below, nerf/renderer.py:440-448)
                vmapping = None
                if isinstance(atlas, str):
                    vt, ft, vmapping = uv_atlas(contract(v) if self.opt.contract else v, f, int(h0 * ssaa), int(w0 * ssaa))
                else:
                    vt, ft = atlas[cas] if atlas is not None else export.grid_atlas(f.shape[0], device=v.device)
                vt, ft = torch.as_tensor(vt).float().to(v.device), torch.as_tensor(ft).int().to(v.device)
                feat0, feat1, mask = self.bake_textures(v, f, vt, ft, h0, w0, ssaa)
                export.write_jpg(os.path.join(path, f"feat0_{cas}.jpg"), feat0.cpu().numpy())
                export.write_jpg(os.path.join(path, f"feat1_{cas}.jpg"), feat1.cpu().numpy())
                export.write_obj(path, cas, v.cpu().numpy(), f.cpu().numpy(), vt.cpu().numpy(), ft.cpu().numpy())
                out[cas] = (feat0, feat1, mask)
                self.last_atlas[cas] = (vt, ft, vmapping)
            if not self.opt.sdf and h0 > 2048 and w0 > 2048:      # half the texture resolution for the remote cascades (:446-448)
                h0 //= 2
                w0 //= 2
        export.write_mlp_json(os.path.join(path, "mlp.json"), self)
        return out

    def stage1_dirs(self, rays_d, h0, w0):
        """Unit view directions per rendered pixel (nerf/renderer.py:821-828: nearest upscale to the ssaa resolution, safe_normalize): a
        function of the view alone, so a trainer that keeps its views resident may keep this too (Stage1Trainer does)."""
        rays_d = rays_d.contiguous().view(-1, 3)
        ssaa = int(self.opt.ssaa)
        if ssaa > 1:
            h, w = int(h0 * ssaa), int(w0 * ssaa)
            rays_d = F.interpolate(rays_d.view(1, h0, w0, 3).permute(0, 3, 1, 2), (h, w), mode="nearest").permute(0, 2, 3, 1).reshape(-1, 3).contiguous()
        return safe_normalize(rays_d)

    def _stage1_front(self, rays_d, mvp, h0, w0, shading="full", dirs=None, packed=False, vertices=None, index=None):
        """Everything of render_stage1 up to and including the two antialias calls (nerf/renderer.py:816-887): returns
        (rast [1,h,w,4], alpha [1,h,w,1] and rgb [1,h,w,3] as antialias hands them out, BEFORE the clamp).  dirs: stage1_dirs(rays_d, h0, w0)
        when the caller has it already.  packed: ONE antialias call on the [1,h,w,4] image RGB + alpha instead of the reference's two (the
        silhouette blend works per channel: same values, one pass over the edges each way instead of two) -- returns (rast, None, rgba)."""
        device = rays_d.device
        ssaa = int(self.opt.ssaa)
        h, w = (int(h0 * ssaa), int(w0 * ssaa)) if ssaa > 1 else (h0, w0)
        if dirs is None:
            dirs = self.stage1_dirs(rays_d, h0, w0)
        if vertices is None:          # (a caller that needs them elsewhere -- the trainer's smoothness loss -- passes its own sum in)
            vertices = self.vertices + self.vertices_offsets
        vertices_clip = to_clip(vertices, mvp).unsqueeze(0)
        rast, _ = dr.rasterize(self.glctx, vertices_clip, self.triangles, (h, w))
        xyzs, _ = dr.interpolate(vertices.unsqueeze(0), rast, self.triangles)
        mask, _ = dr.interpolate(torch.ones_like(vertices[:, :1]).unsqueeze(0), rast, self.triangles)
        mask_flatten = (mask > 0).view(-1).detach()
        xyzs = xyzs.view(-1, 3)
        if self.opt.contract:
            xyzs = contract(xyzs)
        idx = torch.nonzero(mask_flatten, as_tuple=False).squeeze(1)
        self.last_covered = int(idx.numel())
        # individual codes (nerf/renderer.py:850): the trained view's row while training, row 0 otherwise -- one row for every covered pixel
        ind_code = None
        if self.individual_dim > 0 and hasattr(self, "ind_code"):
            row = int(index) if (self.training and index is not None) else None
            ind_code = self.ind_code(None if row is None else torch.full((int(idx.numel()),), row, dtype=torch.int32, device=device))
        if idx.numel() > 0 and xyzs.is_cuda:
            # (the boolean-mask gather / scatter of :875-881 over the index list: torch's index kernels take 50 us per call on 0.7 M rows)
            from .losses import gather_rows, scatter_rows
            pts = gather_rows(xyzs if self.opt.enable_offset_nerf_grad else xyzs.detach(), idx)
            with torch.autocast(device_type="cuda", dtype=torch.float16, enabled=bool(self.opt.fp16)):
                mask_rgbs, _ = self.rgb(pts, gather_rows(dirs, idx), ind_code, shading)
            if packed:
                rgba = scatter_rows(torch.cat([mask_rgbs.float(), gather_rows(mask.view(-1, 1), idx)], dim=1), idx, h * w).view(1, h, w, 4)
                return rast, None, dr.antialias(rgba, rast, vertices_clip, self.triangles, pos_gradient_boost=self.opt.pos_gradient_boost)
            rgbs = scatter_rows(mask_rgbs, idx, h * w)
        else:
            rgbs = torch.zeros(h * w, 3, device=device, dtype=torch.float32)
            if idx.numel() > 0:
                pts = xyzs[idx] if self.opt.enable_offset_nerf_grad else xyzs[idx].detach()
                mask_rgbs, _ = self.rgb(pts, dirs[idx], ind_code, shading)
                rgbs = rgbs.index_copy(0, idx, mask_rgbs.float())
        rgbs = rgbs.view(1, h, w, 3)
        alphas = mask.float()
        boost = self.opt.pos_gradient_boost
        alphas = dr.antialias(alphas, rast, vertices_clip, self.triangles, pos_gradient_boost=boost)
        rgbs = dr.antialias(rgbs, rast, vertices_clip, self.triangles, pos_gradient_boost=boost)
        return rast, alphas, rgbs

    def render_stage1(self, rays_o, rays_d, mvp, h0, w0, index=None, bg_color=None, shading="full", **kwargs):
        """Rasterise the mesh, shade covered pixels with the colour networks, antialias (nerf/renderer.py:816-921)."""
        prefix = rays_d.shape[:-1]
        ssaa = int(self.opt.ssaa)
        h, w = (int(h0 * ssaa), int(w0 * ssaa)) if ssaa > 1 else (h0, w0)
        if bg_color is None:
            bg_color = 1
        if torch.is_tensor(bg_color) and bg_color.dim() == 2:
            bg_color = bg_color.view(h0, w0, 3)
        rast, alphas, rgbs = self._stage1_front(rays_d, mvp, h0, w0, shading, index=index)
        alphas = alphas.squeeze(0).clamp(0, 1)
        rgbs = rgbs.squeeze(0).clamp(0, 1)
        image = alphas * rgbs
        depth = alphas * rast[0, :, :, [2]]
        T = 1 - alphas
        trig_id = rast[0, :, :, -1] - 1
        if ssaa > 1:
            def down(x):   # bilinear minification like scale_img_hwc (nerf/renderer.py:46-65)
                return F.interpolate(x.permute(2, 0, 1).unsqueeze(0), (h0, w0), mode="bilinear").squeeze(0).permute(1, 2, 0).contiguous()
            image, depth, T = down(image), down(depth), down(T)
            trig_id = F.interpolate(trig_id.view(1, 1, h, w), (h0, w0), mode="nearest").view(h0, w0)
        self.triangles_errors_id = trig_id
        image = image + T * bg_color
        # (weights_sum keeps the image shape [h0, w0, 1] like the reference's `1 - T`, nerf/renderer.py:911; its train_step flattens it)
        return {"depth": depth.view(*prefix), "image": image.view(*prefix, 3), "weights_sum": 1 - T}

    @torch.no_grad()
    def update_triangles_errors(self, loss):
        """Accumulates the per-pixel loss on the triangle visible at each pixel (nerf/renderer.py:924-943)."""
        indices = self.triangles_errors_id.view(-1).long()
        keep = indices >= 0
        indices = indices[keep].contiguous()
        values = loss.view(-1)[keep].contiguous()
        self.triangles_errors.scatter_add_(0, indices, values)
        self.triangles_errors_cnt.scatter_add_(0, indices, torch.ones_like(values))
        self.triangles_errors_id = None

    @torch.no_grad()
    def mark_unseen_triangles(self, vertices, triangles, mvps, H, W):
        """Faces not hit by any training camera (nerf/renderer.py:947-981)."""
        dev = self.density_bitfield.device
        vertices = torch.as_tensor(vertices).float().to(dev).contiguous()
        triangles = torch.as_tensor(triangles).int().to(dev).contiguous()
        seen = torch.zeros(triangles.shape[0], dtype=torch.bool, device=dev)
        ctx = self.glctx or dr.RasterizeGLContext(output_db=False)
        for mvp in mvps:
            clip = to_clip(vertices, mvp.to(dev)).unsqueeze(0)
            rast, _ = dr.rasterize(ctx, clip, triangles, (H, W))
            ids = rast[..., -1].long().view(-1) - 1
            # reference quirk, kept: `mask[trig_id] += 1` (:973) indexes with -1 for every empty pixel, which names the LAST face --
            # so the last face counts as seen by any view that has background in it
            seen[ids] = True
        return ~seen
