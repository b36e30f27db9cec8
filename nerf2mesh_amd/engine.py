"""Stage-0 step executor: the iteration of trainer.Stage0Trainer's fast path (lego recipe: fused field, packed tables, fused loss, TV
folded into the table backward, FusedAdamAMP) issued as a FIXED sequence of C-ABI launches on preallocated buffers.

Why it exists: with the kernels of this package a training step is ~0.7 ms of GPU work, and the same step driven through
torch.autograd (custom Functions, ~50 tensor allocations, AccumulateGrad, LambdaLR, optimizer hooks) costs the host ~0.85 ms -- the
step was HOST-bound (tools/cpu_bound.py).  The executor keeps PyTorch for what the task statement keeps it for -- device memory,
streams, the random generators and torch.distributed -- and does the rest itself:

  prepare (side stream, for batch i+2):  torch.rand(N, 6) -> n2m_batch_rays (pixels, rays, ground truth, near/far, jitter, background)
        -> n2m_march_rays_train_fused (one march: counts + recorded chunks, replay) -> count to pinned memory + event
  step (main stream, batch i):  n2m_grid_encode_forward_packed[_tvterms: one GPU, the lookup also leaves the backward's TV terms] ->
        n2m_field_forward -> n2m_composite_loss_train (compositing, loss head,
        both backward passes) -> n2m_field_backward [one GPU: the second stage of its dW reduction deferred and carried by the table backward's
        accumulate kernel as rider workgroups] -> n2m_grid_encode_backward_binned_pair (+TV) / ..._pair_tvt -> [world > 1: SUM all-reduce of the
        fixed gradient buffers, fine levels first] -> n2m_adam_step -> n2m_scaler_update_slots

Three layers: engine_batches.BatchPipeline prepares the batches, this module holds the switches, the construction and the step itself
(train_step: one method per phase), engine_adam.AdamPass is the optimizer pass; engine_sdf holds the SDF recipe's step.

Same kernels, same arguments, same random draws in the same order as Stage0Trainer: the two produce the same parameters
(tests/test_engine.py).  What the reference does per iteration is cited there (nerf/utils.py:628-823,1152-1190, main.py:221-241).
Configurations outside the fast path (unfused MLPs, bound > 1 without the packed tables, multi-rank SDF) stay on Stage0Trainer.
"""
import ctypes
import dataclasses
import os

import numpy as np
import torch

from . import _lib as L
from . import synthetic
from .engine_adam import AdamPass, ShardLayout, lr_lambda, peer_chunk_rows  # noqa: F401  (lr_lambda, peer_chunk_rows: names of this module too)
from .engine_batches import BatchPipeline, _RayBufs  # noqa: F401
from .engine_sdf import sdf_buf, step_sdf
from .fused import SHADING, _affine
from .gridencoder import _host_offsets, same_geometry
from .optim import FusedAdamAMP

_p = L.ptr


def _shard_refresh_default():
    from .parallel import shard_refresh_default
    return shard_refresh_default()


@dataclasses.dataclass
class Switches:
    """Every N2M_* switch of the executor with its interlocks, read once at construction (read_switches); the engine carries each field as an
    attribute of the same name.  Measured numbers that are not repeated here: DESIGN.md section 7."""
    # TV terms of the batch as their own kernel on a third stream beside the field kernels (n2m_grid_tv_terms + ..._pair_tvt): takes the
    # stencil's gathers out of the fill (backward 286 -> 250 us) -- but whatever kernel the terms' launch overlaps slows down by about its
    # own 55-95 us (field forward 31 -> 52, compositing 18 -> 50, field backward 59 -> 102: tools/sweep_tv.sh, profiles/r03_tv_split_sweep.txt),
    # so the step LOSES 14-27 us.  Kept as a measured alternative (N2M_TV_SPLIT=1, N2M_TV_AT, N2M_TV_PRIO); off by default.  Same bits.
    tv_prio: int
    tv_split: bool
    tv_at: int                # where the terms' kernel may start: 0 behind the lookup, 1 behind the field forward, 2 behind compositing
    single_pass: bool         # one-launch marcher (A/B: N2M_MARCH_PASSES=2)
    # side-stream go-ahead: 0 before Adam (default), 1 before the table backward, 2 before the field backward, 3 between the table backward's
    # fill and its accumulate (n2m_grid_backward_mid_event).  Measured (round 4, 200 steps): 3 takes the marcher off the lookup (71.4 ->
    # 67.8 us) and off Adam (99 -> 91) but doubles the accumulate beside it (backward 235 -> 301 us): 0.569 -> 0.613 ms/step.
    marker_at: int
    # [round 6, MEASURED AND REJECTED: off by default, N2M_TV_CORNERS=1 turns it on]  The forward lookup leaves, per (hashed level, sample), the
    # density values of corners 000 / 100 / 010 / 001 of the sample's cell (n2m_grid_encode_forward_packed_tv): centre and +x / +y / +z
    # neighbours of the TV stencil the table backward's fill evaluates for the same sample a few kernels later on the same table -- which
    # then gathers three neighbours instead of six.  Why it was built: the fill's fine levels are bound by their XCD's L2 request rate, that
    # stencil is six of their ~8 scattered requests per (sample, level), and an ABLATION build (three gathers, no records: wrong results)
    # ran the backward 20.8 us faster (208.8 -> 188.0 us, step 0.541 -> 0.516 ms).  What the real thing does (profiles/r06_tv_corners.txt,
    # ABBA): backward 210.9 -> 206.8 us, lookup 71.3 -> 77.1 us (46 MB more stores), step 0.5394 -> 0.5431 ms -- the 16-byte record comes
    # from HBM where the three gathers it replaces hit the L2, and requested a tile ahead like the other inputs it costs the fill's 124-VGPR
    # kernel its last registers (122 + 32 bytes of scratch).  Same bits either way (tests/test_tv_corners.py).
    tv_corners: bool
    # [round 6; the default on one GPU, A/B: N2M_TV_FWD=0]  TV terms from the forward lookup: n2m_grid_encode_forward_packed_tvterms leaves the FINISHED term of every
    # (sample, level) -- the stencil's centre and +x / +y / +z values are corners the lookup holds in registers, at most three more rows are
    # gathered -- and the table backward consumes them through n2m_grid_encode_backward_binned_pair_tvt: its fill reads 4 coalesced bytes per
    # (sample, level) instead of gathering six rows inside its tile's dependent chain (what the corner records above could not deliver: they
    # still left three gathers and a 16-byte record in that chain).  Same bits (tests/test_tv_fwd.py).  Measured (profiles/r06_tv_fwd.txt):
    # backward 208 -> 180 us, lookup 72 -> 94 us; lego step -0.7 % over 40-step windows, -1.4 % over 192 steps, -2.0 % in the diffuse phase; garden +-0.
    tv_fwd: bool
    # [round 6, MEASURED AND NOT ADOPTED: off by default, N2M_ADAM_TAIL=1 turns it on]  The scaler / step-count / loss-value bookkeeping behind the
    # optimizer pass as the TAIL of that pass (n2m_adam_step_scaler: one wave of its last workgroup runs the code of n2m_scaler_update_slots
    # once every other wave has left an arrival mark) instead of a one-workgroup launch of its own on the step's critical path (~10 us + the queue gap
    # in front of the next lookup).  Identical bits (tests/test_optim.py, tests/test_adam_tail.py) -- but the optimizer pass takes 136 us instead of 93
    # in the kernel that also holds the bookkeeping code, whatever the arrival scheme: step 0.540 -> 0.563 ms.
    adam_tail: bool
    # [the default on one GPU, A/B: N2M_RIDERS=0]  Rider workgroups: the second stage of the field backward's weight-gradient reduction (a launch of
    # its own between the field backward and the fill, 5 us on the main stream's serial chain) runs as 120 extra workgroups at the end of the
    # accumulate kernel's grid (n2m_field_backward_defer_dw + n2m_grid_backward_dw_rider).  Its inputs are complete when the field backward ends
    # and only the optimizer pass reads its outputs, so nobody waits for anybody; same body, same order, same bits.  Not with SDF, several
    # ranks, --ind_dim or the depth-supervised heads: they keep the separate launch.  (The scaler update was the other candidate and is NOT a
    # rider: the lookup that leaves the TV terms reads the loss scale, so the update has to be over before the lookup starts -- DESIGN 7.)
    riders: bool
    # Live-first sample order for the table backward (round 5; MEASURED AND REJECTED, off by default -- N2M_LIVE_FIRST=1 turns it on).
    # The compositing kernel leaves per ray how many samples precede its early stop -- the others, 48 % of a trained lego batch
    # (profiles/r05_fill_stats.txt), receive exactly zero gradients (raymarching.cu:553,640) and deliver at most a TV term;
    # n2m_sample_order_live_first turns that into a permutation and the fill visits the samples in that order, so that the dead tails fill
    # whole waves, which take a TV-only path (one entry, one value through the run merge, ~30 % of the VALU work).  Same sums (fixed point).
    # Measured (profiles/r05_live_first_ab.txt, table backward per step, kernel with the additions): off 211.1 us | identity order 212.7 | live-first 212.7 | live-first
    # with the TV-only path switched off 218.7: the path saves 6 us, the order costs 7.6 (a ray's live prefix is 5.5 samples: 22-66 byte
    # pieces per gathered input instead of whole lines) + 4 us of order kernel and longer compositing: the fill is bound by its waits
    # (SQ: waiting 0.51 of wave cycles), not by the instructions the dead half of the batch issues.
    live_first: bool
    identity_order: bool      # N2M_LIVE_FIRST=2 (measurement: the order's indirection alone)
    # [experiment, N2M_LOOKUP_OVERLAP=1, single GPU] Adam in two calls by level half -- fine rows first -- and the NEXT step's lookup of the fine
    # levels on a stream of its own behind the first call: the lookup (L2-request bound) beside the optimizer pass of the coarse rows + the MLP
    # weights (HBM-stream bound).  Same bits (Adam is element-wise, the lookup's levels write disjoint rows).  Measured: see DESIGN section 7.
    lookup_overlap: bool
    fill_dbg: object          # N2M_FILL_DBG (measurement switches of the fill, wrong results for most): None or the value for n2m_debug_fill_times
    sdf_fold: bool            # SDF recipe: finite-difference copies folded into the batch's table backward (A/B: N2M_SDF_FOLD=0)
    sdf_tv_all: bool          # SDF recipe, progressive phase: TV of all levels inside the batch's backward (A/B: N2M_SDF_TV_ALL=0)
    # ---- single GPU, measured alternative (N2M_FUSE_ADAM=1, off by default): the optimizer pass of the hashed levels (94 % of the rows)
    # inside the table backward's accumulate kernels (n2m_grid_encode_backward_binned_pair_adam): parameter and moments of both tables
    # exist twice, the flush reads one set and writes the other, and the two sets swap roles after every step -- model.encoder.embeddings
    # .data / optimizer.state always name the current one, so nothing outside the step sees the double buffering.  The TV stencil reads
    # the density column of the packed table.  Same bits as the separate pass (tests/test_engine.py), but the step LOSES 50-85 us: the
    # accumulates are latency-bound work items (2 per CU, barriers between their phases) and move the optimizer's 0.3 GB at a third of the
    # rate the streaming n2m_adam_step reaches (backward 287 -> 399-434 us against Adam 93 -> 15 us; lookup 74 -> 88 us), DESIGN section 7.
    want_fuse_adam: bool
    # ---- multi-GPU
    shard_adam: bool          # optimizer sharded over the ranks where the layout allows it (A/B: N2M_SHARD_ADAM=0)
    # [opt-in, N2M_PEER_STORE=1] the sharded exchange without a collective in the data path (parallel.PeerExchange, include/n2m_peer.h): the
    # table backward's flush stores gradient rows into their owner's staging slots, the owner sums the W slots in rank order, Adam's
    # refreshed packed rows are stored into every rank's packed table; epoch flags instead of reduce-scatter / all-gather.  Tested between
    # two processes on one GPU, never run over xGMI: off by default.
    peer_store: bool
    peer_pad_rows: int        # N2M_PEER_PAD_ROWS: extra padding, a multiple of four -- exercises the uneven layout with two ranks, tests/test_parallel_gpu.py
    peer_fused_wanted: bool   # n2m_adam_step_peer where the layout allows it (A/B: N2M_PEER_FUSED=0)
    chunked_gather: bool      # A/B (N2M_CHUNKED_GATHER=0): wait for both chunks right behind Adam


def read_switches(opt, world_size, ind_dim):
    env = os.environ.get
    one = world_size == 1
    tv_split = env("N2M_TV_SPLIT", "0") == "1"
    tv_corners = env("N2M_TV_CORNERS", "0") == "1" and one and not opt.sdf and opt.lambda_tv > 0 and not tv_split
    return Switches(
        tv_prio=int(env("N2M_TV_PRIO", "0")), tv_split=tv_split, tv_at=int(env("N2M_TV_AT", "0")),
        single_pass=env("N2M_MARCH_PASSES", "1") != "2", marker_at=int(env("N2M_MARKER_AT", "0")), tv_corners=tv_corners,
        tv_fwd=env("N2M_TV_FWD", "1") != "0" and one and not opt.sdf and opt.lambda_tv > 0 and not tv_split and not tv_corners,
        adam_tail=env("N2M_ADAM_TAIL", "0") == "1" and one,
        riders=env("N2M_RIDERS", "1") != "0" and one and not opt.sdf and ind_dim == 0,
        live_first=env("N2M_LIVE_FIRST", "0") not in ("0", ""), identity_order=env("N2M_LIVE_FIRST", "0") == "2",
        lookup_overlap=env("N2M_LOOKUP_OVERLAP", "0") == "1" and one and not opt.sdf and ind_dim == 0,
        fill_dbg=int(env("N2M_FILL_DBG")) if env("N2M_FILL_DBG") else None,
        sdf_fold=env("N2M_SDF_FOLD", "1") != "0", sdf_tv_all=env("N2M_SDF_TV_ALL", "1") != "0",
        want_fuse_adam=one and not opt.sdf and env("N2M_FUSE_ADAM", "0") == "1",
        shard_adam=env("N2M_SHARD_ADAM", "1") != "0", peer_store=env("N2M_PEER_STORE", "0") == "1",
        peer_pad_rows=int(env("N2M_PEER_PAD_ROWS", "0")), peer_fused_wanted=env("N2M_PEER_FUSED", "1") != "0",
        chunked_gather=env("N2M_CHUNKED_GATHER", "1") != "0")


class _Step:
    """What the phases of ONE step share.  Computed once per step and never kept: _fuse_swap, load_state_dict and the EMA swap change
    addresses between steps."""
    __slots__ = ("b", "M", "N", "w", "s", "shading", "xyzs", "dirs", "ts", "dirs_p", "pk", "seed", "geo", "aff", "tv", "wp", "spec_reg",
                 "depth_step", "d_sigma", "d_rgb", "want_tv", "tv_terms", "tv_done", "order", "fused", "backward")


class Stage0Engine:
    def __init__(self, model, opt, poses, device, rank=0, world_size=1, seed=0, ema_decay=0.95, capture=None):
        self.model, self.opt, self.device = model.to(device), opt, torch.device(device)
        # capture (capture.Capture, opt-in): a captured image set instead of the analytic box scene -- its poses, its intrinsics, its uint8
        # bank (n2m_batch_rays reads the bank in the place of the fp32 images), its per-view depth ranges.  None: everything as it was.
        self.capture = capture
        if capture is not None:
            capture.check_device(self.device)
            poses = capture.poses
        self.rank, self.world = rank, world_size
        self._check_supported()
        L.lib()
        self._init_data(poses, seed + rank, ema_decay)
        self._init_switches()
        self._init_gradient_buffers()
        self.batches = BatchPipeline(self, seed + rank, max(8192, self._depth_rays), self.single_pass)
        self._init_shard_layout()
        self._init_peer_exchange()
        self._init_fused_adam_plan()
        self.adam = AdamPass(self)

    # ------------------------------------------------------------------------------------------------ construction
    def _check_supported(self):
        model, opt, capture, world_size = self.model, self.opt, self.capture, self.world
        assert self.device.type == "cuda", "the step executor drives HIP kernels: no CPU path"
        if bool(opt.sdf) and world_size > 1:
            raise ValueError("Stage0Engine runs the SDF recipe on one rank; use trainer.Stage0Trainer for multi-rank SDF training")
        self.ind_dim = int(getattr(opt, "ind_dim", 0))
        if self.ind_dim > 0 and capture is not None and len(capture) > int(opt.ind_num):
            raise ValueError(f"the capture has {len(capture)} views but ind_num is {int(opt.ind_num)}: every view needs a code row")
        if not self.supported(model, opt, capture=capture, world_size=world_size):
            raise ValueError("Stage0Engine covers the fused recipes (fused_mlp, fp16, individual codes only on a capture -- density mode, "
                             "one rank, ind_dim <= 16 --, power-of-two bound, shared encoder geometry); use trainer.Stage0Trainer for "
                             "other configurations")

    def _init_data(self, poses, seed, ema_decay):
        """Cameras, ground truth, optimizer, EMA, schedules and counters."""
        model, opt, dev, capture = self.model, self.opt, self.device, self.capture
        self.poses = poses.to(dev).float().contiguous()
        self.global_step = 0
        self.num_rays = opt.num_rays
        self.optimizer = FusedAdamAMP(model.get_params(opt.lr), eps=1e-15, amp=True)
        # EMA of the parameters (main.py:241: decay 0.95 for stage 0; nerf/utils.py:544-545), updated once per epoch = every len(loader) =
        # number-of-training-views steps (nerf/utils.py:1213-1214); evaluation runs on the averaged weights (averaged_parameters())
        self.ema = None
        self.epoch_len = max(1, int(poses.shape[0]))
        if ema_decay is not None:
            from .ema import ExponentialMovingAverage
            self.ema = ExponentialMovingAverage(model.parameters(), decay=ema_decay)
        self.images = None
        self.scene = getattr(opt, "scene", "lego")
        self.boxes = synthetic.boxes(dev, self.scene)
        # --enable_cam_near_far (main.py:40, config 4): per-view (near, far) from the sparse points, applied by the batch kernel
        self.cam_near_far = synthetic.cam_near_far(self.poses, self.scene) if getattr(opt, "enable_cam_near_far", False) else None
        if capture is not None:
            self.cam_near_far = capture.cam_near_far
        # --enable_sparse_depth: one batch in ten is all keypoints of one view (capture.DepthSchedule, the same sequence as Stage0Trainer's); the
        # ray buffers are sized for the largest view from the start
        from .capture import dense_depth_for, depth_schedule_for
        # --enable_dense_depth: EVERY batch gathers a depth target beside its colour (n2m_batch_rays with the depth bank) and every step runs the depth
        # head with weight 1; N stays num_rays, so these steps steer adaptive_num_rays like plain ones.  One rank is what is tested.
        self.dense_depth = dense_depth_for(capture, opt)
        self.depth_schedule = depth_schedule_for(capture, opt, seed)
        self._depth_rays = 0 if self.depth_schedule is None else int(max(capture.sparse_depth.counts))
        self.samples_seen = self.rays_seen = 0
        self.last_num_points = 0                  # (last_fold_left: set by the first SDF step that folds, tests/test_engine.py reads its absence)
        self._loss_sum = torch.zeros(1, device=dev)
        self.sync = None
        if self.world > 1:
            from .parallel import GradSync
            self.sync = GradSync(model, self.world)
            # occupancy refresh: every rank queries 1 / W of the cells (Morton ranges) and the densities are all-gathered -- the bit field
            # stays the replicated path's, bit for bit (renderer.update_extra_state; A/B: N2M_SHARD_REFRESH=0)
            self.model.refresh_shard = (self.rank, self.world) if _shard_refresh_default() else None

    def _init_switches(self):
        """The N2M_* switches as attributes of their Switches names, the streams they ask for, and the two settings callers change on the instance."""
        dev = self.device
        sw = read_switches(self.opt, self.world, self.ind_dim)
        vars(self).update(dataclasses.asdict(sw))
        self.tv_stream = L.side_stream(dev, slot=3, priority=sw.tv_prio)
        self.split_backward = True            # multi-rank: table backward in two level halves, the first half's all-reduce under the second
        self.overlap = True                   # next batch on the side stream (False: everything on the main stream, same results)
        self.depth = 2                        # batches prepared ahead of the running step
        self._tail_ticket = torch.zeros(64 * 32, dtype=torch.int32, device=dev)       # N2M_TAIL_TICKET_WORDS
        self._mid_events = None
        self._corners_of = None               # (step, M) whose lookup wrote the corner records in w["tv4"]
        if sw.lookup_overlap:
            self.s_lookup = L.side_stream(dev, slot=4)
        if sw.fill_dbg is not None:
            L.call("n2m_debug_fill_times", sw.fill_dbg, None)

    def _init_gradient_buffers(self):
        model, dev = self.model, self.device
        e1 = model.encoder
        self.rows = e1.embeddings.shape[0]
        self.Lv = e1.num_levels
        self.S = float(np.log2(e1.per_level_scale))
        self.H0 = int(e1.base_resolution)
        self.ho = _host_offsets(e1)
        self.aff = _affine(float(model.bound))
        self.mlp_params = [p for m in (model.sigma_net, model.color_net, model.specular_net) for p in m.parameters()]
        assert len(self.mlp_params) == 7
        # persistent gradient buffers: both table gradients are fully rewritten by every backward (overwrite mode); the seven dW live
        # in one flat buffer that is all-zero between steps (the field backward adds into it, the Adam kernel clears it)
        self.g1 = torch.empty(self.rows, 1, dtype=torch.float32, device=dev)
        self.g2 = torch.empty(self.rows, 2, dtype=torch.float16, device=dev)
        self.dw = torch.zeros(sum(p.numel() for p in self.mlp_params), dtype=torch.float32, device=dev)
        self.dw_views, o = [], 0
        for p in self.mlp_params:
            self.dw_views.append(self.dw[o:o + p.numel()])
            o += p.numel()
        self._dw_ptrs = [_p(g) for g in self.dw_views]      # (the buffer lives as long as the engine)
        # per-image codes (--ind_dim): their gradient lives beside the seven dW in a flat buffer of its own, all-zero between steps like
        # `dw` (the *_ind field backward adds into it, the Adam kernel clears it)
        self.dcodes = torch.zeros_like(model.individual_codes.data) if self.ind_dim > 0 else None
        self._ind_ws = None
        self._work_cap = (0, 0)
        self._w = None
        self._n_spec = int(L.lib().n2m_field_spec_partials())
        self._sdf, self._sdf_cap = None, 0

    def _init_shard_layout(self):
        """---- multi-GPU: optimizer sharded over the ranks (ZeRO-1 for the two tables).  Gradient rows are reduce-scattered (fine levels
        first, under the coarse half of the backward), each rank runs Adam on 1/W of the rows and the packed 8-byte rows the forward
        reads are all-gathered: fewer wire bytes than the all-reduce (73.5 + 49 MB against 2 x 73.5) and 1/W of the 540 MB Adam pass.
        Only the packed table stays complete on every rank: the TV stencil reads its density column (n2m_grid_backward_config);
        the fp32 parameter tensors are current inside the own shard only until sync_parameters() gathers them (checkpoint, export)."""
        dev, W = self.device, self.world
        self.shard, self.layout = False, None
        if W > 1:
            import torch.distributed as dist
            split = int(self.ho[8]) if self.Lv == 16 else 0
            fine = self.rows - split
            # (a slice that starts at an odd row -- the coarse half at 8 ranks -- leaves the packed rows 8-byte aligned only: n2m_adam_step then
            # writes the two columns separately instead of whole 16-byte row pairs; tests/test_optim.py covers that form)
            # peer-store mode: coarse chunks padded to a multiple of FOUR rows (the last rank's is shorter), so that every chunk starts 16-byte aligned
            # in the packed table and n2m_adam_step_peer's fused form covers W = 4 and W = 8 too (split / W = 481 390 / 240 695 rows there: not
            # multiples of four, the second one odd); the collective path needs equal chunks (reduce_scatter_tensor) and keeps split / W.
            peer_mode = self.peer_store and not self.opt.sdf
            cs, uneven = split // W, False
            padded = peer_chunk_rows(split, W, self.peer_pad_rows) if peer_mode else None
            if padded is not None:
                cs, even_ok = padded, True
                uneven = cs * W != split
            else:
                even_ok = split % W == 0
            if self.Lv == 16 and even_ok and fine % W == 0 and self.shard_adam:
                self.shard = True
                self.layout = ShardLayout(self.rank, W, split, cs, fine // W, uneven)
                f32 = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
                f16 = lambda *sh: torch.empty(*sh, dtype=torch.float16, device=dev)
                self.g1s = {"c": f32(cs, 1), "f": f32(fine // W, 1)}
                self.g2s = {"c": f16(cs, 2), "f": f16(fine // W, 2)}
                self._inplace_gather = dist.get_backend() == "nccl"      # RCCL gathers in place; gloo (tests) gets a copy of the shard
                self.optimizer.shard_sync = lambda: self.sync_parameters(moments=True)      # state_dict() of a sharded run: gather first
        # per-thread settings of the binned backward, stated before every backward of this engine (train_step): sharded -> the TV stencil
        # reads the density column of the packed table (row stride 2); W ranks -> gradients are SUMMED, so a local fp16 row above max / W
        # raises found_inf already
        self._bwd_cfg = (2 if self.shard else 1, float(W))

    def _init_peer_exchange(self):
        """The peer-store exchange (Switches.peer_store) of a sharded run."""
        self.peer = None
        if self.shard and self.peer_store:
            if self.opt.sdf:
                raise ValueError("N2M_PEER_STORE covers the NeRF recipes (the SDF head's folded backward is not routed)")
            from .parallel import PeerExchange
            model, lay = self.model, self.layout
            self.peer = PeerExchange(self.rank, self.world, self.rows, lay.split, lay.rows_c, lay.rows_f, self.device, small_n=self.dw.numel() + 1)
            self._peer_small = torch.empty(self.dw.numel() + 1, dtype=torch.float32, device=self.device)
            pk = model.packed_tables()
            self.peer.packed.copy_(pk)
            model._packed = self.peer.packed          # same values, exported memory; _packed_key stays valid
            model._packed_buffer = self.peer.packed   # ... and every later rebuild of the copy (load_state_dict, an edited table) lands in it too
            self._peer_route = self.peer.route()
            # n2m_adam_step_peer: the slot sum inside Adam's gradient load, the row push inside its packed-row store (two passes over the rows and
            # four launches fewer per step); covers even splits (rows per rank a multiple of 2, 16-byte aligned slices), else the separate passes
            self._peer_fused = self.peer_fused_wanted and lay.rows_c % 4 == 0 and lay.rows_f % 4 == 0 and lay.split % 2 == 0

    def _init_fused_adam_plan(self):
        """The fused optimizer pass (Switches.want_fuse_adam): which levels the accumulate kernels update themselves."""
        self.fuse_adam = None
        if self.want_fuse_adam and self.Lv == 16:
            fl, fr = ctypes.c_uint32(0), ctypes.c_uint32(0)
            self._fuse_cap = 1 << 19               # samples per batch the plan below holds for (larger batches take the unfused pass)
            L.call("n2m_grid_pair_fuse_plan", self._fuse_cap, self.Lv, self.ho.ctypes.data, ctypes.byref(fl), ctypes.byref(fr))
            if fl.value < self.Lv:
                self.fuse_adam = {"first_level": int(fl.value), "first_row": int(fr.value), "alt": None, "desc": {}}
                self._bwd_cfg = (2, 1.0)

    # ------------------------------------------------------------------------------------------------ configuration
    @staticmethod
    def supported(model, opt, capture=None, world_size=1):
        e1, e2 = model.encoder, model.encoder_color
        sdf = bool(opt.sdf)      # SDF recipe (config 5): NeuS alpha, finite-difference normals, eikonal loss, progressive levels -- engine_sdf.step_sdf
        # per-image codes (--ind_dim): through the *_ind field kernels on a captured set, density mode, one rank, up to fused.ind_max_dim() columns
        from .fused import ind_max_dim
        ind = int(getattr(opt, "ind_dim", 0))
        ind_ok = ind == 0 or (capture is not None and not sdf and world_size == 1 and ind <= ind_max_dim())
        return (bool(getattr(opt, "fused_mlp", False)) and bool(opt.fp16) and ind_ok
                and _affine(float(model.bound)) is not None and same_geometry(e1, e2) and e1.embeddings.shape[1] == 1
                and e2.embeddings.shape[1] == 2 and (sdf or not getattr(opt, "progressive_level", False))
                and opt.patch_size == 1 and not float(getattr(opt, "lambda_patch_ssim", 0) or 0) > 0 and not float(getattr(opt, "lambda_distort", 0) or 0) > 0 and not bool(getattr(opt, "optimize_poses", False)) and (sdf or model.max_level >= e1.num_levels) and not (sdf and opt.lambda_entropy > 0)
                and not (sdf and (getattr(opt, "enable_sparse_depth", False) or getattr(opt, "enable_dense_depth", False))))      # the depth term is built for density mode

    @property
    def loss_acc(self):
        return self._loss_sum

    def _lambda_mask(self):
        """Weight of the mask term; 0 for a capture without an alpha channel (the reference skips the term for 3-channel images, nerf/utils.py:681)."""
        if self.capture is not None and not self.capture.has_alpha:
            return 0.0
        return float(max(self.opt.lambda_mask, 0.0))

    def mark_untrained(self):
        if self.opt.mark_untrained and self.capture is not None:
            self.model.mark_untrained_grid(self.poses, self.capture.intrinsics, cam_near_far=self.cam_near_far)
        elif self.opt.mark_untrained:
            f = synthetic.LEGO_FOCAL
            self.model.mark_untrained_grid(self.poses, (f, f, synthetic.LEGO_HW / 2, synthetic.LEGO_HW / 2), cam_near_far=self.cam_near_far)

    # ------------------------------------------------------------------------------------------------------ buffers
    def _work(self, M, N):
        """Step-local buffers, grow-only (level-major feature layouts are [16, M] with the step's own M as the stride)."""
        cm, cn = self._work_cap
        if M > cm or N > cn:
            # (the ray part never starts below the largest depth batch: no regrowth of the step's workspace at the first depth step)
            cm, cn = max(cm, int(M * 1.25) + 1024), max(cn, int(N * 1.5) + 1024, self._depth_rays)
            dev = self.device
            f = lambda n: torch.empty(n, dtype=torch.float32, device=dev)
            w = self._w = {}
            w["h1"], w["d_h1"] = f(16 * cm), f(16 * cm)
            w["h2"] = torch.empty(32 * cm, dtype=torch.float16, device=dev)
            w["d_h2"] = torch.empty(32 * cm, dtype=torch.float16, device=dev)
            w["sigma"], w["rgb"], w["weights"], w["d_sr"] = f(cm), f(3 * cm), f(cm), f(4 * cm)
            w["tv"] = f(16 * cm)
            # the forward lookup's corner records for the table backward's TV stencil ([16, M, 4] fp32; hashed levels written): see Switches.tv_corners
            w["tv4"] = f(64 * cm) if self.tv_corners else None
            w["spec_partial"] = torch.zeros(self._n_spec, dtype=torch.float32, device=dev)
            w["ws"], w["depth"], w["image"], w["d_image"], w["d_ws"], w["bg"] = f(cn), f(cn), f(3 * cn), f(3 * cn), f(cn), f(3 * cn)
            w["partial"] = f((cn + 3) // 4 + 1)
            w["live"] = torch.zeros(cn, dtype=torch.int32, device=dev)
            w["block_live"] = torch.zeros((cn + 15) // 16 + 1, dtype=torch.int32, device=dev)
            w["perm"] = torch.empty(cm, dtype=torch.int32, device=dev)
            w["sview"] = torch.empty(cm, dtype=torch.int32, device=dev) if self.ind_dim > 0 else None      # code row of every sample
            w["zeros"] = torch.zeros(max(cm, 3 * cn), dtype=torch.float32, device=dev)
            self._work_cap = (cm, cn)
        return self._w

    def _sdf_buf(self, M=0):
        return sdf_buf(self, M)

    # ------------------------------------------------------------------------------------------------- next batch
    def _refresh(self):
        """Occupancy refresh (every 16th step, nerf/utils.py:1155-1156): reads the parameters, so it runs on the main stream behind the
        optimizer update of the step before."""
        if self.sync is not None:
            self.sync.sync_rng_for_grid_update(self.global_step)
        if self.peer is not None:
            self.peer.check()                            # (the refresh drains the queue anyway: a blocking look at the error word)
        if self.shard:
            self.sync_parameters(density_only=True)      # the refresh evaluates the density from the fp32 table: gather the other ranks' rows
        self.model.update_extra_state()

    def _fill_pipeline(self, max_new=None):
        self.batches.fill(max_new)

    def _mid_step_fill(self):
        self.batches.mid_step_fill()

    def _finish(self, b):
        return self.batches.finish(b)

    def _go_ahead(self):
        """ONE event per step on the main stream (an event record is a marker packet the queue idles ~6 us behind, measured): behind the
        last kernel that reads this batch's buffers -- the side stream's go-ahead."""
        ev = torch.cuda.Event()
        ev.record()
        self.batches.go_ahead(ev)

    # ------------------------------------------------------------------------------------------------------- step
    @torch.no_grad()
    def train_step(self):
        st = self._begin_step()
        if self.opt.sdf:
            return self._step_sdf(st)
        dsum = None
        if st.M > 0:
            fwd_terms = self._lookup(st)
            self._mid_step_fill()
            if st.want_tv or fwd_terms:
                st.tv_terms = st.w["tv"]                          # (fwd_terms: written by this step's lookup, on this stream)
            self._start_tv(st, 0)
            self._field_forward(st)
            self._start_tv(st, 1)
        self._head(st)
        if st.M > 0:
            self._start_tv(st, 2)
            if self.marker_at == 2:
                self._go_ahead()
            dsum = self._field_backward(st)
            self._table_backward(st)
            if self.marker_at == 1:
                self._go_ahead()
        self._exchange(st, dsum)
        self._marker(st)
        self._optimizer(st)
        loss = st.b.loss.view(())                 # written by the scaler kernel (photometric + specular terms); lives in the batch's buffer set (valid until the set comes round again)
        self._fill_pipeline()
        return loss

    def _step_sdf(self, st):
        return step_sdf(self, st)

    def _begin_step(self):
        """Takes the step's batch, completes its samples, advances the counters and schedules; returns what the phases share."""
        opt, model = self.opt, self.model
        if not model.training:
            model.train()
        for g in self.optimizer.param_groups:
            g.setdefault("initial_lr", g["lr"])
        st = _Step()
        b = st.b = self.batches.take()
        self.global_step += 1
        assert b.index == self.global_step
        N = st.N = b.N
        st.shading = SHADING["diffuse" if (self.global_step < opt.diffuse_step or opt.diffuse_only) else "full"]
        M = st.M = self._finish(b)
        self.last_num_points = M
        self.samples_seen += M
        self.rays_seen += N
        if opt.sdf:               # schedules of the SDF recipe (nerf/utils.py:651-655), exactly as trainer.Stage0Trainer sets them
            opt.cos_anneal_ratio = min(1, self.global_step / (0.5 * opt.iters))
            opt.normal_anneal_epsilon = 1e-1 * (1 - min(0.999, self.global_step / (0.5 * opt.iters)))
            if opt.progressive_level:
                model.max_level = 4 + int(12 * min(1, self.global_step / (0.5 * opt.iters)))
        w = st.w = self._work(max(M, 1), N)
        st.s = L.stream()
        c = b.cap_m
        st.xyzs = st.dirs = st.ts = None
        if M > 0:
            st.xyzs, st.dirs, st.ts = b.samples[:3 * c], b.samples[3 * c:6 * c], b.samples[6 * c:]
        st.dirs_p = _p(st.dirs) if st.shading != 0 else None
        o = self.optimizer
        st.pk = model.packed_tables()
        if self.lookup_overlap and self.adam.packed is not None and st.pk.data_ptr() != self.adam.packed.data_ptr():
            # the copy was rebuilt just now, on THIS stream (a table was written through torch since the last step: load_state_dict, the EMA
            # swap): the lookup stream's go-ahead is an event of the last optimizer pass and does not cover it -- this step looks up in order
            self.adam.fine_ready = None
        # seed gradient = loss scale [/ world]: gradients are SUMMED over ranks
        st.seed = o.scale if self.world == 1 else o.scale / self.world
        e1 = model.encoder
        st.geo = (e1.gridtype_id, int(bool(e1.align_corners)), e1.interp_id)
        st.aff = (float(self.aff[0]), float(self.aff[1]))
        st.tv = (float(opt.lambda_tv), float(opt.lambda_tv * (10 if opt.bound > 1 else 1)), float(0.5 / model.bound))
        st.wp = [_p(p) for p in self.mlp_params]
        # full shading: the specular regulariser (nerf/utils.py:733-737) rides in the field kernels -- the forward leaves per-workgroup
        # sums of specular^2, the backward adds 2 lambda / M * specular * seed to the recomputed activation's gradient; the [M,3]
        # specular tensor is neither written nor read
        st.spec_reg = st.shading != 0 and opt.lambda_specular > 0
        # depth step (nerf/utils.py:685-705): the same head + the depth term -- the keypoints' depth and weight on a sparse-depth step, the
        # bank's depth with weight 1 (depth_weight NULL) on every step of a dense-depth run.  The loss value: summed by the scaler kernel.
        st.depth_step = b.depth_view is not None or self.dense_depth is not None
        st.d_sigma, st.d_rgb = w["d_sr"][:max(M, 1)], w["d_sr"][max(M, 1):4 * max(M, 1)]
        st.want_tv = opt.lambda_tv > 0 and self.tv_split and self.Lv == 16
        st.tv_terms = st.tv_done = st.fused = st.backward = None
        st.order = False
        return st

    def _lookup(self, st):
        """The forward lookup of both tables, one of five forms.  Returns True when the lookup left the backward's TV terms in w["tv"]."""
        w, M, s, adam = st.w, st.M, st.s, self.adam
        fwd = (_p(st.xyzs), _p(st.pk), _p(self.model.encoder.offsets), _p(w["h1"]), _p(w["h2"]), M, self.Lv, self.Lv, self.S, self.H0, *st.geo, *st.aff)
        levels = self.Lv == 16
        if self.shard and adam.gathers and levels:
            # the packed rows of the other ranks are still arriving: coarse half first, its lookup runs under the fine half's transfer
            adam.wait_gather(("c",))
            L.call("n2m_grid_encode_forward_packed_levels", *fwd, 0, 8, s)
            adam.wait_gather(("f",))
            L.call("n2m_grid_encode_forward_packed_levels", *fwd, 8, 8, s)
        elif self.lookup_overlap and adam.fine_ready is not None and levels:
            # fine levels on their own stream behind the fine half of the last optimizer pass, coarse levels on the main stream behind all of it
            self.s_lookup.wait_event(adam.fine_ready)
            with torch.cuda.stream(self.s_lookup):
                L.call("n2m_grid_encode_forward_packed_levels", *fwd, 8, 8, L.stream())
                done = torch.cuda.Event()
                done.record()
            L.call("n2m_grid_encode_forward_packed_levels", *fwd, 0, 8, s)
            torch.cuda.current_stream(self.device).wait_event(done)
        elif self.tv_corners and levels and self.fuse_adam is None:
            L.call("n2m_grid_encode_forward_packed_tv", *fwd, _p(w["tv4"]), s)
            self._corners_of = (self.global_step, M)          # the records in w["tv4"] belong to THIS step's samples
        elif self.tv_fwd and levels and self.fuse_adam is None:
            # (weights as in the backward's TV arguments; `seed` = the loss scale this step's backward runs under: the scaler's update of the
            #  last step is ahead of this launch on the stream)
            L.call("n2m_grid_encode_forward_packed_tvterms", *fwd, *st.tv, _p(st.seed), _p(w["tv"]), s)
            return True
        else:
            adam.wait_gather()
            L.call("n2m_grid_encode_forward_packed", *fwd, s)
        return False

    def _start_tv(self, st, at):
        """Switches.tv_split, at position `at` (Switches.tv_at) of the step: the TV terms need the samples and the density table only --
        evaluated on their own stream while the field kernels run."""
        if not st.want_tv or self.tv_at != at:
            return
        go = torch.cuda.Event()
        go.record()
        self.tv_stream.wait_event(go)
        L.grid_backward_config(*self._bwd_cfg)
        with torch.cuda.stream(self.tv_stream):
            L.call("n2m_grid_tv_terms", _p(st.xyzs), _p(st.pk) if self._bwd_cfg[0] == 2 else _p(self.model.encoder.embeddings), self.ho.ctypes.data,
                   st.M, self.Lv, self.S, self.H0, *st.geo, *st.tv, _p(st.seed), *st.aff, _p(st.w["tv"]), L.stream())
            st.tv_done = torch.cuda.Event()
            st.tv_done.record()

    def _field_forward(self, st):
        w, M, s = st.w, st.M, st.s
        spec = _p(w["spec_partial"]) if st.spec_reg else None
        if self.ind_dim > 0:
            codes = self.model.individual_codes
            L.call("n2m_field_sample_views", _p(st.b.rays), _p(st.b.views), st.N, M, _p(w["sview"]), s)
            L.call("n2m_field_forward_ind_train", _p(st.xyzs), st.dirs_p, _p(w["h1"]), _p(w["h2"]), *st.wp,
                   _p(codes), _p(w["sview"]), codes.shape[0], codes.shape[1], M, st.shading, 1, _p(w["sigma"]), _p(w["rgb"]), None, spec, s)
        else:
            L.call("n2m_field_forward_train", _p(st.xyzs), st.dirs_p, _p(w["h1"]), _p(w["h2"]), *st.wp, M, st.shading, 1,
                   _p(w["sigma"]), _p(w["rgb"]), None, spec, s)

    def _head(self, st):
        """Compositing + loss head + both backward passes: one launch (+ the entropy regulariser of config 4, nerf/utils.py:728-733: its
        per-sample gradient is the backward's grad_weights).  Sets st.order: the table backward visits the samples live-first."""
        opt, w, b, M, N, s = self.opt, st.w, st.b, st.M, st.N, st.s
        bg_t, bg_s = (b.bg, 0.0) if b.bg is not None else (None, 1.0)
        order = st.order = self.live_first and M > 0 and M <= (1 << 20) and self.peer is None
        head = L.CompositeLoss(sigmas=_p(w["sigma"]), rgbs=_p(w["rgb"]), ts=_p(st.ts), rays=_p(b.rays), M=M, N=N, T_thresh=1e-4, gt_rgba=_p(b.rgba),
                               bg=_p(bg_t), bg_scalar=bg_s, lambda_rgb=float(opt.lambda_rgb), lambda_mask=self._lambda_mask(), grad_loss=_p(st.seed),
                               grad_sigmas=_p(st.d_sigma), grad_rgbs=_p(st.d_rgb), partial=_p(w["partial"]),
                               lambda_entropy=float(max(opt.lambda_entropy, 0.0)),
                               live=_p(w["live"]) if order else None, block_live=_p(w["block_live"]) if order else None)
        if st.depth_step:
            head.gt_depth, head.depth_weight = _p(b.gtd), _p(b.dw) if b.depth_view is not None else None
            head.lambda_depth = float(opt.lambda_depth * min(1.0, self.global_step / 1000))
        L.call("n2m_composite_loss_train", ctypes.addressof(head), s)
        if order:
            L.call("n2m_sample_order_live_first", _p(b.rays), _p(w["live"]), _p(w["block_live"]), N, M, _p(w["perm"]), s)
            if self.identity_order:
                torch.arange(M, dtype=torch.int32, device=self.device, out=w["perm"][:M])

    def _field_backward(self, st):
        """Returns the second stage of the dW reduction (L.DwSum) when the backward deferred it (Switches.riders), else None."""
        opt, w, M, s, o = self.opt, st.w, st.M, st.s, self.optimizer
        spec = (float(2.0 * opt.lambda_specular / M) if st.spec_reg else 0.0, _p(st.seed) if st.spec_reg else None)
        if self.ind_dim > 0:
            codes = self.model.individual_codes
            need = int(L.lib().n2m_field_ind_workspace_bytes(self._work_cap[0], codes.shape[0]))      # grow-only, sized with the step's buffers
            if self._ind_ws is None or self._ind_ws.numel() < need:
                self._ind_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            L.call("n2m_field_backward_ind_train", _p(st.xyzs), st.dirs_p, _p(w["h1"]), _p(w["h2"]), *st.wp,
                   _p(codes), _p(w["sview"]), codes.shape[0], codes.shape[1], M, st.shading, 1, _p(st.d_sigma), _p(st.d_rgb), None, _p(w["d_h1"]),
                   _p(w["d_h2"]), *self._dw_ptrs, _p(self.dcodes), _p(self._ind_ws), self._ind_ws.numel(), _p(o.found_inf), *spec, s)
            return None
        # the backward describes the second stage of its dW reduction in dsum instead of launching it
        dsum = L.DwSum() if self.riders and not st.depth_step and self.fuse_adam is None else None
        with L.thread_locals(dsum is not None and ("n2m_field_backward_defer_dw", ctypes.addressof(dsum))):
            L.call("n2m_field_backward_train", _p(st.xyzs), st.dirs_p, _p(w["h1"]), _p(w["h2"]), *st.wp, M, st.shading, 1,
                   _p(st.d_sigma), _p(st.d_rgb), None, _p(w["d_h1"]), _p(w["d_h2"]), *self._dw_ptrs, _p(o.found_inf), *spec, s)
        return dsum if dsum is not None and dsum.partial else None

    def _table_backward(self, st):
        """Chooses the table backward's entry point -- the fused optimizer pass (st.fused: its N2mAdamFuse), the TV terms somebody left in
        w["tv"], or the plain call with the stencil inside -- and leaves (entry, arguments) in st.backward for _backward()."""
        opt, w, M, o = self.opt, st.w, st.M, self.optimizer
        L.grid_backward_config(*self._bwd_cfg)
        ho = self.ho.ctypes.data
        ws = L.workspace(self.device, L.lib().n2m_grid_binned_pair_workspace_bytes(M, self.Lv, ho))
        tv = opt.lambda_tv > 0
        common = (_p(w["d_h1"]), _p(w["d_h2"]), _p(st.xyzs), ho, _p(self.g1), _p(self.g2), M, self.Lv, self.Lv, self.S, self.H0, *st.geo)
        tail = (_p(o.found_inf), *st.aff, 1, _p(ws), ws.numel(), st.s)
        if self.fuse_adam is not None and M <= self._fuse_cap and st.tv_terms is None:
            self.adam.desc(st.shading != 0, dense_only=True)             # (names adam.packed)
            st.fused = self.adam.fuse_desc(lr_lambda(self.global_step - 1, opt.iters))
        if st.fused is not None:
            st.backward = ("n2m_grid_encode_backward_binned_pair_adam",
                           (*common, _p(st.pk) if tv else None, *st.tv, _p(st.seed) if tv else None, *tail[:3], _p(ws), ws.numel(),
                            ctypes.addressof(st.fused), st.s))
        elif st.tv_terms is not None:
            if st.tv_done is not None:
                torch.cuda.current_stream(self.device).wait_event(st.tv_done)
            st.backward = ("n2m_grid_encode_backward_binned_pair_tvt", (*common, _p(st.tv_terms), *tail))
        else:
            table = st.pk if self._bwd_cfg[0] == 2 else self.model.encoder.embeddings
            st.backward = ("n2m_grid_encode_backward_binned_pair", (*common, _p(table) if tv else None, *st.tv, _p(st.seed) if tv else None, *tail))

    def _backward(self, st, half):
        """The table backward of level half `half` (0: all levels, 1: fine, 2: coarse); nothing for a batch without samples."""
        if st.backward is None:
            return
        entry, args = st.backward
        # (live-first order: set right in front of the call it is meant for)
        with L.thread_locals(st.order and st.fused is None and ("n2m_grid_backward_sample_order", _p(st.w["perm"]))):
            if st.fused is not None or half == 0 and st.tv_terms is None:
                L.call(entry, *args)
            elif st.tv_terms is not None:
                L.call(entry, *args, half)
            else:
                L.call(entry + "_half", *args, half)

    def _backward_whole(self, st, dsum):
        """One GPU (or an unsplit multi-rank backward): all levels in one call, with what rides on it -- the mid-backward go-ahead event
        (Switches.marker_at 3), the lookup's corner records (Switches.tv_corners) and the deferred dW sum (Switches.riders)."""
        w = st.w
        mid = self.marker_at == 3 and st.fused is None and st.tv_terms is None
        if mid:
            if self._mid_events is None:          # a few events, created (= recorded once) up front, re-recorded by the library
                self._mid_events = [torch.cuda.Event() for _ in range(4)]
                for e in self._mid_events:
                    e.record()
            ev = self._mid_events[self.global_step % len(self._mid_events)]
            L.call("n2m_grid_backward_mid_event", ctypes.c_void_p(ev.cuda_event))
        use_corners = (self.tv_corners and st.fused is None and st.tv_terms is None and self.opt.lambda_tv > 0
                       and self._corners_of == (self.global_step, st.M))      # ... and only if THIS step's forward wrote them
        carried = ctypes.c_int(0)
        # (the rider is a one-shot thread-local of the library, like the event above: the accumulate takes the dW sum along)
        with L.thread_locals(use_corners and ("n2m_grid_backward_tv_corners", _p(w["tv4"])),
                             dsum is not None and ("n2m_grid_backward_dw_rider", ctypes.addressof(dsum), ctypes.byref(carried))):
            self._backward(st, 0)
        if mid:
            self.batches.go_ahead(ev)
        if dsum is not None and not carried.value:
            # the table backward took a path without the rider kernel (few samples: the tile-major path): the sum as the launch it always was
            L.call("n2m_field_dw_sum", ctypes.addressof(dsum), st.s)

    def _reduce_scatter(self, h):
        """SUM reduce-scatter of level half h ("f" / "c") of both table gradients into this rank's slices; returns the two work handles."""
        import torch.distributed as dist
        sp = self.layout.split
        rows = slice(sp, None) if h == "f" else slice(None, sp)
        rs = lambda out, src: dist.reduce_scatter_tensor(out.view(-1), src.view(-1), op=dist.ReduceOp.SUM, async_op=True)
        return [rs(self.g1s[h], self.g1[rows]), rs(self.g2s[h], self.g2[rows])]

    def _exchange(self, st, dsum):
        """The table backward with the gradient exchange of its mode around it: peer stores, reduce-scatter (sharded optimizer), all-reduce
        in two level halves, or none.  A batch without samples has zero gradients and no backward (st.backward is None) and takes part in the
        same collectives in the same ORDER as the ranks that have samples (fine halves, coarse halves, then the small bucket)."""
        o, sync, peer = self.optimizer, self.sync, self.peer
        empty = st.M == 0
        if empty:
            self.g1.zero_()
            self.g2.zero_()
        early = None
        if peer is not None and empty:      # zeros into this rank's slots -- once every owner's rows of the last step have arrived (see PeerExchange)
            self.adam.wait_gather()
            peer.begin_step()
            peer.zero_slots()
        elif peer is not None:
            # the flush of each level half stores its rows into their owners' slots; the signal behind it is the whole exchange
            peer.begin_step()
            with L.thread_locals(("n2m_grid_backward_peer_route", ctypes.byref(self._peer_route))):
                self._backward(st, 1)
                peer.signal_grad("f")
                self._backward(st, 2)
                peer.signal_grad("c")
        elif self.shard:
            self._backward(st, 1)
            early = self._reduce_scatter("f")          # fine rows: exchanged under the coarse half
            self._backward(st, 2)
            early += self._reduce_scatter("c")
        elif sync is not None and self.split_backward and self.Lv == 16:
            # multi-GPU: the table backward in two halves of the levels.  The rows of the fine half (levels 8..15: 68 % of the
            # bytes) are final after the first call; their SUM all-reduce runs on the collective stream while the coarse half is
            # still being computed, so most of the exchange hides behind the backward's own tail (at 0.75 ms per step
            # a 49 MB all-reduce no longer is the "< 4 %" the survey estimated at 26 ms per step)
            split = int(self.ho[8])
            self._backward(st, 1)
            early = sync.all_reduce_sum_begin([self.g1[split:], self.g2[split:]], [])
            self._backward(st, 2)
        elif not empty:
            self._backward_whole(st, dsum)
        # ---- [multi-GPU] one SUM all-reduce per fixed gradient buffer (the colour table's stays fp16) + the small bucket
        if peer is not None:
            # no collective anywhere in the step: weight gradients + non-finite flag go to every rank's slot and are summed in rank order
            # everywhere; then, owner side, the W gradient slots of each level half -> their sum where the reduce-scatter would have put it
            n_dw = self.dw.numel()
            torch.cat([self.dw, o.found_inf.reshape(-1)], out=self._peer_small)
            peer.all_sum_small(self._peer_small)
            self.dw.copy_(self._peer_small[:n_dw])
            o.found_inf.copy_(self._peer_small[n_dw:].view_as(o.found_inf))
            for h in ("f", "c"):
                if self._peer_fused:
                    peer.wait_grad(h)                    # (the sum itself happens in n2m_adam_step_peer's gradient load)
                else:
                    peer.reduce(h, self.g1s[h], self.g2s[h])
            # a wait that ran into its timeout has summed stale slots: the step is skipped on the device (found_inf) and the host raises as
            # soon as it sees the error word (one step later at most: the word travels to pinned memory behind the step's last wait)
            peer.fold_error_into(o.found_inf)
            peer.raise_if_failed()
        elif self.shard:
            token = sync.all_reduce_sum_begin([], [self.dw, o.found_inf])
            for work in early:
                work.wait()
            sync.all_reduce_sum_end(token)
        elif sync is not None:
            if early is not None:
                split = int(self.ho[8])
                token = sync.all_reduce_sum_begin([self.g1[:split], self.g2[:split]], [self.dw, o.found_inf])
                sync.all_reduce_sum_end(early)
            else:
                token = sync.all_reduce_sum_begin([self.g1, self.g2], [self.dw, o.found_inf])
            sync.all_reduce_sum_end(token)

    def _marker(self, st):
        """The side stream's go-ahead in front of the optimizer update, unless the step has given it earlier (Switches.marker_at)."""
        if self.marker_at == 0 or st.M == 0 or (self.marker_at == 3 and not (self.sync is None and st.fused is None and st.tv_terms is None)):
            self._go_ahead()

    def _optimizer(self, st):
        """Adam + loss-scale bookkeeping, LR schedule (main.py:239)."""
        extra = (st.w["spec_partial"], float(self.opt.lambda_specular / st.M)) if st.M > 0 and st.spec_reg else None
        self._lr_step(st.shading != 0, loss_out=(st.N, st.b.loss, extra), fused=st.fused)

    def _lr_step(self, full, loss_out=None, fused=None):
        if full is not None:
            self.adam.step(full, lr_lambda(self.global_step - 1, self.opt.iters), loss_out, fused)
        if self.ema is not None and self.global_step % self.epoch_len == 0:      # end of an epoch (nerf/utils.py:1213-1214)
            self.ema_update()

    @torch.no_grad()
    def sync_parameters(self, density_only=False, moments=False):
        """Sharded optimizer: bring the fp32 parameter tensors of both tables up to date on every rank (each rank owns 1/W of the
        rows; the training step itself only needs the packed copy).  Called before the occupancy refresh (density table, every 16
        steps: 24.5 MB) and to be called before a checkpoint, an export, an evaluation or a comparison."""
        self.adam.sync_parameters(density_only, moments)

    def ema_update(self):
        """One update of the averaged weights from the current parameters (one launch, stream-ordered behind the optimizer pass)."""
        if self.shard:
            self.sync_parameters()          # each rank has advanced its own rows of the fp32 tables only (a collective, at a symmetric step)
        self.ema.update()

    # ------------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """Everything the next train_step() depends on, under the reference's checkpoint keys (nerf/utils.py:1345-1365) plus "n2m": each layer
        names the state it owns -- the model, optimizer and EMA theirs, `batches` the pipeline's, this class its counters.  A fresh engine
        built with the same arguments continues bit for bit after load_state_dict() (tests/test_checkpoint_engine_gpu.py).  COLLECTIVE when
        the optimizer is sharded (optimizer.state_dict() gathers the moments)."""
        from . import checkpoint
        self.sync_parameters()
        sd = checkpoint.stage0_state(self)
        sd["n2m"].update(driver="Stage0Engine", batches=self.batches.state_dict())
        if hasattr(self, "last_fold_left"):
            sd["n2m"]["last_fold_left"] = int(self.last_fold_left)
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd, model_only=False):
        """model_only: the model, the averaged weights and mean_density alone (the reference's rule, nerf/utils.py:1446-1447)."""
        from . import checkpoint
        if self.world > 1:
            raise NotImplementedError("loading a checkpoint into a multi-rank engine (the packed rows and shards of every rank would have to follow)")
        torch.cuda.synchronize(self.device)
        checkpoint.load_stage0_state(self, sd, model_only)
        if model_only:
            return
        n2m = sd.get("n2m", {})
        self.batches.load_state_dict(checkpoint.batch_state(sd))
        self.adam.reset()
        # gradient buffers are all-zero between steps (the optimizer pass clears them); nothing of an interrupted step may survive
        self.dw.zero_()
        if self.dcodes is not None:
            self.dcodes.zero_()
        if self._sdf is not None:
            self._sdf["d_var"].zero_()
            self._sdf["fold_cnt"].zero_()
        self._corners_of = None
        if "last_fold_left" in n2m:
            self.last_fold_left = int(n2m["last_fold_left"])
        elif hasattr(self, "last_fold_left"):
            del self.last_fold_left

    def averaged_parameters(self):
        """Context: the model carries the EMA weights (store / copy_to ... restore, nerf/utils.py:1250-1252,1340-1341); no-op without EMA."""
        import contextlib
        if self.ema is None:
            return contextlib.nullcontext()
        self.sync_parameters()
        return self.ema.average_parameters()

    @torch.no_grad()
    def eval_psnr(self, cam=0, downscale=4, use_ema=False, capture=None):
        """use_ema: evaluate the averaged weights, as the reference's evaluate_one_epoch does (nerf/utils.py:1250-1252).  capture: the set the view
        is taken from (default: the training capture, if there is one) -- a held-out split, for instance."""
        from .trainer import Stage0Trainer
        self.sync_parameters()
        if use_ema and self.ema is not None:
            with self.averaged_parameters():
                return Stage0Trainer.eval_psnr(self, cam, downscale, capture=capture)
        return Stage0Trainer.eval_psnr(self, cam, downscale, capture=capture)
